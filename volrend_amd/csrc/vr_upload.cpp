// vr_upload.cpp -- tree upload, clone and free (include/volrend_hip.h): the topology check and
// node renumbering on the host, the staged host-to-device copy pipeline, the quantised decode.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "vr_host.h"

namespace {

// Walks the child links from the root: every link must land on a node that has
// not been reached before (a tree, not a DAG / cycle), inside [1, capacity).
// Returns the deepest leaf level or -1.  A malformed file would otherwise make
// the device descent loop forever.
// level[n] = depth of node n (root 0), 255 = not reachable from the root.
int validate_topology(const int32_t* child, int64_t cap, int N3, std::vector<uint8_t>& level,
                      char* why, size_t why_len) {
    if (cap <= 0) {
        snprintf(why, why_len, "capacity must be positive");
        return -1;
    }
    // Fast path: files written breadth- or depth-first link every child FORWARD (to a higher
    // index), and then one sweep in index order sees every parent before its children -- no
    // queue, sequential reads (a 2 M-node tree: ~20 ms instead of ~50).  The first backward link
    // abandons the sweep for the general walk below.
    {
        level.assign((size_t)cap, 255);
        level[0] = 0;
        int depth = 0;
        bool forward_only = true;
        for (int64_t n = 0; n < cap && forward_only; ++n) {
            const uint8_t ln = level[(size_t)n];
            if (ln == 255) continue;  // not reachable (so far: decided for good if all links go forward)
            const int32_t* c = child + n * N3;
            for (int s = 0; s < N3; ++s) {
                const int64_t skip = c[s];
                if (skip == 0) continue;
                const int64_t m = n + skip;
                if (m <= n) {
                    forward_only = false;
                    break;
                }
                if (m >= cap) {
                    snprintf(why, why_len, "node %lld slot %d links outside the tree (%lld)",
                             (long long)n, s, (long long)m);
                    return -1;
                }
                if (level[(size_t)m] != 255) {
                    snprintf(why, why_len, "node %lld is linked twice (cycle or DAG)", (long long)m);
                    return -1;
                }
                if (ln + 1 > 60) {
                    snprintf(why, why_len, "tree deeper than 60 levels");
                    return -1;
                }
                level[(size_t)m] = (uint8_t)(ln + 1);
                if (ln + 1 > depth) depth = ln + 1;
            }
        }
        if (forward_only) return depth;
    }
    std::vector<uint8_t> seen((size_t)cap, 0);
    level.assign((size_t)cap, 255);
    level[0] = 0;
    std::vector<int64_t> cur{0}, next;
    seen[0] = 1;
    int depth = 0;
    for (;;) {
        next.clear();
        for (int64_t n : cur) {
            const int32_t* c = child + n * N3;
            for (int s = 0; s < N3; ++s) {
                const int64_t skip = c[s];
                if (skip == 0) continue;
                const int64_t m = n + skip;
                if (m <= 0 || m >= cap) {
                    snprintf(why, why_len, "node %lld slot %d links outside the tree (%lld)",
                             (long long)n, s, (long long)m);
                    return -1;
                }
                if (seen[(size_t)m]) {
                    snprintf(why, why_len, "node %lld is linked twice (cycle or DAG)", (long long)m);
                    return -1;
                }
                seen[(size_t)m] = 1;
                level[(size_t)m] = (uint8_t)(depth + 1);
                next.push_back(m);
            }
        }
        if (next.empty()) break;
        if (++depth > 60) {
            snprintf(why, why_len, "tree deeper than 60 levels");
            return -1;
        }
        cur.swap(next);
    }
    return depth;
}

// New node numbering: pre-order depth-first from the root (children in slot order), so a
// subtree is one contiguous run of the arrays.  Exception for the lookup structure (N == 2,
// G0 > 0): behind an internal node of level G0 (a brick root) come first ALL its descendants of
// the next BL - 1 levels, breadth-first (<= 8 + 64 nodes: a brick entry names the parent of its
// leaf as root + delta), and only then the subtrees hanging below level G0 + BL - 1, each
// depth-first.  Unreachable nodes keep their relative order behind the reachable ones.
// brick_roots receives the new indices of the level-G0 internal nodes (ascending).
std::vector<int32_t> node_permutation(const int32_t* child, int64_t cap, int N3, int G0, int BL,
                                      const std::vector<uint8_t>& level,
                                      std::vector<int32_t>& brick_roots) {
    std::vector<int32_t> perm((size_t)cap, -1);
    brick_roots.clear();
    int32_t next = 0;
    std::vector<int64_t> stack{0}, ring, ring_next;
    while (!stack.empty()) {
        const int64_t n = stack.back();
        stack.pop_back();
        perm[(size_t)n] = next++;
        const int32_t* c = child + n * N3;
        if (G0 > 0 && level[(size_t)n] == G0) {
            brick_roots.push_back(perm[(size_t)n]);
            // levels G0+1 .. G0+BL-1 breadth-first right behind the root
            ring.assign(1, n);
            for (int k = 1; k < BL; ++k) {
                ring_next.clear();
                for (int64_t m : ring)
                    for (int s = 0; s < N3; ++s)
                        if (child[m * N3 + s] != 0) {
                            const int64_t ch = m + child[m * N3 + s];
                            perm[(size_t)ch] = next++;
                            ring_next.push_back(ch);
                        }
                ring.swap(ring_next);
            }
            // `ring` = the nodes of level G0+BL-1: their children start ordinary subtrees
            for (size_t i = ring.size(); i-- > 0;) {
                const int64_t m = ring[i];
                for (int s = N3 - 1; s >= 0; --s)
                    if (child[m * N3 + s] != 0) stack.push_back(m + child[m * N3 + s]);
            }
            continue;
        }
        for (int s = N3 - 1; s >= 0; --s)  // reversed: slot 0 is visited first
            if (c[s] != 0) stack.push_back(n + c[s]);
    }
    for (int64_t i = 0; i < cap; ++i)
        if (perm[(size_t)i] < 0) perm[(size_t)i] = next++;
    return perm;
}

// ---------------------------------------------------------------------------
// Host -> device copies of the tree arrays at link speed.  hipMemcpy from pageable memory
// stages through ONE thread's memcpy (~9 GB/s measured: 1.67 GB in 0.19 s); here up to
// kCopyWorkersMax threads each stream chunks through two pinned slots of their own: memcpy into
// slot (i & 1) while the DMA of the previous chunk drains slot (i & 1) ^ 1 (with the source pages
// mapped ahead of time -- prefault_host_range -- 8 threads keep the link busy: 36-45 GB/s
// measured; without, the memcpy is page-fault bound at ~20).  All the DMAs go to
// ONE stream per device (creating a stream costs milliseconds -- an HSA queue -- and the link is
// the shared resource anyway); that stream and the pinned slots (with their events) live in a
// process-wide cache, so only the first upload of a process pays for them.  Chunks are claimed
// dynamically across all segments of a call.  Anything small, or any failure to set the pipeline
// up, falls back to the plain blocking copy.  VR_UPLOAD_TIMING=1 prints the phases.
// ---------------------------------------------------------------------------
constexpr size_t kCopyChunk = 2u << 20;  // (pinned memory costs ~0.5 ms per MB to allocate: 8 workers x 2 slots = 32 MB)
constexpr int kCopyWorkersMax = 4;  // (with the pages mapped ahead, 4 memcpy threads fill the link; every slot is 2 MB of pinned memory to allocate)

struct CopySegment {
    void* dst;
    const void* src;
    size_t bytes;
};
struct PinnedSlot {
    void* mem = nullptr;
    hipEvent_t done = nullptr;  // the last DMA out of this slot
    bool used = false;
};
struct UploadCache {
    static constexpr int kDevices = 16;
    std::mutex mu;
    // per DEVICE: a slot's event belongs to the device that was current when it was created, and
    // recording it on another device's stream is an error
    std::vector<PinnedSlot> free_slots[kDevices];
    hipStream_t stream[kDevices] = {};  // per device, created on first use
    // (call with `device` current)
    bool take(PinnedSlot& out, int device) {
        if (device < 0 || device >= kDevices) return false;
        {
            std::lock_guard<std::mutex> g(mu);
            if (!free_slots[device].empty()) {
                out = free_slots[device].back();
                out.used = false;
                free_slots[device].pop_back();
                return true;
            }
        }
        PinnedSlot sl;
        if (hipHostMalloc(&sl.mem, kCopyChunk, hipHostMallocPortable) != hipSuccess ||
            hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (sl.mem) (void)hipHostFree(sl.mem);
            return false;
        }
        out = sl;
        return true;
    }
    void give(const PinnedSlot& sl, int device) {
        std::lock_guard<std::mutex> g(mu);
        free_slots[device].push_back(sl);
    }
    // the stream and 2 x kCopyWorkersMax slots up front (first upload of the process)
    void warm(int device) {
        (void)stream_of(device);
        std::vector<PinnedSlot> got;
        for (int i = 0; i < 2 * kCopyWorkersMax; ++i) {
            PinnedSlot sl;
            if (!take(sl, device)) break;
            got.push_back(sl);
        }
        for (const PinnedSlot& sl : got) give(sl, device);
    }
    hipStream_t stream_of(int device) {
        std::lock_guard<std::mutex> g(mu);
        if (device < 0 || device >= kDevices) return nullptr;
        if (!stream[device] &&
            hipStreamCreateWithFlags(&stream[device], hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            stream[device] = nullptr;
        }
        return stream[device];
    }
};
UploadCache& upload_cache() {
    static UploadCache* c = new UploadCache();  // never destroyed: no HIP calls at exit
    return *c;
}

// Maps the pages of a host range into this process ahead of the staged copy (tree files are
// handed over as views of an mmap'ed npz: every 4 KB page of the 1.6 GB costs a minor fault the
// first time a copy worker reads it, and the copy is fault-bound).  Runs on a few threads while
// the HIP runtime starts up; best effort, no effect on results.
void prefault_host_range(const void* ptr, size_t bytes) {
    if (!ptr || bytes < (64u << 20)) return;
    const unsigned hw = std::thread::hardware_concurrency();
    const int n_thr = hw >= 32 ? 8 : (hw >= 8 ? 4 : 1);
    const uintptr_t page = 4096;
    const uintptr_t lo = (reinterpret_cast<uintptr_t>(ptr) + page - 1) & ~(page - 1);
    const uintptr_t hi = (reinterpret_cast<uintptr_t>(ptr) + bytes) & ~(page - 1);
    if (hi <= lo) return;
    const uintptr_t per = ((hi - lo) / n_thr + page - 1) & ~(page - 1);
    auto work = [=](int i) {
        const uintptr_t a = lo + per * (uintptr_t)i, b = a + per < hi ? a + per : hi;
        if (a >= b) return;
        // (one read per page, not madvise(MADV_POPULATE_READ): the bulk call holds the process's
        // mmap lock for its whole range and the HIP runtime's own mappings -- start-up, every
        // allocation -- queue up behind it; single faults take the per-VMA lock only)
        volatile unsigned char sink = 0;
        for (uintptr_t q = a; q < b; q += page) sink = sink + *reinterpret_cast<const volatile unsigned char*>(q);
        (void)sink;
    };
    std::vector<std::thread> pool;
    try {
        for (int i = 1; i < n_thr; ++i) pool.emplace_back(work, i);
    } catch (...) {
    }
    work(0);
    for (auto& t : pool) t.join();
}

hipError_t staged_h2d_multi(const CopySegment* seg, int n_seg, int device) {
    const auto t0 = std::chrono::steady_clock::now();
    size_t total = 0, n_chunks = 0;
    std::vector<size_t> first_chunk((size_t)n_seg + 1, 0);
    for (int i = 0; i < n_seg; ++i) {
        first_chunk[(size_t)i] = n_chunks;
        n_chunks += (seg[i].bytes + kCopyChunk - 1) / kCopyChunk;
        total += seg[i].bytes;
    }
    first_chunk[(size_t)n_seg] = n_chunks;
    auto plain = [&]() {
        for (int i = 0; i < n_seg; ++i)
            if (seg[i].bytes) {
                const hipError_t e = hipMemcpy(seg[i].dst, seg[i].src, seg[i].bytes, hipMemcpyHostToDevice);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    };
    const unsigned hw = std::thread::hardware_concurrency();
    int workers = hw >= 8 ? kCopyWorkersMax : (hw >= 4 ? 2 : 1);
    if ((size_t)workers > n_chunks) workers = (int)n_chunks;
    hipStream_t st = (total >= (32u << 20) && workers >= 2) ? upload_cache().stream_of(device) : nullptr;
    if (!st) return plain();
    std::atomic<int> failed{0};
    std::atomic<size_t> next{0};
    auto work = [&]() {
        PinnedSlot slot[2];
        bool ok = hipSetDevice(device) == hipSuccess && upload_cache().take(slot[0], device) &&
                  upload_cache().take(slot[1], device);
        // chunks are claimed dynamically (a worker that was scheduled late does not hold the others up)
        for (int k = 0; ok; k ^= 1) {
            const size_t c = next.fetch_add(1);
            if (c >= n_chunks) break;
            int si = 0;
            while (c >= first_chunk[(size_t)si + 1]) ++si;
            const size_t off = (c - first_chunk[(size_t)si]) * kCopyChunk;
            const size_t len = seg[si].bytes - off < kCopyChunk ? seg[si].bytes - off : kCopyChunk;
            if (slot[k].used) ok = hipEventSynchronize(slot[k].done) == hipSuccess;  // its last DMA is done
            if (!ok) break;
            memcpy(slot[k].mem, static_cast<const char*>(seg[si].src) + off, len);
            ok = hipMemcpyAsync(static_cast<char*>(seg[si].dst) + off, slot[k].mem, len,
                                hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipEventRecord(slot[k].done, st) == hipSuccess;
            slot[k].used = ok;  // (only a RECORDED event may be waited for)
        }
        // A failed enqueue / record may have left a DMA out of a slot in flight with no event to
        // wait for: drain the stream before the slots go back to the cache.
        if (!ok) (void)hipStreamSynchronize(st);
        for (auto& sl : slot) {
            if (!sl.mem) continue;
            if (sl.used && hipEventSynchronize(sl.done) != hipSuccess) ok = false;  // before the slot is reused
            upload_cache().give(sl, device);
        }
        if (!ok) failed.store(1);
    };
    std::vector<std::thread> pool;
    try {
        for (int w = 1; w < workers; ++w) pool.emplace_back(work);
    } catch (...) {  // could not start (all) helpers: this thread copies what is left
    }
    work();
    for (auto& t : pool) t.join();
    if (failed.load()) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(st);
        return plain();  // plain copy of everything
    }
    if (getenv("VR_UPLOAD_TIMING")) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[volrend_hip] staged H2D: %.1f MB in %d segments, %d workers, %.1f ms (%.1f GB/s)\n",
                total / 1e6, n_seg, workers, ms, total / ms / 1e6);
    }
    return hipSuccess;
}

// Joins a helper thread on every way out of a scope; `release` first lets a thread waiting on it
// (0: the topology check is still running) go: an early exit must not leave it waiting.
struct Joiner {
    std::thread& th;
    std::atomic<int>* release = nullptr;
    ~Joiner() {
        int pending = 0;
        if (release) release->compare_exchange_strong(pending, -1);
        if (th.joinable()) th.join();
    }
};

// Validates the codebook arrays of a quantised tree against the tree description.
int check_quant(const VrTreeDesc* d, const VrQuantDesc* q) {
    if (q->n_quant < 0 || q->n_retained < 0 || q->n_quant + q->n_retained < 1)
        return fail(VR_ERR_INVALID_ARGUMENT, "quantised tree needs at least one basis function");
    if (3 * (q->n_quant + q->n_retained) + 1 > d->data_dim)
        return fail(VR_ERR_INVALID_ARGUMENT, "%d quantised + %d retained basis functions do not "
                    "fit data_dim=%d", q->n_quant, q->n_retained, d->data_dim);
    if (!q->sigma) return fail(VR_ERR_INVALID_ARGUMENT, "sigma is NULL");
    if (q->n_quant && (!q->quant_colors || !q->quant_map))
        return fail(VR_ERR_INVALID_ARGUMENT, "quant_colors/quant_map is NULL");
    if (q->n_retained && !q->data_retained)
        return fail(VR_ERR_INVALID_ARGUMENT, "data_retained is NULL");
    return VR_OK;
}

// Stages the codebook arrays on the device (unless they are there already) and decodes
// them into `d_data` (flat reference layout, n_slots * data_dim halfs, device memory).
hipError_t decode_quant_on_device(const VrTreeDesc* d, const VrQuantDesc* q, size_t n_slots,
                                  uint16_t* d_data, int device) {
    const void* src[4] = {q->quant_colors, q->quant_map, q->sigma, q->data_retained};
    const size_t sz[4] = {(size_t)q->n_quant * 65536 * 3 * sizeof(uint16_t), (size_t)q->n_quant * n_slots * sizeof(uint16_t),
                          n_slots * sizeof(uint16_t), (size_t)q->n_retained * n_slots * 3 * sizeof(uint16_t)};
    DeviceBuffer tmp[4];
    const void* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    CopySegment segs[4];
    int n_seg = 0;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) {
        if (!sz[i]) continue;
        if (d->memory == 1) {
            dev[i] = src[i];
            continue;
        }
        e = tmp[i].alloc(sz[i]);
        segs[n_seg++] = CopySegment{tmp[i].get(), src[i], sz[i]};
        dev[i] = tmp[i].get();
    }
    if (e == hipSuccess && n_seg) e = staged_h2d_multi(segs, n_seg, device);
    if (e == hipSuccess)
        e = vr::launch_decode_quant((const uint16_t*)dev[0], (const uint16_t*)dev[1],
                                    (const uint16_t*)dev[2], (const uint16_t*)dev[3], d_data,
                                    (int64_t)n_slots, q->n_quant, q->n_retained, d->data_dim,
                                    nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

int check_tree_desc(const VrTreeDesc* d, bool need_data) {
    if (!d->child || (need_data && !d->data))
        return fail(VR_ERR_INVALID_ARGUMENT, "child/data is NULL");
    if (d->N < 2 || d->N > 16) return fail(VR_ERR_INVALID_ARGUMENT, "N=%d out of range", d->N);
    if (d->capacity <= 0) return fail(VR_ERR_INVALID_ARGUMENT, "capacity must be positive");
    if (d->format < VR_FORMAT_RGBA || d->format > VR_FORMAT_ASG)
        return fail(VR_ERR_INVALID_ARGUMENT, "unknown data format %d", d->format);
    const int min_dim = d->format == VR_FORMAT_RGBA ? 4 : 3 * d->basis_dim + 1;
    if (d->format != VR_FORMAT_RGBA && (d->basis_dim < 1 || d->basis_dim > VR_MAX_BASIS))
        return fail(VR_ERR_INVALID_ARGUMENT, "basis_dim=%d out of range [1,%d]", d->basis_dim,
                    VR_MAX_BASIS);
    if (d->data_dim < min_dim)
        return fail(VR_ERR_INVALID_ARGUMENT, "data_dim=%d too small for the format (need %d)",
                    d->data_dim, min_dim);
    if (d->format == VR_FORMAT_SG && (!d->extra || d->extra_count < (uint64_t)d->basis_dim * 4))
        return fail(VR_ERR_INVALID_ARGUMENT, "SG needs basis_dim*4 extra floats");
    if (d->format == VR_FORMAT_ASG && (!d->extra || d->extra_count < (uint64_t)d->basis_dim * 11))
        return fail(VR_ERR_INVALID_ARGUMENT, "ASG needs basis_dim*11 extra floats");
    return VR_OK;
}

// Everything of a tree that is not tree data, on the current device (= t->device): status and
// tally words, the launch-slot ring (events, frame tables, queue heads, probe coefficients).
hipError_t alloc_launch_scratch(VrTreeOpaque* t) {
    hipError_t e = t->status.alloc(sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemset(t->status.get(), 0, sizeof(uint32_t));
    if (e == hipSuccess) e = t->sched_stats.alloc(vr::kSchedStats * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(t->sched_stats.get(), 0, vr::kSchedStats * sizeof(unsigned long long));
    if (e == hipSuccess) e = t->probe_buf.alloc(sizeof(float) * (size_t)t->desc.data_dim * kLaunchSlots);
    for (unsigned i = 0; i < kLaunchSlots && e == hipSuccess; ++i) e = t->slots[i].done.create();
    if (e == hipSuccess) e = t->slot_frames.alloc(sizeof(vr::FrameDesc) * vr::kMaxBatch * kLaunchSlots);
    if (e == hipSuccess) e = t->slot_heads.alloc(sizeof(uint32_t) * vr::kSlotWords * kLaunchSlots);
    if (e == hipSuccess) e = t->slot_aovs.alloc(sizeof(vr::AovDesc) * vr::kMaxBatch * kLaunchSlots);
    int cus = 0;
    if (e == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) == hipSuccess &&
        cus > 0)
        t->n_cus = cus;
    return e;
}

int upload_body(const VrTreeDesc* d, const VrQuantDesc* q, vr_tree_t* out) {
    if (!d || !out) return fail(VR_ERR_INVALID_ARGUMENT, "desc/out is NULL");
    *out = nullptr;
    if (int rc = check_tree_desc(d, q == nullptr)) return rc;
    if (int rc = q ? check_quant(d, q) : VR_OK) return rc;

    const int N3 = d->N * d->N * d->N;
    const size_t n_slots = (size_t)d->capacity * N3;
    const size_t child_sz = n_slots * sizeof(int32_t);
    const size_t data_sz = n_slots * (size_t)d->data_dim * sizeof(uint16_t);

    const bool timing = getenv("VR_UPLOAD_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&]() {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    };
    // topology check needs the child words on the host
    std::vector<int32_t> staged;
    const int32_t* host_child = d->child;
    if (d->memory == 1) {
        staged.resize(n_slots);
        HIP_TRY(hipMemcpy(staged.data(), d->child, child_sz, hipMemcpyDeviceToHost));
        host_child = staged.data();
    }
    // The big host-to-device copies (and the codebook decode of a quantised file) run on a
    // helper thread while this one walks the tree on the host (topology check, node numbering):
    // the walks only read the child array, and hide completely behind the copies.
    // (a malformed tree is reported as such even where no device exists: no HIP error before that)
    // The first HIP call of a process starts the runtime (~50 ms; 145-200 ms now and then, right
    // after another process released gigabytes of device memory -- the outlier of
    // tools/upload_bench.py).  It has to be made on THIS thread (the tree goes to the caller's
    // current device, and a new thread's current device is 0), so the topology check starts first,
    // on a thread of its own, and runs beside it.
    char why[256] = "";
    std::vector<uint8_t> level;
    int max_depth = -1;
    bool walk_threw = false;
    std::thread walker([&] {
        try {
            max_depth = validate_topology(host_child, d->capacity, N3, level, why, sizeof(why));
        } catch (...) {
            walk_threw = true;
        }
        if (timing) fprintf(stderr, "[volrend_hip] upload: topology checked at %.1f ms\n", since());
    });
    Joiner walker_join{walker};
    int device = 0;
    const hipError_t e_dev = hipGetDevice(&device);
    if (timing) fprintf(stderr, "[volrend_hip] upload: HIP runtime up at %.1f ms\n", since());
    // staging copies of the reference arrays, written by the copier: declared before it and its join
    // guard, so that every exit joins the copier before they are freed
    DeviceBuffer d_child, d_data;
    hipError_t e_copy = e_dev;
    // (the copier only moves the small child array and pays the runtime's start-up before it
    // looks at `topo`: a malformed file is rejected after ~30 ms of host walk, not after a
    // multi-GB upload)
    std::atomic<int> topo{0};  // 0: the check is still running, 1: tree is sound, -1: bad tree
    // the file's pages are mapped (prefault_host_range) beside the runtime's start-up and the
    // topology check, ahead of the copy that reads them
    std::thread prefaulter([&] {
        if (d->memory != 1 && !q) prefault_host_range(d->data, data_sz);
    });
    Joiner prefault_join{prefaulter};
    std::thread copier([&] {
        if (e_dev != hipSuccess) return;
        hipError_t e = hipSetDevice(device);
        // runtime start-up, the allocations and the copy pipeline's pinned slots + stream first:
        // they need the process's mmap lock exclusively, which a page-mapping pass would hold
        if (d->memory != 1 && e == hipSuccess) e = d_child.alloc(child_sz);
        if ((q || d->memory != 1) && e == hipSuccess) e = d_data.alloc(data_sz);
        if (d->memory != 1 && e == hipSuccess) upload_cache().warm(device);
        if (timing) fprintf(stderr, "[volrend_hip] upload: runtime + buffers ready at %.1f ms\n", since());
        while (topo.load(std::memory_order_acquire) == 0) std::this_thread::sleep_for(std::chrono::microseconds(100));
        if (topo.load(std::memory_order_acquire) < 0) {
            e_copy = e;
            return;
        }
        if (q) {  // quantised file: only the codebook arrays cross PCIe, the decode runs on the device
            const CopySegment child{d_child.get(), d->child, child_sz};
            if (e == hipSuccess && d->memory != 1) e = staged_h2d_multi(&child, 1, device);
            if (e == hipSuccess) e = decode_quant_on_device(d, q, n_slots, d_data.get<uint16_t>(), device);
        } else if (d->memory != 1 && e == hipSuccess) {
            const CopySegment both[2] = {{d_child.get(), d->child, child_sz}, {d_data.get(), d->data, data_sz}};
            e = staged_h2d_multi(both, 2, device);
        }
        e_copy = e;
        if (timing) fprintf(stderr, "[volrend_hip] upload: copies done at %.1f ms\n", since());
    });
    Joiner copier_join{copier, &topo};  // every exit below waits for the copies

    walker.join();
    if (walk_threw) {  // (the copier must be released before the exception travels on)
        topo.store(-1, std::memory_order_release);
        throw std::bad_alloc();
    }
    topo.store(max_depth < 0 ? -1 : 1, std::memory_order_release);
    if (max_depth < 0) return fail(VR_ERR_BAD_TREE, "bad tree: %s", why);
    if (e_dev != hipSuccess)
        return fail(VR_ERR_HIP, "hipGetDevice failed: %s", hipGetErrorString(e_dev));
    // Lookup structure (N == 2 fast path): leaves must sit within 24 levels (exact integer
    // digits of a binary32 coordinate) and node*8+slot byte offsets must fit 32 bits.
    int G0 = 0, BL = 0;
    const Tuning tn = default_tuning();  // the new tree's own copy from here on
    if (vr_query_mode_for(d->N, max_depth, d->capacity) == VR_QUERY_LOOKUP) {
        // auto: top grid + brick reach the deepest leaf (depth max_depth + 1) without a child-word
        // walk where a top grid of <= 256^3 cells allows it -- 64^3 (2 MB) for lego-class trees of
        // 9 levels, 128^3 for 10 (measured: C1 0.269 ms at (6,3) against 0.301 at (5,3); C3 0.790
        // at (7,3) against 0.847 at (6,3))
        G0 = tn.top_levels > 0 ? tn.top_levels : (max_depth + 1 - 3 < 6 ? 6 : max_depth + 1 - 3);
        if (G0 > 8) G0 = 8;
        if (G0 > max_depth + 1) G0 = max_depth + 1;  // deepest leaf depth
        BL = tn.brick_levels < 1 ? 1 : (tn.brick_levels > 4 ? 4 : tn.brick_levels);
        if (BL > max_depth + 1 - G0) BL = max_depth + 1 - G0;  // 0: the top grid resolves every leaf
        // the kernel addresses brick entries with 32-bit byte offsets: keep the brick array < 4 GB
        uint64_t n_roots = 0;
        for (uint8_t l : level) n_roots += (l == G0);
        while (BL > 1 && ((n_roots << (3 * BL)) * sizeof(uint32_t)) >= (1ull << 32)) --BL;
    }

    std::unique_ptr<VrTreeOpaque> t(new (std::nothrow) VrTreeOpaque());
    if (!t) return fail(VR_ERR_OUT_OF_MEMORY, "host allocation failed");
    t->desc = *d;
    t->desc.child = nullptr;
    t->desc.data = nullptr;
    t->desc.extra = nullptr;
    t->max_depth = max_depth;
    t->device = device;
    t->tn = tn;
    // new node numbering (host walk) while the copies are still in flight
    std::vector<int32_t> brick_roots;
    const std::vector<int32_t> perm =
        node_permutation(host_child, d->capacity, N3, G0, BL, level, brick_roots);
    // the reference arrays are staged on the device now (unless they already were there);
    // re-layout into nodes/leaves, build the lookup structure, drop the staging copies
    if (timing) fprintf(stderr, "[volrend_hip] upload: host walks done at %.1f ms\n", since());
    copier.join();
    hipError_t e = e_copy;
    const int32_t* src_child = d->memory != 1 ? d_child.get<int32_t>() : d->child;
    const uint16_t* src_data = (q || d->memory != 1) ? d_data.get<uint16_t>() : d->data;
    t->leaf_stride_h = vr::leaf_stride_halfs(d->data_dim);
    const size_t leaves_sz = n_slots * (size_t)t->leaf_stride_h * sizeof(uint16_t);
    DeviceBuffer& nodes = t->arrays[kNodes];
    if (e == hipSuccess) e = nodes.alloc(child_sz);
    if (e == hipSuccess) e = t->arrays[kLeaves].alloc(leaves_sz);
    if (e == hipSuccess) e = alloc_launch_scratch(t.get());
    DeviceBuffer d_perm;
    if (e == hipSuccess) e = d_perm.alloc(perm.size() * sizeof(int32_t));
    if (e == hipSuccess)
        e = hipMemcpy(d_perm.get(), perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = vr::launch_relayout(src_child, src_data, d_perm.get<int32_t>(), nodes.get<uint32_t>(),
                                t->arrays[kLeaves].get<uint16_t>(), (int64_t)n_slots, N3, d->data_dim,
                                t->leaf_stride_h, nullptr);
    t->device_bytes = child_sz + leaves_sz + sizeof(uint32_t);
    // lookup structure: top grid + bricks (vr_dev_layout.h), built from the node words
    DeviceBuffer d_roots;
    if (e == hipSuccess && G0 > 0) {
        const size_t top_sz = ((size_t)1 << (3 * G0)) * sizeof(uint2);
        const int n_bricks = BL > 0 ? (int)brick_roots.size() : 0;
        const size_t brick_sz = ((size_t)n_bricks << (3 * BL)) * sizeof(uint32_t);
        e = t->arrays[kTop].alloc(top_sz);
        if (e == hipSuccess && n_bricks) e = t->arrays[kBricks].alloc(brick_sz);
        if (e == hipSuccess && n_bricks) e = d_roots.alloc(n_bricks * sizeof(int32_t));
        if (e == hipSuccess && n_bricks)
            e = hipMemcpy(d_roots.get(), brick_roots.data(), n_bricks * sizeof(int32_t),
                          hipMemcpyHostToDevice);
        // entry order of the bricks: blocked where the lookups are fabric traffic (a lookup structure
        // far beyond the 32 MB of L2), x-major where they mostly hit (six instructions cheaper)
        const int blocked = (n_bricks && BL == 3)
                                ? (tn.brick_blocked >= 0 ? tn.brick_blocked
                                                         : (top_sz + brick_sz > (128ull << 20)))
                                : 0;
        if (e == hipSuccess)
            e = vr::launch_build_lookup(nodes.get<uint32_t>(), d_roots.get<int32_t>(), n_bricks,
                                        t->arrays[kTop].get<uint2>(), t->arrays[kBricks].get<uint32_t>(),
                                        G0, BL, blocked, t->status.get<uint32_t>(), nullptr);
        uint32_t flag = 0;
        if (e == hipSuccess) e = hipMemcpy(&flag, t->status.get(), sizeof(flag), hipMemcpyDeviceToHost);
        if (e == hipSuccess && flag != 0)
            return fail(VR_ERR_BAD_TREE, "lookup structure build failed (flag %u)", flag);
        if (e == hipSuccess) {
            t->top_levels = G0;
            t->brick_levels = n_bricks ? BL : 0;
            t->brick_blocked = blocked;
            t->n_bricks = n_bricks;
            t->device_bytes += top_sz + brick_sz;
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && d->extra && d->extra_count) {
        const size_t esz = (size_t)d->extra_count * sizeof(float);
        const hipMemcpyKind kind =
            d->memory == 1 ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        e = t->extra.alloc(esz);
        if (e == hipSuccess) e = hipMemcpy(t->extra.get(), d->extra, esz, kind);
        t->device_bytes += esz;
    }
    if (e != hipSuccess) return fail(hip_code(e), "tree upload failed: %s", hipGetErrorString(e));
    if (timing) fprintf(stderr, "[volrend_hip] upload: device-ready at %.1f ms\n", since());
    *out = t.release();
    return VR_OK;
}

// The host side of an upload allocates (level / permutation vectors) and starts threads: nothing
// of that may leave through the C boundary as an exception.
int upload_impl(const VrTreeDesc* d, const VrQuantDesc* q, vr_tree_t* out) {
    try {
        return upload_body(d, q, out);
    } catch (const std::bad_alloc&) {
        if (out) *out = nullptr;
        return fail(VR_ERR_OUT_OF_MEMORY, "tree upload: host allocation failed");
    } catch (const std::exception& e) {  // std::system_error of a thread that could not start
        if (out) *out = nullptr;
        return fail(VR_ERR_OUT_OF_MEMORY, "tree upload: %s", e.what());
    }
}

}  // namespace

extern "C" {

int vr_tree_upload(const VrTreeDesc* d, vr_tree_t* out) { return upload_impl(d, nullptr, out); }

int vr_tree_upload_quantized(const VrTreeDesc* d, const VrQuantDesc* q, vr_tree_t* out) {
    if (!q) return fail(VR_ERR_INVALID_ARGUMENT, "quant desc is NULL");
    return upload_impl(d, q, out);
}

int vr_decode_quantized(const VrTreeDesc* d, const VrQuantDesc* q, uint16_t* data_out) {
    if (!d || !q || !data_out) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->N < 2 || d->N > 16 || d->capacity <= 0 || d->data_dim < 1)
        return fail(VR_ERR_INVALID_ARGUMENT, "bad N / capacity / data_dim");
    if (int rc = check_quant(d, q)) return rc;
    const size_t n_slots = (size_t)d->capacity * d->N * d->N * d->N;
    const size_t data_sz = n_slots * (size_t)d->data_dim * sizeof(uint16_t);
    DeviceBuffer staging;  // (a host destination: the decode runs into device memory first)
    hipError_t e = hipSuccess;
    if (d->memory != 1) e = staging.alloc(data_sz);
    uint16_t* d_data = d->memory != 1 ? staging.get<uint16_t>() : data_out;
    int device = 0;
    if (e == hipSuccess) e = hipGetDevice(&device);
    if (e == hipSuccess) e = decode_quant_on_device(d, q, n_slots, d_data, device);
    if (e == hipSuccess && d->memory != 1)
        e = hipMemcpy(data_out, d_data, data_sz, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(hip_code(e), "quantised decode failed: %s", hipGetErrorString(e));
    return VR_OK;
}

int vr_tree_clone(vr_tree_t src, int device, vr_tree_t* out) {
    if (!src || !out) return fail(VR_ERR_INVALID_ARGUMENT, "tree/out is NULL");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev)
        return fail(VR_ERR_INVALID_ARGUMENT, "device %d outside [0,%d)", device, n_dev);
    // the source may still be rendering on its own device; no launch may be enqueued on it (nor
    // its bitmaps / slots change) while its arrays are read
    std::lock_guard<std::mutex> src_lock(src->launch_mutex);
    {
        DeviceGuard g(src->device);
        HIP_TRY(hipDeviceSynchronize());
    }
    DeviceGuard guard(device);
    std::unique_ptr<VrTreeOpaque> t(new (std::nothrow) VrTreeOpaque());
    if (!t) return fail(VR_ERR_OUT_OF_MEMORY, "host allocation failed");
    static_cast<TreeShape&>(*t) = *src;
    t->device = device;
    t->tn = src->tn;
    // the re-laid-out arrays travel device to device (over xGMI between two GPUs of a node):
    // no second pass over PCIe, no second re-layout
    // direct peer access (xGMI / PCIe P2P) when the two devices have it: hipMemcpyPeer then moves
    // the arrays device to device; without it the runtime stages them through host memory
    // (still correct, ~10x slower) -- a note goes to stderr
    bool p2p = true;
    if (src->device != device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, src->device) != hipSuccess) can = 0;
        p2p = can != 0;
        if (p2p) {
            const hipError_t pe = hipDeviceEnablePeerAccess(src->device, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) p2p = false;
        }
        (void)hipGetLastError();
    }
    auto copy = [&](DeviceBuffer& to, const DeviceBuffer& from) {
        if (!from) return hipSuccess;
        const hipError_t e = to.alloc(from.bytes());
        return e != hipSuccess ? e : hipMemcpyPeer(to.get(), device, from.get(), src->device, from.bytes());
    };
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = copy(t->arrays[i], src->arrays[i]);
    if (e == hipSuccess) e = copy(t->extra, src->extra);
    if (e == hipSuccess) e = alloc_launch_scratch(t.get());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess)
        return fail(hip_code(e), "tree clone from device %d to device %d failed: %s%s", src->device, device,
                    hipGetErrorString(e),
                    p2p ? "" : " (the devices have NO peer access: check `rocm-smi --showtopo`, "
                               "IOMMU / ACS settings and HSA_ENABLE_IPC_MODE_LEGACY=0)");
    if (!p2p)  // (a note, not an error: vr_last_error() stays empty after a call that returned VR_OK)
        fprintf(stderr, "[volrend_hip] note: devices %d and %d have no peer access; the clone was "
                        "staged through host memory\n", src->device, device);
    *out = t.release();
    return VR_OK;
}

int vr_tree_free(vr_tree_t t) {
    delete t;  // (the tree's owners free its memory on its device)
    return VR_OK;
}

}  // extern "C"
