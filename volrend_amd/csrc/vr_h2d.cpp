// vr_h2d.cpp -- the staged host-to-device copy pipeline of an upload (vr_h2d.h).
//
// hipMemcpy from pageable memory stages through ONE thread's memcpy (~9 GB/s measured: 1.67 GB in
// 0.19 s); here up to kCopyWorkersMax threads each stream chunks through two pinned slots of their
// own: memcpy into slot k while the DMA of the previous chunk drains slot k ^ 1.  With the source
// pages mapped ahead of time (prefault_host_range) the memcpy threads keep the link busy, 36-45 GB/s
// measured; without, the memcpy is page-fault bound at ~20.  All the DMAs go to ONE stream per device
// (creating a stream costs milliseconds -- an HSA queue -- and the link is the shared resource
// anyway); that stream and the pinned slots (with their events) live in a process-wide cache, so only
// the first upload of a process pays for them.  Chunks are claimed dynamically across all segments of
// a call.  Anything small, or any failure to set the pipeline up, falls back to the plain blocking
// copy.  VR_UPLOAD_TIMING=1 prints the phases.
#include "vr_h2d.h"

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace {

constexpr size_t kCopyChunk = 2u << 20;  // one pinned slot (pinned memory costs ~0.5 ms per MB to allocate:
                                         // kCopyWorkersMax workers x 2 slots = 16 MB)
constexpr int kCopyWorkersMax = 4;       // (with the pages mapped ahead, 4 memcpy threads fill the link)

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
        if (device < 0 || device >= kDevices) return;  // (take hands nothing out for such a device)
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

}  // namespace

void warm_upload_cache(int device) { upload_cache().warm(device); }

// (tree files are handed over as views of an mmap'ed npz: every 4 KB page of the 1.6 GB costs a
// minor fault the first time a copy worker reads it, and the copy is fault-bound.  Runs on a few
// threads while the HIP runtime starts up.)
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
