// vr_upload.cpp -- tree upload, clone and free (include/volrend_hip.h): vr_tree_upload as a list of
// steps, the quantised decode.  The host walks are vr_tree_walk.cpp, the copy pipeline is vr_h2d.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <future>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "vr_h2d.h"
#include "vr_host.h"
#include "vr_tree_walk.h"

namespace {

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
    const size_t cull_sz = (size_t)vr::kCullStatLines * vr::kCullStatStride * sizeof(unsigned long long);
    if (e == hipSuccess) e = t->cull_stats.alloc(cull_sz);
    if (e == hipSuccess) e = hipMemset(t->cull_stats.get(), 0, cull_sz);
    if (e == hipSuccess) e = t->head_stats.alloc(cull_sz);
    if (e == hipSuccess) e = hipMemset(t->head_stats.get(), 0, cull_sz);
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

// The steps of vr_tree_upload / vr_tree_upload_quantized.  The big host-to-device copies (and the
// codebook decode of a quantised file) run on a helper thread while the calling thread walks the
// tree on the host: the walks only read the child array, and hide completely behind the copies.
// Every helper is a std::async task.  It owns what it writes and hands it over as its result -- or
// its exception, which arrives at the caller as what it was -- and its future joins it on every way
// out of the scope that holds it: no exit frees memory that a helper still writes.  What helpers
// only read (UploadJob) belongs to the frame above theirs.

// What one upload works on: the caller's descriptors and the sizes that follow from them.
struct UploadJob {
    const VrTreeDesc* d;
    const VrQuantDesc* q;       // NULL: a plain tree
    const int32_t* host_child;  // the child words in host memory, for the walks
    int N3;
    size_t n_slots, child_sz, data_sz;
    bool from_host;  // the caller's arrays are host memory (d->memory != 1)
    bool timing;     // VR_UPLOAD_TIMING=1: the phase marks
    std::chrono::steady_clock::time_point t_start;
    void mark(const char* what) const {
        const std::chrono::duration<double, std::milli> ms = std::chrono::steady_clock::now() - t_start;
        if (timing) fprintf(stderr, "[volrend_hip] upload: %s at %.1f ms\n", what, ms.count());
    }
};

// Step: the descriptors, before anything else looks at them.  Clears *out.
int check_upload_args(const VrTreeDesc* d, const VrQuantDesc* q, vr_tree_t* out) {
    if (!d || !out) return fail(VR_ERR_INVALID_ARGUMENT, "desc/out is NULL");
    *out = nullptr;
    if (int rc = check_tree_desc(d, q == nullptr)) return rc;
    return q ? check_quant(d, q) : VR_OK;
}

// Step: the topology check needs the child words on the host.  Those of a device-resident tree are
// fetched into `fetched`, which the caller keeps for as long as the job runs.
int fetch_child_words(UploadJob& j, std::vector<int32_t>& fetched) {
    if (j.from_host) return VR_OK;
    fetched.resize(j.n_slots);
    HIP_TRY(hipMemcpy(fetched.data(), j.d->child, j.child_sz, hipMemcpyDeviceToHost));
    j.host_child = fetched.data();
    return VR_OK;
}

// Step: the topology check, on a thread of its own and started before the first HIP call, so that it
// runs beside the runtime's start-up and a malformed tree is reported as such even where no device
// exists.  max_depth < 0: a bad tree, and `why`.
struct Walk {
    int max_depth = -1;
    std::vector<uint8_t> level;
    char why[256] = "";
};
std::shared_future<Walk> start_walk(const UploadJob& j) {
    return std::async(std::launch::async, [&j] {
        Walk w;
        w.max_depth = validate_topology(j.host_child, j.d->capacity, j.N3, w.level, w.why, sizeof(w.why));
        j.mark("topology checked");
        return w;
    }).share();
}

// Step: the copier.  It allocates the staging copies of the reference arrays on `device`, copies (or,
// for a quantised file, decodes) into them and hands them over.  The runtime's start-up on this
// thread, the allocations and the copy pipeline's pinned slots + stream come first (they need the
// process's mmap lock exclusively, which a page-mapping pass would hold); then it blocks for the
// verdict of the walk and moves no bulk data for a bad tree: a malformed file is rejected after
// ~30 ms of host walk, not after a multi-GB upload.
struct Staged {
    hipError_t e = hipSuccess;
    DeviceBuffer child, data;  // empty where the caller's own device arrays are the source
};
std::future<Staged> start_copies(const UploadJob& j, hipError_t e_dev, int device,
                                 std::shared_future<Walk> walk) {
    return std::async(std::launch::async, [&j, e_dev, device, walk] {
        Staged s;
        hipError_t& e = s.e;
        if ((e = e_dev) != hipSuccess) return s;
        e = hipSetDevice(device);
        if (j.from_host && e == hipSuccess) e = s.child.alloc(j.child_sz);
        if ((j.q || j.from_host) && e == hipSuccess) e = s.data.alloc(j.data_sz);
        if (j.from_host && e == hipSuccess) warm_upload_cache(device);
        j.mark("runtime + buffers ready");
        if (walk.get().max_depth < 0) return s;
        const CopySegment both[2] = {{s.child.get(), j.d->child, j.child_sz},
                                     {s.data.get(), j.d->data, j.data_sz}};
        if (j.q) {  // quantised file: only the codebook arrays cross PCIe, the decode runs on the device
            if (e == hipSuccess && j.from_host) e = staged_h2d_multi(both, 1, device);
            if (e == hipSuccess) e = decode_quant_on_device(j.d, j.q, j.n_slots, s.data.get<uint16_t>(), device);
        } else if (j.from_host && e == hipSuccess) {
            e = staged_h2d_multi(both, 2, device);
        }
        j.mark("copies done");
        return s;
    });
}

// Step: the host side of the new tree: the caller's description without its pointers, the knobs.
std::unique_ptr<VrTreeOpaque> new_tree(const UploadJob& j, int max_depth, int device, const Tuning& tn) {
    std::unique_ptr<VrTreeOpaque> t(new (std::nothrow) VrTreeOpaque());
    if (!t) return t;
    t->desc = *j.d;
    t->desc.child = nullptr;
    t->desc.data = nullptr;
    t->desc.extra = nullptr;
    t->max_depth = max_depth;
    t->device = device;
    t->tn = tn;
    t->leaf_stride_h = vr::leaf_stride_halfs(j.d->data_dim);
    return t;
}

// Step: allocates the tree's node and leaf arrays and its launch scratch, and re-lays the staged
// reference arrays out into them under the new numbering.  `d_perm` is what the kernel reads: the
// caller keeps it until the device has been synchronised.
hipError_t relayout(const UploadJob& j, const Staged& s, const std::vector<int32_t>& perm, VrTreeOpaque* t,
                    DeviceBuffer& d_perm) {
    const int32_t* src_child = j.from_host ? s.child.get<int32_t>() : j.d->child;
    const uint16_t* src_data = (j.q || j.from_host) ? s.data.get<uint16_t>() : j.d->data;
    const size_t leaves_sz = j.n_slots * (size_t)t->leaf_stride_h * sizeof(uint16_t);
    DeviceBuffer& nodes = t->arrays[kNodes];
    hipError_t e = nodes.alloc(j.child_sz);
    if (e == hipSuccess) e = t->arrays[kLeaves].alloc(leaves_sz);
    if (e == hipSuccess) e = alloc_launch_scratch(t);
    if (e == hipSuccess) e = d_perm.alloc(perm.size() * sizeof(int32_t));
    if (e == hipSuccess)
        e = hipMemcpy(d_perm.get(), perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = vr::launch_relayout(src_child, src_data, d_perm.get<int32_t>(), nodes.get<uint32_t>(),
                                t->arrays[kLeaves].get<uint16_t>(), (int64_t)j.n_slots, j.N3, j.d->data_dim,
                                t->leaf_stride_h, nullptr);
    t->device_bytes = j.child_sz + leaves_sz + sizeof(uint32_t);
    return e;
}

// Step: the lookup structure, top grid + bricks (vr_dev_layout.h), built from the node words.  `flag`
// is what the build kernel left in the tree's status word: non-zero = the tree does not fit the
// structure.  `d_roots` is kept by the caller like d_perm.
hipError_t build_lookup(const LookupPlan& plan, const std::vector<int32_t>& brick_roots, VrTreeOpaque* t,
                        DeviceBuffer& d_roots, uint32_t& flag) {
    const int G0 = plan.G0, BL = plan.BL;
    const size_t top_sz = ((size_t)1 << (3 * G0)) * sizeof(uint2);
    const int n_bricks = BL > 0 ? (int)brick_roots.size() : 0;
    const size_t brick_sz = ((size_t)n_bricks << (3 * BL)) * sizeof(uint32_t);
    hipError_t e = t->arrays[kTop].alloc(top_sz);
    if (e == hipSuccess && n_bricks) e = t->arrays[kBricks].alloc(brick_sz);
    if (e == hipSuccess && n_bricks) e = d_roots.alloc(n_bricks * sizeof(int32_t));
    if (e == hipSuccess && n_bricks)
        e = hipMemcpy(d_roots.get(), brick_roots.data(), n_bricks * sizeof(int32_t), hipMemcpyHostToDevice);
    // entry order of the bricks: blocked where the lookups are fabric traffic (a lookup structure
    // far beyond the 32 MB of L2), x-major where they mostly hit (six instructions cheaper)
    const int blocked = (n_bricks && BL == 3)
                            ? (t->tn.brick_blocked >= 0 ? t->tn.brick_blocked
                                                        : (top_sz + brick_sz > (128ull << 20)))
                            : 0;
    if (e == hipSuccess)
        e = vr::launch_build_lookup(t->arrays[kNodes].get<uint32_t>(), d_roots.get<int32_t>(), n_bricks,
                                    t->arrays[kTop].get<uint2>(), t->arrays[kBricks].get<uint32_t>(),
                                    G0, BL, blocked, t->status.get<uint32_t>(), nullptr);
    if (e == hipSuccess) e = hipMemcpy(&flag, t->status.get(), sizeof(flag), hipMemcpyDeviceToHost);
    if (e == hipSuccess && flag == 0) {
        t->top_levels = G0;
        t->brick_levels = n_bricks ? BL : 0;
        t->brick_blocked = blocked;
        t->n_bricks = n_bricks;
        t->brick_root.assign(brick_roots.begin(), brick_roots.begin() + n_bricks);  // what vr_tree_update_data refreshes the bricks by
        t->device_bytes += top_sz + brick_sz;
    }
    return e;
}

// Step: the occupancy of the block cull (vr_internal.h "Block cull") for a tree that has its lookup structure:
// allocated for the worst case -- every cell in the list -- and built from the node words.
hipError_t build_occupancy(VrTreeOpaque* t) {
    if (t->top_levels <= 0) return hipSuccess;
    const int deepest = t->max_depth + 1;  // depth of the deepest leaf
    t->occ_levels = deepest < vr::kOccMaxLevels ? deepest : vr::kOccMaxLevels;
    const size_t bytes = vr::occ_words(t->occ_levels) * sizeof(uint32_t);
    hipError_t e = t->occ.alloc(bytes);
    if (e == hipSuccess) e = refresh_occupancy(t, nullptr);
    t->device_bytes += bytes;
    return e;
}

// Step: the extra array (SG / ASG lobes), from wherever the caller's arrays are.
hipError_t upload_extra(const UploadJob& j, VrTreeOpaque* t) {
    if (!j.d->extra || !j.d->extra_count) return hipSuccess;
    const size_t esz = (size_t)j.d->extra_count * sizeof(float);
    hipError_t e = t->extra.alloc(esz);
    if (e == hipSuccess)
        e = hipMemcpy(t->extra.get(), j.d->extra, esz,
                      j.from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
    t->device_bytes += esz;
    return e;
}

// An upload whose child words are on the host, in steps.
int upload_steps(const UploadJob& j, vr_tree_t* out) {
    std::shared_future<Walk> walk = start_walk(j);
    // The first HIP call of a process starts the runtime (~50 ms; 145-200 ms now and then, right
    // after another process released gigabytes of device memory -- the outlier of
    // tools/upload_bench.py).  It has to be made on THIS thread (the tree goes to the caller's
    // current device, and a new thread's current device is 0), with the topology check already
    // running beside it.
    int device = 0;
    const hipError_t e_dev = hipGetDevice(&device);
    j.mark("HIP runtime up");
    // the file's pages are mapped beside the runtime's start-up and the topology check, ahead of the
    // copy that reads them
    std::future<void> prefault = std::async(std::launch::async, [&j] {
        if (j.from_host && !j.q) prefault_host_range(j.d->data, j.data_sz);
    });
    std::future<Staged> copies = start_copies(j, e_dev, device, walk);

    const Walk& w = walk.get();
    if (w.max_depth < 0) return fail(VR_ERR_BAD_TREE, "bad tree: %s", w.why);
    if (e_dev != hipSuccess)
        return fail(VR_ERR_HIP, "hipGetDevice failed: %s", hipGetErrorString(e_dev));
    const Tuning tn = default_tuning();  // the new tree's own copy from here on
    const LookupPlan plan =
        plan_lookup(j.d->N, w.max_depth, j.d->capacity, tn.top_levels, tn.brick_levels, [&w](int l) {
            return (uint64_t)std::count(w.level.begin(), w.level.end(), (uint8_t)l);
        });
    std::unique_ptr<VrTreeOpaque> t = new_tree(j, w.max_depth, device, tn);
    if (!t) return fail(VR_ERR_OUT_OF_MEMORY, "host allocation failed");
    // new node numbering (host walk) while the copies are still in flight
    std::vector<int32_t> brick_roots;
    const std::vector<int32_t> perm =
        node_permutation(j.host_child, j.d->capacity, j.N3, plan.G0, plan.BL, w.level, brick_roots);
    t->file_node = inverse_permutation(perm);  // what vr_accumulate_weights indexes its outputs by
    j.mark("host walks done");

    // the reference arrays are staged on the device now (unless they already were there);
    // re-layout into nodes / leaves, build the lookup structure, drop the staging copies
    const Staged staged = copies.get();
    DeviceBuffer d_perm, d_roots;  // read by the kernels below: freed behind the synchronise
    hipError_t e = staged.e;
    if (e == hipSuccess) e = relayout(j, staged, perm, t.get(), d_perm);
    uint32_t flag = 0;
    if (e == hipSuccess && plan.G0 > 0) e = build_lookup(plan, brick_roots, t.get(), d_roots, flag);
    if (e == hipSuccess && flag != 0)
        return fail(VR_ERR_BAD_TREE, "lookup structure build failed (flag %u)", flag);
    if (e == hipSuccess) e = build_occupancy(t.get());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = upload_extra(j, t.get());
    if (e != hipSuccess) return fail(hip_code(e), "tree upload failed: %s", hipGetErrorString(e));
    j.mark("device-ready");
    *out = t.release();
    return VR_OK;
}

int upload_body(const VrTreeDesc* d, const VrQuantDesc* q, vr_tree_t* out) {
    if (int rc = check_upload_args(d, q, out)) return rc;
    const int N3 = d->N * d->N * d->N;
    const size_t n_slots = (size_t)d->capacity * N3;
    UploadJob j{d, q, d->child, N3, n_slots, n_slots * sizeof(int32_t),
                n_slots * (size_t)d->data_dim * sizeof(uint16_t), d->memory != 1,
                getenv("VR_UPLOAD_TIMING") != nullptr, std::chrono::steady_clock::now()};
    std::vector<int32_t> fetched;  // (in this frame: it outlives every helper of upload_steps)
    if (int rc = fetch_child_words(j, fetched)) return rc;
    return upload_steps(j, out);
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

hipError_t refresh_occupancy(const VrTreeOpaque* t, hipStream_t hs) {
    if (!t->occ) return hipSuccess;
    return vr::launch_build_occupancy(t->arrays[kNodes].get<uint32_t>(), t->occ_levels, t->occ.get<uint32_t>(), hs);
}

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
    t->file_node = src->file_node;  // (its device copy is made on the clone's first vr_accumulate_weights)
    t->brick_root = src->brick_root;  // (likewise: on the clone's first vr_tree_update_data / vr_tree_read_data)
    t->device_bytes -= src->file_node_dev.bytes() + src->brick_root_dev.bytes() + src->node_of_file_dev.bytes();
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
    if (e == hipSuccess) e = copy(t->occ, src->occ);  // (bitmap and list travel with the arrays they were built from)
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
