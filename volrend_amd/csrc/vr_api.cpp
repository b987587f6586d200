// vr_api.cpp -- the C ABI of libvolrend_hip.so (include/volrend_hip.h), host side: version, errors,
// devices, defaults, tuning, statistics, status and touch bitmaps, tile assembly, probe, read-back.
// Upload, clone and free are in vr_upload.cpp (its host walks in vr_tree_walk.cpp, its copy pipeline in
// vr_h2d.cpp), launches in vr_launch.cpp (their scheduling rules in vr_launch_plan.cpp, the launch-slot ring and
// vr_reserve* in vr_slots.cpp), the value passes in vr_values.cpp.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "vr_host.h"
#include "vr_tree_walk.h"

namespace {

thread_local char g_err[512] = "";

// One row per tuning knob (struct Tuning): its vr_set_tuning key, the environment variable the
// process default is read from (once), how a value from either source is brought into range, and
// whether the knob is fixed at upload (it shapes the lookup structure built then).
enum KnobRange { kClamp, kClamp64, kFlag, kAutoFlag };  // [lo, hi]; then down to a multiple of 64 (1..63: 64);
                                                        // 0 / 1; -1 (per tree) for v < 0, else 0 / 1
struct Knob { const char *key, *env; int Tuning::*field; KnobRange range; int lo, hi; bool fixed_at_upload; };
const Knob kKnobs[] = {
    {"march_max", "VR_MARCH_MAX", &Tuning::march_max, kClamp, 1, INT_MAX, false},
    {"refill_min", "VR_REFILL_MIN", &Tuning::refill_min, kClamp, 1, 64, false},
    {"drain_flush", "VR_DRAIN_FLUSH", &Tuning::drain_flush, kClamp, 0, 64, false},
    {"waves_per_cu", "VR_WAVES_PER_CU", &Tuning::waves_per_cu, kClamp, 0, 64, false},
    {"frame_group", "VR_FRAME_GROUP", &Tuning::frame_group, kClamp, 0, INT_MAX, false},
    {"super_block", "VR_SUPER_BLOCK", &Tuning::super_block, kClamp, 0, 64, false},
    {"records_nt", "VR_RECORDS_NT", &Tuning::records_nt, kAutoFlag, 0, 0, false},
    {"xcd_queues", "VR_XCD_QUEUES", &Tuning::xcd_queues, kFlag, 0, 0, false},
    {"chunk_max", "VR_CHUNK_MAX", &Tuning::chunk_max, kClamp64, 0, INT_MAX, false},
    {"raygen_waves", "VR_RAYGEN_WAVES", &Tuning::raygen_waves, kClamp, 0, INT_MAX, false},
    {"top_levels", "VR_TOP_LEVELS", &Tuning::top_levels, kClamp, INT_MIN, INT_MAX, true},
    {"brick_levels", "VR_BRICK_LEVELS", &Tuning::brick_levels, kClamp, INT_MIN, INT_MAX, true},
    {"brick_blocked", "VR_BRICK_BLOCKED", &Tuning::brick_blocked, kAutoFlag, 0, 0, true},
    {"max_iter", "VR_MAX_ITER", &Tuning::max_iter, kClamp, 1, INT_MAX, false},
    {"weights_check", "VR_WEIGHTS_CHECK", &Tuning::weights_check, kFlag, 0, 0, false},
    {"block_cull", "VR_BLOCK_CULL", &Tuning::block_cull, kFlag, 0, 0, false},
    {"head_march", "VR_HEAD_MARCH", &Tuning::head_march, kFlag, 0, 0, false},
    {"head_min_lanes", "VR_HEAD_MIN_LANES", &Tuning::head_min_lanes, kClamp, 0, 64, false},
    {"head_max", "VR_HEAD_MAX", &Tuning::head_max, kClamp, 0, INT_MAX, false},
};

const Knob* find_knob(const char* key) {
    for (const Knob& k : kKnobs)
        if (!strcmp(key, k.key)) return &k;
    return nullptr;
}

void set_knob(Tuning& tn, const Knob& k, int v) {
    const int clamped = v < k.lo ? k.lo : (v > k.hi ? k.hi : v);
    tn.*k.field = k.range == kFlag       ? v != 0
                  : k.range == kAutoFlag ? (v < 0 ? -1 : v != 0)
                  : k.range == kClamp64  ? (clamped > 0 && clamped < 64 ? 64 : clamped & ~63)
                                         : clamped;
}

std::mutex g_tuning_mutex;
Tuning& default_tuning_locked() {  // call with g_tuning_mutex held
    static Tuning tn = [] {
        Tuning x;
        for (const Knob& k : kKnobs)
            if (const char* e = getenv(k.env)) set_knob(x, k, atoi(e));
        return x;
    }();
    return tn;
}

uint64_t touch_granule(int which) {  // bytes one bit of the bitmap stands for
    return which == 0 ? (1ull << vr::kTouchLeafShift) : 128ull;
}
size_t touch_words(uint64_t array_bytes, int which) {  // one bit per 128-byte line
    const uint64_t g = touch_granule(which);
    return (size_t)(((array_bytes + g - 1) / g + 31) / 32);
}

}  // namespace

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

Tuning default_tuning() {
    std::lock_guard<std::mutex> g(g_tuning_mutex);
    return default_tuning_locked();
}

extern "C" {

int vr_abi_version(void) { return VR_ABI_VERSION; }

const char* vr_last_error(void) { return g_err; }

int vr_device_count(int* count) {
    if (!count) return fail(VR_ERR_INVALID_ARGUMENT, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(VR_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return VR_OK;
}

int vr_set_device(int device) {
    if (device < 0) return VR_OK;
    HIP_TRY(hipSetDevice(device));
    return VR_OK;
}

int vr_device_name(int device, char* name, size_t name_len) {
    if (!name || name_len == 0) return fail(VR_ERR_INVALID_ARGUMENT, "name buffer is NULL");
    hipDeviceProp_t prop;
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(name, name_len, "%s", prop.gcnArchName);
    return VR_OK;
}

void vr_default_tree_desc(VrTreeDesc* d) {
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->N = 2;
    d->format = VR_FORMAT_RGBA;
    d->basis_dim = -1;
    d->ndc_width = -1.f;
}

int vr_tree_info(vr_tree_t t, VrTreeInfo* info) {
    if (!t || !info) return fail(VR_ERR_INVALID_ARGUMENT, "tree/info is NULL");
    info->capacity = t->desc.capacity;
    info->N = t->desc.N;
    info->data_dim = t->desc.data_dim;
    info->format = t->desc.format;
    info->basis_dim = t->desc.basis_dim;
    info->max_depth = t->max_depth;
    info->device = t->device;
    info->device_bytes = t->device_bytes;
    info->leaf_stride = (uint64_t)t->leaf_stride_h * 2u;
    info->query_mode = t->top_levels > 0 ? VR_QUERY_LOOKUP : VR_QUERY_DESCENT;
    info->top_levels = t->top_levels;
    info->brick_levels = t->brick_levels;
    info->brick_blocked = t->brick_blocked;
    return VR_OK;
}

// The integer lookup needs exact digits of a binary32 coordinate (leaves within 24 levels: child
// words read <= 24) and 32-bit byte offsets into the node array (node * 8 + slot words < 2^30).
int vr_query_mode_for(int N, int max_depth, int64_t capacity) {
    return lookup_applies(N, max_depth, capacity) ? VR_QUERY_LOOKUP : VR_QUERY_DESCENT;
}

void vr_default_options(VrRenderOptions* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->step_size = 1e-4f;
    o->sigma_thresh = 1e-2f;
    o->stop_thresh = 1e-2f;
    o->background_brightness = 1.f;
    o->render_bbox[3] = o->render_bbox[4] = o->render_bbox[5] = 1.f;
    o->basis_minmax[0] = 0;
    o->basis_minmax[1] = VR_MAX_BASIS - 1;
    o->grid_max_depth = 4;
    o->probe[2] = 1.f;
    o->probe_disp_size = 100;
}

void vr_default_frame(VrFrame* f) {
    if (!f) return;
    memset(f, 0, sizeof(*f));
    f->offscreen = 1;
    f->layout = VR_LAYOUT_FRAME;
    f->world = 1;
    f->fp_mode = VR_FP_STRICT;
}

int64_t vr_compact_bytes(int width, int height, int tile_w, int tile_h, int world) {
    vr::KParams g;  // (rank 0 holds the most tiles)
    if (tile_geometry(width, height, tile_w, tile_h, 0, world, g) != VR_OK) return -1;
    return (int64_t)g.n_local_tiles * g.tile_w * g.tile_h * 4;
}

int vr_set_tuning(const char* key, int value) {
    if (!key) return fail(VR_ERR_INVALID_ARGUMENT, "key is NULL");
    const Knob* k = find_knob(key);
    if (!k) return fail(VR_ERR_INVALID_ARGUMENT, "unknown tuning key '%s'", key);
    std::lock_guard<std::mutex> g(g_tuning_mutex);
    set_knob(default_tuning_locked(), *k, value);
    return VR_OK;
}

int vr_tree_set_tuning(vr_tree_t t, const char* key, int value) {
    if (!t || !key) return fail(VR_ERR_INVALID_ARGUMENT, "tree/key is NULL");
    const Knob* k = find_knob(key);
    if (!k) return fail(VR_ERR_INVALID_ARGUMENT, "unknown tuning key '%s'", key);
    if (k->fixed_at_upload)
        return fail(VR_ERR_INVALID_ARGUMENT, "'%s' is fixed at upload (vr_set_tuning before it)", key);
    std::lock_guard<std::mutex> g(t->launch_mutex);
    set_knob(t->tn, *k, value);
    return VR_OK;
}

int vr_sched_stats(vr_tree_t t, uint64_t out[vr::kSchedStats], int reset) {
    if (!t || !out) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(t->device);
    HIP_TRY(hipMemcpy(out, t->sched_stats.get(), vr::kSchedStats * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(t->sched_stats.get(), 0, vr::kSchedStats * sizeof(uint64_t)));
    return VR_OK;
}

int vr_tree_cull_stats(vr_tree_t t, uint64_t out[2], int reset) {
    if (!t || !out) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(t->device);
    uint64_t lines[vr::kCullStatLines * vr::kCullStatStride];
    HIP_TRY(hipMemcpy(lines, t->cull_stats.get(), sizeof(lines), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(t->cull_stats.get(), 0, sizeof(lines)));
    out[0] = out[1] = 0;
    for (int i = 0; i < vr::kCullStatLines; ++i) {
        out[0] += lines[i * vr::kCullStatStride];
        out[1] += lines[i * vr::kCullStatStride + 1];
    }
    return VR_OK;
}

int vr_tree_head_stats(vr_tree_t t, uint64_t out[3], int reset) {
    if (!t || !out) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(t->device);
    uint64_t lines[vr::kCullStatLines * vr::kCullStatStride];
    HIP_TRY(hipMemcpy(lines, t->head_stats.get(), sizeof(lines), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(t->head_stats.get(), 0, sizeof(lines)));
    for (int k = 0; k < vr::kHeadStatWords; ++k) {
        out[k] = 0;
        for (int i = 0; i < vr::kCullStatLines; ++i) out[k] += lines[i * vr::kCullStatStride + k];
    }
    return VR_OK;
}

int vr_tree_status(vr_tree_t t, uint32_t* status, int reset) {
    if (!t || !status) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(t->device);
    HIP_TRY(hipMemcpy(status, t->status.get(), sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(t->status.get(), 0, sizeof(uint32_t)));
    return VR_OK;
}

int vr_tree_status_on(vr_tree_t t, uint32_t* status, int reset, void* stream) {
    if (!t || !status) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(t->device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    // a pinned word per calling thread: the copy is asynchronous and ordered on `hs` alone.
    // Portable: the thread may read the status of trees on several devices through it.
    thread_local uint32_t* pinned = nullptr;
    if (!pinned) HIP_TRY(hipHostMalloc((void**)&pinned, sizeof(uint32_t), hipHostMallocPortable));
    HIP_TRY(hipMemcpyAsync(pinned, t->status.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, hs));
    if (reset) HIP_TRY(hipMemsetAsync(t->status.get(), 0, sizeof(uint32_t), hs));
    HIP_TRY(hipStreamSynchronize(hs));
    *status = *pinned;
    return VR_OK;
}

int vr_touch_enable(vr_tree_t t, int enable) {
    if (!t) return fail(VR_ERR_INVALID_ARGUMENT, "tree is NULL");
    DeviceGuard guard(t->device);
    std::lock_guard<std::mutex> lock(t->launch_mutex);  // no launch is being enqueued meanwhile
    HIP_TRY(hipDeviceSynchronize());  // no launch may be using the bitmaps while they change
    for (int i = 0; i < 4; ++i) {
        HIP_TRY(t->touch[i].reset());
        const size_t words = touch_words(t->arrays[i].bytes(), i);
        if (enable && words) {
            HIP_TRY(t->touch[i].alloc(words * sizeof(uint32_t)));
            HIP_TRY(hipMemset(t->touch[i].get(), 0, words * sizeof(uint32_t)));
        }
    }
    if (enable && !t->touch_out) HIP_TRY(t->touch_out.alloc(4 * sizeof(unsigned long long)));
    return VR_OK;
}

int vr_touch_count(vr_tree_t t, uint64_t out[4], int reset) {
    if (!t || !out) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!t->touch_out) return fail(VR_ERR_INVALID_ARGUMENT, "vr_touch_enable(tree, 1) first");
    DeviceGuard guard(t->device);
    std::lock_guard<std::mutex> lock(t->launch_mutex);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(t->touch_out.get(), 0, 4 * sizeof(unsigned long long)));
    for (int i = 0; i < 4; ++i) {
        if (!t->touch[i]) continue;
        const size_t words = touch_words(t->arrays[i].bytes(), i);
        HIP_TRY(vr::launch_popcount(t->touch[i].get<uint32_t>(), words,
                                    t->touch_out.get<unsigned long long>() + i, nullptr));
        if (reset) HIP_TRY(hipMemsetAsync(t->touch[i].get(), 0, words * sizeof(uint32_t), nullptr));
    }
    HIP_TRY(hipMemcpy(out, t->touch_out.get(), 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VR_OK;
}

int vr_touch_read(vr_tree_t t, int which, uint32_t* host_words, uint64_t n_words,
                  uint64_t* bitmap_words, uint64_t* granule_bytes) {
    if (!t || which < 0 || which > 3) return fail(VR_ERR_INVALID_ARGUMENT, "tree / array index");
    if (!t->touch_out) return fail(VR_ERR_INVALID_ARGUMENT, "vr_touch_enable(tree, 1) first");
    DeviceGuard guard(t->device);
    std::lock_guard<std::mutex> lock(t->launch_mutex);
    // (an array the tree does not have -- no bricks, say -- has an empty bitmap)
    const uint64_t words = t->touch[which] ? touch_words(t->arrays[which].bytes(), which) : 0;
    if (bitmap_words) *bitmap_words = words;
    if (granule_bytes) *granule_bytes = touch_granule(which);
    const uint64_t n = n_words < words ? n_words : words;
    if (host_words && n) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(host_words, t->touch[which].get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return VR_OK;
}

int vr_assemble_tiles(void* frame_rgba, int64_t pitch, const void* gathered, int width, int height,
                      int tile_w, int tile_h, int world, void* stream) {
    if (world < 1) world = 1;
    const int64_t rank_bytes = vr_compact_bytes(width, height, tile_w, tile_h, world);
    if (rank_bytes < 0) return VR_ERR_INVALID_ARGUMENT;
    return vr_assemble_tiles_batch(frame_rgba, 0, pitch, gathered, rank_bytes, 0, 1, width, height,
                                   tile_w, tile_h, world, stream);
}

int vr_assemble_tiles_batch(void* frames_rgba, int64_t frame_stride, int64_t pitch,
                            const void* gathered, int64_t rank_stride, int64_t in_frame_stride,
                            int n_frames, int width, int height, int tile_w, int tile_h, int world,
                            void* stream) {
    if (!frames_rgba || !gathered) return fail(VR_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (n_frames < 1) return fail(VR_ERR_INVALID_ARGUMENT, "n_frames must be positive");
    if (world < 1) world = 1;
    vr::KParams g;
    if (int rc = tile_geometry(width, height, tile_w, tile_h, 0, world, g)) return rc;
    HIP_TRY(vr::launch_assemble(static_cast<uint8_t*>(frames_rgba),
                                pitch ? pitch : (int64_t)width * 4,
                                static_cast<const uint8_t*>(gathered), width, height, g.tile_w, g.tile_h, world,
                                n_frames, frame_stride, rank_stride, in_frame_stride,
                                static_cast<hipStream_t>(stream)));
    return VR_OK;
}

int vr_probe_coeffs(vr_tree_t t, const VrRenderOptions* opt, float* out_dev, void* stream) {
    if (!t || !opt || !out_dev) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(t->device);
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    fill_tree_params(k, t);
    HIP_TRY(vr::launch_probe(k, opt->probe, out_dev, static_cast<hipStream_t>(stream)));
    return VR_OK;
}

int vr_read_back(void* host_rgba, const void* dev_rgba, int64_t pitch, int width, int height,
                 void* stream) {
    if (!host_rgba || !dev_rgba) return fail(VR_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (pitch == 0) pitch = (int64_t)width * 4;
    HIP_TRY(hipMemcpy2DAsync(host_rgba, (size_t)width * 4, dev_rgba, (size_t)pitch,
                             (size_t)width * 4, (size_t)height, hipMemcpyDeviceToHost,
                             static_cast<hipStream_t>(stream)));
    return VR_OK;
}

int vr_stream_sync(void* stream) {
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return VR_OK;
}

}  // extern "C"
