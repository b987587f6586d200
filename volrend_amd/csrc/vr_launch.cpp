// vr_launch.cpp -- the march launches (include/volrend_hip.h): vr_render_batch, vr_render_aov, vr_accumulate_weights,
// vr_render_backward and their ray-list siblings vr_render_rays / vr_accumulate_weights_rays / vr_render_backward_rays
// (the backward calls also in their marked form, *_touched) and vr_fit_rays, the fused loss + backward of a list:
// argument checks, launch geometry, KParams, and the ONE sequence they all go through (run_launch).  The scheduling
// rules are vr_launch_plan.cpp, the launch-slot ring is vr_slots.cpp.  Built with -ffp-contract=off (the host-side
// Rodrigues pre-computation below must round like the oracle).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>

#include "vr_host.h"

static_assert(kPlanQueues == vr::kMaxQueues, "vr_launch_plan.h restates the queue count of vr_internal.h");

namespace {

// same rounding sequence as the oracle's norm3 (strict / fma)
float host_norm3(const float* d, int fma) {
    float s;
    if (fma) {
        s = std::fmaf(d[0], d[0], d[1] * d[1]);
        s = std::fmaf(d[2], d[2], s);
    } else {
        s = d[0] * d[0] + d[1] * d[1];
        s = d[2] * d[2] + s;
    }
    return std::sqrt(s);
}

}  // namespace

void fill_tree_params(vr::KParams& k, const VrTreeOpaque* t) {
    k.nodes = t->arrays[kNodes].get<uint32_t>();
    k.leaves = t->arrays[kLeaves].get<uint16_t>();
    k.top = t->arrays[kTop].get<uint2>();
    k.bricks = t->arrays[kBricks].get<uint32_t>();
    k.top_levels = t->top_levels;
    k.brick_levels = t->brick_levels;
    k.brick_blocked = t->brick_blocked;
    k.extra = t->extra.get<float>();
    for (int i = 0; i < 3; ++i) {
        k.offset[i] = t->desc.offset[i];
        k.scale[i] = t->desc.scale[i];
    }
    k.N = t->desc.N;
    k.N3 = t->desc.N * t->desc.N * t->desc.N;
    k.capacity = t->desc.capacity;
    k.data_dim = t->desc.data_dim;
    k.format = t->desc.format;
    k.basis_dim = t->desc.basis_dim;
    k.leaf_stride_h = t->leaf_stride_h;
    k.max_depth = t->max_depth;
    k.ndc_width = t->desc.ndc_width;
    k.ndc_height = t->desc.ndc_height;
    k.ndc_focal = t->desc.ndc_focal;
    k.status = t->status.get<uint32_t>();
    k.sched_stats = t->sched_stats.get<unsigned long long>();
    for (int i = 0; i < 4; ++i) k.touch[i] = t->touch[i].get<uint32_t>();
}

int tile_geometry(int width, int height, int tile_w, int tile_h, int rank, int world, vr::KParams& k) {
    if (width <= 0 || height <= 0) return fail(VR_ERR_INVALID_ARGUMENT, "empty image");
    if (tile_w == 0 && tile_h == 0) {
        tile_w = (width + 7) & ~7;
        tile_h = (height + 7) & ~7;
    }
    if (tile_w <= 0 || tile_h <= 0 || (tile_w & 7) || (tile_h & 7))
        return fail(VR_ERR_INVALID_ARGUMENT, "tile size %dx%d must be positive multiples of 8",
                    tile_w, tile_h);
    k.tile_w = tile_w;
    k.tile_h = tile_h;
    k.tiles_x = (width + tile_w - 1) / tile_w;
    k.tiles_y = (height + tile_h - 1) / tile_h;
    k.rank = rank;
    k.world = world < 1 ? 1 : world;
    k.n_local_tiles = (int32_t)(((int64_t)k.tiles_x * k.tiles_y - rank + k.world - 1) / k.world);
    k.wblocks_per_tile_x = tile_w / 8;
    k.wblocks_per_tile = (tile_w / 8) * (tile_h / 8);
    k.n_wave_blocks = (int64_t)k.n_local_tiles * k.wblocks_per_tile;
    return VR_OK;
}

int launch_geometry(int width, int height, int tile_w, int tile_h, int rank, int world, int n_frames,
                    vr::KParams& k) {
    // pixel coordinates travel as 16+16 bits, pixel offsets as 32 bits
    if (width < 1 || height < 1 || width > 65535 || height > 65535)
        return fail(VR_ERR_INVALID_ARGUMENT, "image size %dx%d outside [1, 65535]", width, height);
    if (int rc = tile_geometry(width, height, tile_w, tile_h, rank, world, k)) return rc;
    const int64_t total = k.n_wave_blocks * 64 * n_frames;
    if (total >= (1ll << 30))  // ray-buffer fields are addressed with 32-bit byte offsets
        return fail(VR_ERR_INVALID_ARGUMENT, "batch of %lld rays exceeds the 2^30-ray queue",
                    (long long)total);
    k.total_rays = (uint32_t)total;
    return VR_OK;
}

int list_geometry(const char* what, int64_t n, vr::KParams& k) {
    if (n < 0 || n >= (1ll << 30))  // (the limit of launch_geometry: 32-bit byte offsets into the ray buffer)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n=%lld outside [0, 2^30)", what, (long long)n);
    k.total_rays = vr::ray_list_slots(n);
    k.n_wave_blocks = k.total_rays >> 6;
    k.n_frames = n > 0 ? 1 : 0;
    k.width = vr::kRayListWidth;
    k.height = (int32_t)((n + vr::kRayListWidth - 1) >> vr::kRayListShift);
    k.fx = k.fy = 1.f;  // (nothing reads them: a list has no pixels to turn into directions)
    k.pitch = (int64_t)k.width * 4;
    k.tile_w = k.width;
    k.tile_h = (k.height + 7) & ~7;
    k.tiles_x = k.tiles_y = k.world = k.n_local_tiles = 1;
    return VR_OK;
}

namespace {  // the steps of a launch

// What a launch marches: the pixels of n_frames poses, or a list of rays.  Made at the entry point and asked
// where a launch is planned and enqueued (run_launch, enqueue_tables, the `rays` argument of vr::launch_*).
struct Views {
    const VrCamera* cams = nullptr;  // poses: cams[0 .. n_frames)
    int n_frames = 0;
    vr::RayList list{};              // a list: list.n rays
    bool is_list = false;
    const vr::RayList* rays() const { return is_list ? &list : nullptr; }
};

// The view checks: the launch has a focal length, and frame i the intrinsics of frame 0.
int check_focal(const VrCamera& cam) {
    if (!(cam.fx != 0.f) || !(cam.fy != 0.f)) return fail(VR_ERR_INVALID_ARGUMENT, "focal length must be non-zero");
    return VR_OK;
}
int check_intrinsics(const VrCamera* cams, int i) {
    if (cams[i].width != cams[0].width || cams[i].height != cams[0].height || cams[i].fx != cams[0].fx ||
        cams[i].fy != cams[0].fy)
        return fail(VR_ERR_INVALID_ARGUMENT, "frame %d: intrinsics differ within the batch", i);
    return VR_OK;
}

// the reference spins forever on step_size <= 0 (rt_core.cuh:108-175: t never advances past
// a leaf face); the kernel's iteration cap would cut such rays short silently -- refuse.
int check_step_size(const VrRenderOptions* opt) {
    if (!(opt->step_size > 0.f))
        return fail(VR_ERR_INVALID_ARGUMENT, "step_size must be positive (got %g)", (double)opt->step_size);
    return VR_OK;
}

// launch_geometry for n_frames poses with the intrinsics of `cam`, which the march reads from `k` as well.
int pose_geometry(const VrCamera& cam, int tile_w, int tile_h, int rank, int world, int n_frames, vr::KParams& k) {
    if (int rc = launch_geometry(cam.width, cam.height, tile_w, tile_h, rank, world, n_frames, k)) return rc;
    k.width = cam.width;
    k.height = cam.height;
    k.fx = cam.fx;
    k.fy = cam.fy;
    k.n_frames = n_frames;
    return VR_OK;
}

// One launch shares everything but the pose and the buffers: checks the batch against its first
// frame and leaves in `k` what the checks compute -- the launch geometry, pitch, instrumented, any_accum.
int validate_batch(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                   const VrFrame* frames, vr::KParams& k) {
    if (!t || !cams || !opt || !frames) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_frames < 1 || n_frames > VR_MAX_BATCH)
        return fail(VR_ERR_INVALID_ARGUMENT, "n_frames=%d outside [1,%d]", n_frames, VR_MAX_BATCH);
    const VrFrame* f = &frames[0];
    const VrCamera* cam = &cams[0];
    if (f->fp_mode != VR_FP_STRICT && f->fp_mode != VR_FP_FMA)
        return fail(VR_ERR_INVALID_ARGUMENT, "unknown fp_mode %d", f->fp_mode);
    if (f->layout != VR_LAYOUT_FRAME && f->layout != VR_LAYOUT_COMPACT)
        return fail(VR_ERR_INVALID_ARGUMENT, "unknown layout %d", f->layout);
    const int world = f->world < 1 ? 1 : f->world;
    if (f->rank < 0 || f->rank >= world)
        return fail(VR_ERR_INVALID_ARGUMENT, "rank %d outside world %d", f->rank, world);
    if (int rc = pose_geometry(*cam, f->tile_w, f->tile_h, f->rank, world, n_frames, k))
        return rc;
    k.pitch = f->pitch ? f->pitch : (int64_t)cam->width * 4;
    if (k.pitch < (int64_t)cam->width * 4 || k.pitch * cam->height >= (1ll << 32))
        return fail(VR_ERR_INVALID_ARGUMENT, "pitch %lld unusable for a %dx%d frame",
                    (long long)k.pitch, cam->width, cam->height);
    if (int rc = check_focal(*cam)) return rc;

    bool instrumented = false, any_accum = false;
    for (int i = 0; i < n_frames; ++i) {
        const VrFrame& fi = frames[i];
        if (!fi.rgba) return fail(VR_ERR_INVALID_ARGUMENT, "frame %d: rgba is NULL", i);
        // one launch shares everything but the pose and the buffers
        if (int rc = check_intrinsics(cams, i)) return rc;
        if (fi.pitch != f->pitch || fi.offscreen != f->offscreen || fi.layout != f->layout ||
            fi.tile_w != f->tile_w || fi.tile_h != f->tile_h || fi.rank != f->rank ||
            fi.world != f->world || fi.fp_mode != f->fp_mode)
            return fail(VR_ERR_INVALID_ARGUMENT, "frame %d: layout/shard/fp_mode differ within the batch", i);
        instrumented = instrumented || fi.counters != nullptr;
        any_accum = any_accum || fi.accum != nullptr;
    }

    if (int rc = check_step_size(opt)) return rc;
    k.instrumented = instrumented ? 1 : 0;
    k.any_accum = any_accum ? 1 : 0;
    return VR_OK;
}

// What the march reads of the caller's options (the intrinsics are in `k` with the geometry).
void fill_march_params(vr::KParams& k, const VrRenderOptions* opt) {
    k.step_size = opt->step_size;
    k.sigma_thresh = opt->sigma_thresh;
    k.stop_thresh = opt->stop_thresh;
    memcpy(k.bbox, opt->render_bbox, sizeof(k.bbox));
}

// The part of KParams that a colour launch takes from the caller: options, the launch-uniform half of
// the view-direction rotation, and how the frames are written (`f` = the first frame; a ray list: its pseudo-frame).
void fill_caller_params(vr::KParams& k, const VrRenderOptions* opt, const VrFrame* f) {
    fill_march_params(k, opt);
    k.background_brightness = opt->background_brightness;
    k.basis_min = opt->basis_minmax[0];
    k.basis_max = opt->basis_minmax[1];
    k.render_depth = opt->render_depth != 0;
    k.enable_probe = opt->enable_probe != 0;
    k.probe_disp_size = opt->probe_disp_size;

    // rodrigues (reference src/cuda/volrend.cu:57-71): angle/axis/cos/sin are
    // uniform over the frame -> once here, with the oracle's rounding sequence
    const float angle = host_norm3(opt->rot_dirs, f->fp_mode == VR_FP_FMA);
    if ((double)angle < 1e-6) {
        k.rot_enabled = 0;
    } else {
        k.rot_enabled = 1;
        for (int i = 0; i < 3; ++i) k.rot_k[i] = opt->rot_dirs[i] / angle;
        k.rot_cos = cosf(angle);
        k.rot_sin = sinf(angle);
    }
    k.offscreen = f->offscreen != 0;
    k.layout = f->layout;
}

// The part of KParams that comes from the tree's knobs, resolved for this launch (`plan`), and from what its
// basis flavour makes a ray carry.  Under the launch mutex, from the copy of the knobs the launch goes by.
void fill_tuning_params(vr::KParams& k, const VrTreeOpaque* t, const Tuning& tn, const LaunchPlan& plan) {
    k.records_nt = plan.records_nt;
    k.march_max = tn.march_max;
    k.refill_min = tn.refill_min;
    k.drain_flush = tn.drain_flush;
    k.max_iter = tn.max_iter;
    k.frame_group = plan.frame_group;
    k.super_block = plan.super_block;
    k.n_queues = plan.n_queues;
    k.chunk_max = plan.chunk_max;
    const int flavour = vr::basis_flavour(t->desc.format, t->desc.basis_dim);
    k.basis_words = vr::basis_words(flavour);
    k.ray_tail_words = vr::ray_tail_words(t->desc.format, flavour);
    k.ray_vdir = vr::ray_vdir(t->desc.format, flavour) ? 1 : 0;
}

// What a launch of a kind differs in before it enqueues: the words of its ray record (a colour ray: the head
// plus what the tree's basis flavour puts behind it) and whether it reports in the file's order.
int record_words(LaunchKind kind, int ray_tail_words) {
    return kind == LaunchKind::kWeights ? vr::kWeightRayWords
           : kind == LaunchKind::kBackward ? vr::kGradRayWords : vr::kRayWords + ray_tail_words;
}
bool needs_file_order(LaunchKind kind) { return kind == LaunchKind::kWeights || kind == LaunchKind::kBackward; }

// Whether the tree and the kernel flavour of a launch admit the lead-in march of ray generation (vr_internal.h
// "Lead-in march"): the N == 2 lookup path and the FAST flavours -- uses_lookup() and !needs_full(), asked before the
// tree's part of `k` is filled in.  (The FULL flavours' counters equal the oracle's to the integer.)
bool lead_in_applies(const VrTreeOpaque* t, const vr::KParams& k) {
    return t->desc.N == 2 && t->top_levels > 0 && t->desc.format != VR_FORMAT_SG && t->desc.format != VR_FORMAT_ASG &&
           !k.instrumented && !k.render_depth;
}

// What the enqueue step of a launch finds ready: the finished KParams, the knobs the launch goes by, the waves
// of a ray-generation workgroup, its slot, its stream, and the pixel words it asked for (else NULL).
struct Turn { const vr::KParams& k; const Tuning& tn; const LaunchPlan& plan; int gen_waves; unsigned slot; hipStream_t hs; void* extra; };

// THE launch sequence; every march launch goes through it.  `k` holds what the entry point checked and filled
// (geometry, caller's part); extra_bytes: that much more of the slot's buffer behind the records, Turn.extra
// (vr_render_rays without an rgba array: 4 bytes per ray, the march stores a pixel word per ray anyway; a frame
// launch of a tree with occupancy: its block masks); enqueue(Turn) puts tables and kernels into the
// stream, behind the slot's previous launch.  The device guard comes before the mutex.
//   * The launch mutex covers slot bookkeeping and the enqueue order of one launch, and everything that other
//     calls change under it: the knobs (vr_tree_set_tuning), the touch bitmaps (vr_touch_enable / vr_touch_count
//     (re)allocate them), the tables made on first use.  It is dropped ONCE, inside acquire_slot, while a slot
//     grows (or while the launch waits for one, all of them growing): so the launch goes by a copy of the
//     knobs, and the tree's part of `k` is filled after acquire_slot has returned -- from there to the last
//     kernel launch the mutex is held.
//   * The file-order table is made before anything else (the call's one host-blocking step), also by a warm-up
//     call -- no frames, or an empty list -- which launches nothing.
template <typename Enqueue>
int run_launch(VrTreeOpaque* t, LaunchKind kind, const Views& v, size_t extra_bytes, vr::KParams& k, void* stream,
               Enqueue&& enqueue) {
    DeviceGuard device_guard(t->device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::unique_lock<std::mutex> guard(t->launch_mutex);
    if (needs_file_order(kind))
        if (int rc = ensure_file_nodes(t)) return rc;
    if (k.n_frames == 0) return VR_OK;
    const Tuning tn = t->tn;
    const LaunchPlan plan = plan_launch(kind, v.is_list ? RaySource::kList : RaySource::kFrames, k.n_frames, v.list.n,
                                        tn, t->arrays[kTop].bytes() + t->arrays[kBricks].bytes(), lead_in_applies(t, k));
    fill_tuning_params(k, t, tn, plan);
    const size_t records = ray_buffer_bytes(k.total_rays, record_words(kind, k.ray_tail_words));
    unsigned slot;
    if (int rc = acquire_slot(t, guard, hs, k, records + extra_bytes, slot)) return rc;
    fill_tree_params(k, t);
    SlotTurn turn;
    if (int rc = turn.begin(t->slots[slot], hs)) return rc;
    void* const extra = extra_bytes ? t->slots[slot].rays.get<char>() + records : nullptr;
    return enqueue(Turn{k, tn, plan, plan.raygen_waves, slot, hs, extra});  // (`turn` records the slot's event)
}

// What vr_render_aov adds to the checks of a batch; leaves pitch and depth_world in `a`.
int validate_aov(int n_frames, const VrCamera* cams, const VrRenderOptions* opt, const VrFrame* frames,
                 const VrAov* aovs, int depth_units, vr::AovParams& a) {
    if (!aovs) return fail(VR_ERR_INVALID_ARGUMENT, "aovs is NULL");
    if (depth_units != VR_DEPTH_TREE && depth_units != VR_DEPTH_WORLD)
        return fail(VR_ERR_INVALID_ARGUMENT, "unknown depth_units %d", depth_units);
    const int64_t row = (int64_t)cams[0].width * 4;
    const int64_t pitch = aovs[0].pitch ? aovs[0].pitch : row;
    for (int i = 0; i < n_frames; ++i) {
        if (!aovs[i].depth && !aovs[i].transmittance)
            return fail(VR_ERR_INVALID_ARGUMENT, "frame %d: both AOV planes are NULL", i);
        const int64_t pi = aovs[i].pitch ? aovs[i].pitch : row;
        if (pi < row || (pi & 3))
            return fail(VR_ERR_INVALID_ARGUMENT, "frame %d: AOV pitch %lld unusable for rows of %d floats", i,
                        (long long)aovs[i].pitch, cams[0].width);
        if (pi != pitch) return fail(VR_ERR_INVALID_ARGUMENT, "frame %d: AOV pitch differs within the batch", i);
    }
    if (opt->render_depth)
        return fail(VR_ERR_UNSUPPORTED, "vr_render_aov with render_depth: the depth visualisation already is that launch");
    if (opt->enable_probe)
        return fail(VR_ERR_UNSUPPORTED, "vr_render_aov with enable_probe: pixels under the probe disc are not traced");
    for (int i = 0; i < n_frames; ++i)
        if (frames[i].counters)
            return fail(VR_ERR_UNSUPPORTED, "frame %d: vr_render_aov has no instrumented flavour (counters)", i);
    a.pitch = pitch;
    a.depth_world = depth_units == VR_DEPTH_WORLD;
    return VR_OK;
}

// The frame table (poses, and the queue reset) -> device memory, kTableChunk poses per (tiny) kernel.  A ray list
// has its one pseudo-frame and no pose.  frames = NULL: no buffers (a leaf-weight or backward launch, which
// only needs the poses and the queue reset); aovs: also the plane table of an AOV launch, through `a`.
int enqueue_tables(const vr::KParams& k, const Views& v, hipStream_t hs, const VrFrame* frames = nullptr,
                   const VrAov* aovs = nullptr, const vr::AovParams& a = vr::AovParams{},
                   const vr::MaskParams& m = vr::MaskParams{}) {
    for (int first = 0; first < k.n_frames; first += vr::kTableChunk) {
        vr::FrameTable tbl;
        memset(&tbl, 0, sizeof(tbl));
        tbl.first = first;
        tbl.n = k.n_frames - first < vr::kTableChunk ? k.n_frames - first : vr::kTableChunk;
        for (int i = 0; i < tbl.n; ++i) {
            if (!v.is_list) memcpy(tbl.f[i].xf, v.cams[first + i].transform, sizeof(tbl.f[i].xf));
            if (!frames) continue;
            tbl.f[i].rgba = static_cast<uint8_t*>(frames[first + i].rgba);
            tbl.f[i].accum = frames[first + i].accum;
            tbl.f[i].depth = frames[first + i].depth;
            tbl.f[i].counters = reinterpret_cast<VrCounters*>(frames[first + i].counters);
        }
        HIP_TRY(vr::launch_prepare(k, tbl, hs, m.mask, m.words_per_frame));  // (also clears the frames' block masks)
        if (aovs) {
            vr::AovTable at;
            memset(&at, 0, sizeof(at));
            at.first = first;
            at.n = tbl.n;
            for (int i = 0; i < at.n; ++i) {
                at.f[i].depth = aovs[first + i].depth;
                at.f[i].transmittance = aovs[first + i].transmittance;
            }
            HIP_TRY(vr::launch_prepare_aov(a, at, hs));
        }
    }
    return VR_OK;
}

// Whether the launch culls blocks (vr_internal.h "Block cull"), from the finished KParams, the knobs it goes by
// and its options.  Off: the knob; a tree without occupancy (not on the N == 2 lookup path); the FULL flavours
// (their counters equal the oracle's); sigma_thresh < 0 (a sample of sigma 0 is a hit then); an NDC tree (its rays
// are warped); a render_bbox that leaves the unit cube (samples outside it are clamped into the border leaves); a
// frame of more blocks than block_mask_kernel holds.
bool culls_blocks(const VrTreeOpaque* t, const vr::KParams& k, const Tuning& tn, const VrRenderOptions* opt) {
    if (!tn.block_cull || !t->occ || !vr::uses_lookup(k) || vr::needs_full(k)) return false;
    if (opt->sigma_thresh < 0.f || k.ndc_width > 0) return false;
    for (int i = 0; i < 3; ++i)
        if (!(opt->render_bbox[i] >= 0.f) || !(opt->render_bbox[i + 3] <= 1.f)) return false;
    return block_mask_words(k) <= (uint32_t)vr::kMaskMaxWords;
}

// The lead-in march of the launch's ray generation (vr_internal.h "Lead-in march"), as the plan says (which was
// told what lead_in_applies() found; the finished `k` must agree).
vr::HeadParams head_params(const VrTreeOpaque* t, const vr::KParams& k, const LaunchPlan& plan) {
    if (plan.head_max <= 0 || !vr::uses_lookup(k) || vr::needs_full(k)) return vr::HeadParams{};
    return vr::HeadParams{plan.head_max, plan.head_min_lanes, t->head_stats.get<unsigned long long>()};
}

// vr_render_batch (aovs = NULL) and vr_render_aov.  Into the stream go the probe pre-kernel, the frame table
// (for an AOV launch also the plane table, in the launch's slot), the block masks, ray generation + render.
int render_launch(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                  const VrFrame* frames, const VrAov* aovs, int depth_units, bool want_aov, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    vr::AovParams a;
    memset(&a, 0, sizeof(a));
    if (int rc = validate_batch(t, n_frames, cams, opt, frames, k)) return rc;
    if (want_aov)
        if (int rc = validate_aov(n_frames, cams, opt, frames, aovs, depth_units, a)) return rc;
    fill_caller_params(k, opt, &frames[0]);
    const Views v{cams, n_frames};
    const size_t mask_bytes = t->occ ? block_mask_bytes(k, n_frames) : 0;  // (room for them, whatever the knob says)
    return run_launch(t, want_aov ? LaunchKind::kAov : LaunchKind::kColour, v, mask_bytes, k, stream, [&](const Turn& u) -> int {
        a.planes = t->slot_aovs.get<vr::AovDesc>() + (size_t)u.slot * vr::kMaxBatch;
        if (u.k.enable_probe)  // launch_renderer's pre-kernel, volrend.cu:202-209
            HIP_TRY(vr::launch_probe(u.k, opt->probe, const_cast<float*>(u.k.probe_coeffs), u.hs));
        vr::MaskParams m{};
        vr::CullParams cull{};
        if (u.extra && culls_blocks(t, u.k, u.tn, opt)) {
            m.mask = static_cast<uint32_t*>(u.extra);
            m.words_per_frame = block_mask_words(u.k);
            m.nbx = (uint32_t)(u.k.tiles_x * (u.k.tile_w / 8));
            m.nby = (uint32_t)(u.k.tiles_y * (u.k.tile_h / 8));
            m.occ = t->occ.get<uint32_t>();
            m.levels = t->occ_levels;
            const int groups = 2048 / n_frames;  // workgroups that share the cell list for one frame
            m.groups_per_frame = groups < 4 ? 4 : (groups > 128 ? 128 : groups);
            cull = vr::CullParams{m.mask, m.words_per_frame, m.nbx, t->cull_stats.get<unsigned long long>()};
        }
        if (int rc = enqueue_tables(u.k, v, u.hs, frames, want_aov ? aovs : nullptr, a, m)) return rc;
        if (m.mask) HIP_TRY(vr::launch_block_mask(u.k, m, u.hs));
        const vr::HeadParams head = head_params(t, u.k, u.plan);
        if (want_aov)
            HIP_TRY(vr::launch_render_aov(u.k, a, cull, head, frames[0].fp_mode, t->n_cus, u.tn.waves_per_cu, u.gen_waves, u.hs));
        else
            HIP_TRY(vr::launch_render(u.k, cull, head, frames[0].fp_mode, t->n_cus, u.tn.waves_per_cu, u.gen_waves, u.hs));
        return VR_OK;
    });
}

// What a leaf-weight call and a backward call check of their views, without following the tree handle: FP
// model, frame count (0 = the warm-up call), step, one size and one set of intrinsics.  Leaves the launch
// geometry in `k`.
int validate_march(int n_frames, const VrCamera* cams, const VrRenderOptions* opt, int fp_mode, vr::KParams& k) {
    if (fp_mode != VR_FP_STRICT && fp_mode != VR_FP_FMA)
        return fail(VR_ERR_INVALID_ARGUMENT, "unknown fp_mode %d", fp_mode);
    if (n_frames < 0 || n_frames > VR_MAX_BATCH)
        return fail(VR_ERR_INVALID_ARGUMENT, "n_frames=%d outside [0,%d]", n_frames, VR_MAX_BATCH);
    if (int rc = check_step_size(opt)) return rc;
    if (n_frames == 0) return VR_OK;
    if (int rc = pose_geometry(cams[0], 0, 0, 0, 1, n_frames, k)) return rc;
    if (int rc = check_focal(cams[0])) return rc;
    for (int i = 1; i < n_frames; ++i)
        if (int rc = check_intrinsics(cams, i)) return rc;
    return VR_OK;
}

// Everything that can be refused without following the tree handle.
int validate_weights(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt, int fp_mode,
                     const VrLeafWeights* out, vr::KParams& k) {
    if (!t || !opt || !out || (n_frames > 0 && !cams)) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!out->max_weight && !out->hits) return fail(VR_ERR_INVALID_ARGUMENT, "both outputs are NULL");
    return validate_march(n_frames, cams, opt, fp_mode, k);
}

// The checks of a ray list that need no tree, in front of the function's own: the list itself, the FP model, the
// count and the step.  Leaves the list's geometry in `k` and the list in `v`.
int validate_rays(const char* what, vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt,
                  int fp_mode, const void* out, vr::KParams& k, Views& v) {
    if (!t || !rays || !rays->origins || !rays->dirs || !opt || !out)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (fp_mode != VR_FP_STRICT && fp_mode != VR_FP_FMA)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: unknown fp_mode %d", what, fp_mode);
    if (int rc = list_geometry(what, n, k)) return rc;
    if (int rc = check_step_size(opt)) return rc;
    v.list = vr::RayList{rays->origins, rays->dirs, n};
    v.is_list = true;
    return VR_OK;
}

// What a leaf-weight launch and a backward launch share once their arguments are checked: an offscreen frame
// without mesh depth, probe, depth mode or view-direction rotation, the pose table without buffers, and then
// launch(Turn).
template <typename Launch>
int march_launch(vr_tree_t t, LaunchKind kind, const Views& v, const VrRenderOptions* opt, vr::KParams& k, void* stream,
                 Launch&& launch) {
    fill_march_params(k, opt);
    k.offscreen = 1;
    k.layout = VR_LAYOUT_FRAME;
    k.pitch = (int64_t)k.width * 4;
    return run_launch(t, kind, v, 0, k, stream, [&](const Turn& u) -> int {
        if (int rc = enqueue_tables(u.k, v, u.hs)) return rc;
        HIP_TRY(launch(u));
        return VR_OK;
    });
}

// vr_accumulate_weights and vr_accumulate_weights_rays: `k` holds the checked geometry.
int weights_launch(vr_tree_t t, const Views& v, const VrRenderOptions* opt, int fp_mode, const VrLeafWeights* out,
                   vr::KParams& k, void* stream) {
    return march_launch(t, LaunchKind::kWeights, v, opt, k, stream, [&](const Turn& u) {
        vr::WeightParams w;
        w.max_weight = reinterpret_cast<uint32_t*>(out->max_weight);
        w.hits = out->hits;
        w.file_node = t->file_node_dev.get<int32_t>();
        return vr::launch_weights(u.k, w, fp_mode, t->n_cus, u.tn.waves_per_cu, u.gen_waves, u.tn.weights_check != 0,
                                  u.hs, v.rays());
    });
}

// ---- vr_render_backward ----

// What the backward refuses of the options without a tree (`what` names the function).
int check_backward_options(const char* what, const VrRenderOptions* opt) {
    if (opt->render_depth)
        return fail(VR_ERR_UNSUPPORTED, "%s with render_depth: the depth visualisation has no derivative here", what);
    if (opt->enable_probe)
        return fail(VR_ERR_UNSUPPORTED, "%s with enable_probe: pixels under the probe disc are not traced", what);
    if (!(opt->rot_dirs[0] == 0.f) || !(opt->rot_dirs[1] == 0.f) || !(opt->rot_dirs[2] == 0.f))
        return fail(VR_ERR_UNSUPPORTED, "%s with rot_dirs: the view direction is not rotated", what);
    return VR_OK;
}

// Everything that can be refused without following the tree handle.
int validate_backward(const char* what, vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                      int fp_mode, const float* grad_accum, const float* grad_data, vr::KParams& k) {
    if (!t || !opt || !grad_accum || !grad_data || (n_frames > 0 && !cams))
        return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int rc = validate_march(n_frames, cams, opt, fp_mode, k)) return rc;
    return check_backward_options(what, opt);
}

// What needs the tree: the formats the backward kernels shade, and the whole basis.
int check_backward_tree(const VrTreeOpaque* t, const VrRenderOptions* opt, const char* what) {
    const int format = t->desc.format, basis_dim = t->desc.basis_dim;
    if (format == VR_FORMAT_SG || format == VR_FORMAT_ASG)
        return fail(VR_ERR_UNSUPPORTED, "%s: SG / ASG trees are not supported", what);
    if (vr::basis_flavour(format, basis_dim) != vr::BASIS_RGBA &&
        (opt->basis_minmax[0] > 0 || opt->basis_minmax[1] < basis_dim - 1))
        return fail(VR_ERR_UNSUPPORTED, "%s: basis_minmax [%d, %d] leaves out basis functions of the tree (%d)", what,
                    opt->basis_minmax[0], opt->basis_minmax[1], basis_dim);
    return VR_OK;
}

// vr_render_backward, vr_render_backward_rays and their marked siblings (`what`; touched = NULL: unmarked), as
// weights_launch.
int backward_launch(const char* what, vr_tree_t t, const Views& v, const VrRenderOptions* opt, int fp_mode,
                    const float* grad_accum, float* grad_data, uint32_t* touched, vr::KParams& k, void* stream) {
    if (int rc = check_backward_tree(t, opt, what)) return rc;
    return march_launch(t, LaunchKind::kBackward, v, opt, k, stream, [&](const Turn& u) {
        vr::GradParams g;
        g.grad_accum = grad_accum;
        g.grad_data = grad_data;
        g.file_node = t->file_node_dev.get<int32_t>();
        g.touched = touched;  // (NULL: the unmarked kernels)
        return vr::launch_grad(u.k, g, fp_mode, t->n_cus, u.tn.waves_per_cu, u.gen_waves, u.hs, v.rays());
    });
}

// vr_render_backward_rays (touched = NULL) and vr_render_backward_rays_touched (`what`).
int backward_rays(const char* what, vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt,
                  int fp_mode, const float* grad_accum, float* grad_data, uint32_t* touched, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    Views v;
    if (!grad_accum) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (int rc = validate_rays(what, t, n, rays, opt, fp_mode, grad_data, k, v)) return rc;
    if (int rc = check_backward_options(what, opt)) return rc;
    return backward_launch(what, t, v, opt, fp_mode, grad_accum, grad_data, touched, k, stream);
}

}  // namespace

extern "C" {

int vr_render_backward(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt, int fp_mode,
                       const float* grad_accum, float* grad_data, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    if (int rc = validate_backward("vr_render_backward", t, n_frames, cams, opt, fp_mode, grad_accum, grad_data, k)) return rc;
    return backward_launch("vr_render_backward", t, Views{cams, n_frames}, opt, fp_mode, grad_accum, grad_data, nullptr,
                           k, stream);
}

int vr_render_backward_touched(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt, int fp_mode,
                               const float* grad_accum, float* grad_data, uint32_t* touched, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    if (!touched) return fail(VR_ERR_INVALID_ARGUMENT, "vr_render_backward_touched: NULL argument");
    if (int rc = validate_backward("vr_render_backward_touched", t, n_frames, cams, opt, fp_mode, grad_accum, grad_data, k))
        return rc;
    return backward_launch("vr_render_backward_touched", t, Views{cams, n_frames}, opt, fp_mode, grad_accum, grad_data,
                           touched, k, stream);
}

int vr_render_backward_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                            const float* grad_accum, float* grad_data, void* stream) {
    return backward_rays("vr_render_backward_rays", t, n, rays, opt, fp_mode, grad_accum, grad_data, nullptr, stream);
}

int vr_render_backward_rays_touched(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                                    const float* grad_accum, float* grad_data, uint32_t* touched, void* stream) {
    if (!touched) return fail(VR_ERR_INVALID_ARGUMENT, "vr_render_backward_rays_touched: NULL argument");
    return backward_rays("vr_render_backward_rays_touched", t, n, rays, opt, fp_mode, grad_accum, grad_data, touched,
                         stream);
}

// vr_fit_rays: the checks of backward_rays (its `out` is the VrFit), then a backward launch whose march forms
// grad_accum itself.
int vr_fit_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode, const VrFit* fit,
                void* stream) {
    const char* const what = "vr_fit_rays";
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    Views v;
    if (int rc = validate_rays(what, t, n, rays, opt, fp_mode, fit, k, v)) return rc;
    if (!fit->target || !fit->grad_data) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (!std::isfinite(fit->grad_scale))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: grad_scale must be finite (got %g)", what, (double)fit->grad_scale);
    if (int rc = check_backward_options(what, opt)) return rc;
    if (int rc = check_backward_tree(t, opt, what)) return rc;
    return march_launch(t, LaunchKind::kBackward, v, opt, k, stream, [&](const Turn& u) {
        vr::FitParams f;
        f.target = fit->target;
        f.grad_data = fit->grad_data;
        f.file_node = t->file_node_dev.get<int32_t>();
        f.touched = fit->touched;
        f.sq_err = fit->sq_err;
        f.accum = fit->accum;
        f.bg = opt->background_brightness;
        f.grad_scale = fit->grad_scale;
        return vr::launch_fit(u.k, f, fp_mode, t->n_cus, u.tn.waves_per_cu, u.gen_waves, u.hs, v.rays());
    });
}

int vr_accumulate_weights(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                          int fp_mode, const VrLeafWeights* out, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    if (int rc = validate_weights(t, n_frames, cams, opt, fp_mode, out, k)) return rc;
    return weights_launch(t, Views{cams, n_frames}, opt, fp_mode, out, k, stream);
}

int vr_accumulate_weights_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                               const VrLeafWeights* out, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    Views v;
    if (int rc = validate_rays("vr_accumulate_weights_rays", t, n, rays, opt, fp_mode, out, k, v)) return rc;
    if (!out->max_weight && !out->hits)
        return fail(VR_ERR_INVALID_ARGUMENT, "vr_accumulate_weights_rays: both outputs are NULL");
    return weights_launch(t, v, opt, fp_mode, out, k, stream);
}

// One colour launch of a ray list: the list's pseudo-frame for the frame table.  A call without rgba still has
// the march store a pixel word per ray: into the pixel words of the launch's slot.
int vr_render_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                   const VrRayOut* out, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    Views v;
    if (int rc = validate_rays("vr_render_rays", t, n, rays, opt, fp_mode, out, k, v)) return rc;
    if (!out->rgba && !out->accum) return fail(VR_ERR_INVALID_ARGUMENT, "vr_render_rays: both outputs are NULL");
    if (opt->render_depth)
        return fail(VR_ERR_UNSUPPORTED, "vr_render_rays with render_depth: the depth visualisation is not what a ray list is for");
    if (opt->enable_probe)
        return fail(VR_ERR_UNSUPPORTED, "vr_render_rays with enable_probe: the probe disc is a set of pixel positions");
    if (n == 0) return VR_OK;
    VrFrame f;  // the pseudo-frame
    memset(&f, 0, sizeof(f));
    f.offscreen = 1;
    f.layout = VR_LAYOUT_FRAME;
    f.fp_mode = fp_mode;
    f.accum = out->accum;
    fill_caller_params(k, opt, &f);
    k.any_accum = out->accum ? 1 : 0;
    const size_t pixel_bytes = out->rgba ? 0 : list_pixel_bytes(k.total_rays);
    return run_launch(t, LaunchKind::kColour, v, pixel_bytes, k, stream, [&](const Turn& u) -> int {
        f.rgba = out->rgba ? out->rgba : u.extra;
        if (int rc = enqueue_tables(u.k, v, u.hs, &f)) return rc;
        HIP_TRY(vr::launch_render(u.k, vr::CullParams{}, vr::HeadParams{}, fp_mode, t->n_cus, u.tn.waves_per_cu, u.gen_waves, u.hs, v.rays()));
        return VR_OK;
    });
}

int vr_render_batch(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                    const VrFrame* frames, void* stream) {
    return render_launch(t, n_frames, cams, opt, frames, nullptr, 0, false, stream);
}

int vr_render_aov(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                  const VrFrame* frames, const VrAov* aovs, int depth_units, void* stream) {
    return render_launch(t, n_frames, cams, opt, frames, aovs, depth_units, true, stream);
}

int vr_render(vr_tree_t t, const VrCamera* cam, const VrRenderOptions* opt, const VrFrame* f,
              void* stream) {
    return vr_render_batch(t, 1, cam, opt, f, stream);
}

}  // extern "C"
