// vr_launch.cpp -- launches (include/volrend_hip.h): vr_render_batch, vr_render_aov, vr_accumulate_weights,
// vr_render_backward, their ray-list siblings vr_render_rays / vr_accumulate_weights_rays /
// vr_render_backward_rays, vr_reserve*, vr_tree_status*, the value passes vr_tree_update_data / vr_tree_read_data
// (which share the file-order table of the march launches), the launch geometry and the launch-slot ring.  Built with -ffp-contract=off (the host-side
// Rodrigues pre-computation below must round like the oracle).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>

#include "vr_host.h"

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

// what a ray of this tree carries behind the head of its record (vr_internal.h)
int ray_tail_words_of(const VrTreeOpaque* t) {
    return vr::ray_tail_words(t->desc.format, vr::basis_flavour(t->desc.format, t->desc.basis_dim));
}

size_t ray_buffer_bytes(uint32_t total_rays, int words_per_ray) {
    return vr::ray_slots(total_rays) * (size_t)words_per_ray * sizeof(uint32_t);
}

// vr_render_rays without an rgba array: the pixel words the march stores anyway, behind the records
size_t list_pixel_bytes(uint32_t total_rays) { return (size_t)total_rays * 4; }

// Replaces the ray buffer of a slot the caller owns (it holds the launch mutex, or has marked the
// slot `growing` and dropped it) by one of `bytes`.  The slot's last launch must have finished
// before its buffer goes; if that wait fails the buffer is still freed (hipFree synchronises by
// itself): only a failing allocation fails, and nothing is leaked either way.
hipError_t replace_ray_buffer(LaunchSlot& ls, size_t bytes) {
    if (ls.rays) {
        if (ls.used) (void)hipEventSynchronize(ls.done.get());
        (void)ls.rays.reset();
        (void)hipGetLastError();
    }
    return ls.rays.alloc(bytes);
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

namespace {  // the steps of a launch: vr_render_batch, vr_render_aov, vr_accumulate_weights, vr_render_backward

// launch_geometry for a list of n rays (vr::RayList): the one pseudo-frame of vr::kRayListWidth pixels a row
// whose pixel y * width + x is ray i, as whole blocks of 64 rays.  `what` names the function in the refusal.
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
    if (int rc = launch_geometry(cam->width, cam->height, f->tile_w, f->tile_h, f->rank, world, n_frames, k))
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
    k.n_frames = n_frames;
    k.instrumented = instrumented ? 1 : 0;
    k.any_accum = any_accum ? 1 : 0;
    return VR_OK;
}

// What the march reads of the caller's arguments: the intrinsics (cam = NULL: a ray list, whose pseudo-frame
// list_geometry left in `k`) and four options.
void fill_march_params(vr::KParams& k, const VrCamera* cam, const VrRenderOptions* opt) {
    if (cam) {
        k.width = cam->width;
        k.height = cam->height;
        k.fx = cam->fx;
        k.fy = cam->fy;
    }
    k.step_size = opt->step_size;
    k.sigma_thresh = opt->sigma_thresh;
    k.stop_thresh = opt->stop_thresh;
    memcpy(k.bbox, opt->render_bbox, sizeof(k.bbox));
}

// The part of KParams that comes from the caller: intrinsics, options, the launch-uniform half of
// the view-direction rotation, and how the frames are written (`f` = the first frame; cam = NULL: a ray list).
void fill_caller_params(vr::KParams& k, const VrCamera* cam, const VrRenderOptions* opt, const VrFrame* f) {
    fill_march_params(k, cam, opt);
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

// The knobs that are "auto" (0) by default, resolved for one launch.  `colour`: a colour or AOV launch
// (render_kernel / render_aov_kernel); the leaf-weight and backward launches keep the values they were
// measured with (guided chunks of up to 4096 rays, row-major block order).
//   * chunk_max: the cap of a wave's guided chunk (grab_chunk, vr_dev_rays.h).  256 for colour launches of
//     any shape: four block-poses.  With 4096 one wave marched an 8x8 pixel block through all the poses of a
//     64-frame launch, one after the other, and the lines it fetched for pose k were long evicted from its
//     XCD's L2 at pose k + 1; with 256 the poses of a block go to 16 waves of the XCD at about the same time
//     (fabric reads per C1 frame -7 %).  Below 256 the reads fall further (-24 % at 64) and the time RISES:
//     a wave whose lanes hold unrelated blocks loses more in its own L1 than the L2 gains -- also with
//     grabs that cost the wave no latency (EXPERIMENTS.md, round 7).  Small launches never reach the cap:
//     the guided size of a one-frame launch is 64.
//   * super_block: 4 (blocks visited in 4 x 4 super-blocks: consecutive chunks are screen neighbours in
//     both directions) for launches of three frames and more, row-major for the small ones, which it
//     costs 2 % (measured at one frame; four frames: no difference).
// A colour launch of a ray list takes the colour rule's 256; super_block orders the blocks of a SCREEN and is
// never consulted for a list (its ray generation does not call locate()).
constexpr int kColourChunkCap = 256, kGuidedChunkCap = 4096;
int auto_chunk_max(const Tuning& tn, bool colour) {
    return tn.chunk_max > 0 ? tn.chunk_max : colour ? kColourChunkCap : kGuidedChunkCap;
}
int auto_super_block(const Tuning& tn, bool colour, int n_frames) {
    return tn.super_block > 0 ? tn.super_block : (colour && n_frames > 2) ? 4 : 1;
}

// The part of KParams that comes from the tree's knobs and from what its basis flavour makes a ray
// carry.  Under the launch mutex, from the copy of the knobs the launch goes by.
void fill_tuning_params(vr::KParams& k, const VrTreeOpaque* t, const Tuning& tn, bool colour) {
    // lookup structure (top + bricks) beyond 4x the aggregate L2 (8 x 4 MiB on MI355X): the record
    // stream would keep evicting it -- see the DMA loads in vr_render.hip
    k.records_nt = tn.records_nt >= 0 ? tn.records_nt
                                      : (t->arrays[kTop].bytes() + t->arrays[kBricks].bytes() > (128ull << 20));
    k.march_max = tn.march_max;
    k.refill_min = tn.refill_min;
    k.drain_flush = tn.drain_flush;
    k.max_iter = tn.max_iter;
    k.frame_group = tn.frame_group < 1 || tn.frame_group > k.n_frames ? k.n_frames : tn.frame_group;
    k.super_block = auto_super_block(tn, colour, k.n_frames);
    k.n_queues = tn.xcd_queues ? vr::kMaxQueues : 1;
    k.chunk_max = auto_chunk_max(tn, colour);
    const int flavour = vr::basis_flavour(t->desc.format, t->desc.basis_dim);
    k.basis_words = vr::basis_words(flavour);
    k.ray_tail_words = vr::ray_tail_words(t->desc.format, flavour);
    k.ray_vdir = vr::ray_vdir(t->desc.format, flavour) ? 1 : 0;
}

// Launch slot: per-launch scratch in device memory (ring, see LaunchSlot).  Picks the slot of this
// launch, points `k` at its scratch and makes its ray buffer large enough (`need` bytes).  `guard` holds the
// launch mutex on entry and on return.
int acquire_slot(VrTreeOpaque* t, std::unique_lock<std::mutex>& guard, hipStream_t hs, vr::KParams& k,
                 size_t need, unsigned& slot) {
    slot = kLaunchSlots;
    for (int want_fit = 1; want_fit >= 0 && slot == kLaunchSlots; --want_fit) {
        for (int pass = 0; pass < 2 && slot == kLaunchSlots; ++pass)
            for (unsigned i = 0; i < kLaunchSlots; ++i) {
                const LaunchSlot& c = t->slots[i];
                if (c.growing || (want_fit && c.rays.bytes() < need)) continue;
                const bool ok = pass == 0 ? (c.used && c.last_stream == hs)
                                          : (!c.used || hipEventQuery(c.done.get()) == hipSuccess);
                if (ok) {
                    slot = i;
                    break;
                }
            }
    }
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is an answer, not an error
    if (slot == kLaunchSlots) {  // all busy elsewhere: queue up behind one (not one that is growing)
        for (unsigned a = 0; a < kLaunchSlots && slot == kLaunchSlots; ++a)
            if (!t->slots[(t->launch_seq + a) % kLaunchSlots].growing) slot = (t->launch_seq + a) % kLaunchSlots;
        if (slot == kLaunchSlots)
            return fail(VR_ERR_HIP, "all %u launch slots are being resized by other threads", kLaunchSlots);
    }
    t->launch_seq++;
    LaunchSlot& ls = t->slots[slot];
    k.frames = t->slot_frames.get<vr::FrameDesc>() + (size_t)slot * vr::kMaxBatch;
    k.queue_head = t->slot_heads.get<uint32_t>() + vr::kSlotWords * slot + vr::kSlotHeaderWords;
    k.probe_coeffs = t->probe_buf.get<float>() + (size_t)slot * (size_t)t->desc.data_dim;
    if (ls.rays.bytes() < need) {
        // First use of the slot, or a larger batch than any before: (re)allocate.  This is the
        // one place where an enqueue-only call may block -- on THIS slot's previous launch
        // only, and hipFree/hipMalloc may synchronise the device; vr_reserve() / vr_reserve_tiles()
        // move it out of the render loop.
        // The wait, the free and the allocation run WITHOUT the launch mutex: the slot is marked
        // `growing` (nobody else picks it) and other threads keep enqueueing on the other slots.
        ls.growing = true;
        guard.unlock();
        const hipError_t ge = replace_ray_buffer(ls, need);
        guard.lock();
        ls.growing = false;
        fill_tree_params(k, t);  // (the mutex was dropped: vr_touch_enable / vr_touch_count (re)allocate the bitmaps)
        if (ge != hipSuccess)
            return fail(hip_code(ge), "ray buffer of %zu bytes: %s", need, hipGetErrorString(ge));
    }
    k.ray_buf_rw = ls.rays.get<uint32_t>();
    k.ray_buf = k.ray_buf_rw;
    return VR_OK;
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

// A launch's turn at its slot; begin() is the only way to take one.  Whoever used the slot last (any stream)
// must have finished before its scratch is rewritten: begin() makes the stream wait for it (a failed wait
// leaves the slot as it was).  From then on kernels of the launch may be in the stream: whatever happens
// afterwards (a later enqueue failing), the slot's event is recorded behind them and the slot is marked used,
// so that the next user of the slot -- any stream -- waits for whatever did get enqueued.
class SlotTurn {
    LaunchSlot* slot_ = nullptr;
    hipStream_t stream_ = nullptr;
public:
    int begin(LaunchSlot& ls, hipStream_t hs) {
        if (ls.used) HIP_TRY(hipStreamWaitEvent(hs, ls.done.get(), 0));
        slot_ = &ls;
        stream_ = hs;
        return VR_OK;
    }
    ~SlotTurn() {
        if (!slot_) return;
        if (hipEventRecord(slot_->done.get(), stream_) == hipSuccess) {
            slot_->used = true;
            slot_->last_stream = stream_;
        } else {
            (void)hipGetLastError();
        }
    }
};

// The frame table (poses, and the queue reset) -> device memory, kTableChunk poses per (tiny) kernel.
// frames = NULL: poses alone (a leaf-weight launch); aovs: also the plane table of an AOV launch, through `a`.
int enqueue_tables(const vr::KParams& k, const VrCamera* cams, hipStream_t hs, const VrFrame* frames = nullptr,
                   const VrAov* aovs = nullptr, const vr::AovParams& a = vr::AovParams{}) {
    for (int first = 0; first < k.n_frames; first += vr::kTableChunk) {
        vr::FrameTable tbl;
        memset(&tbl, 0, sizeof(tbl));
        tbl.first = first;
        tbl.n = k.n_frames - first < vr::kTableChunk ? k.n_frames - first : vr::kTableChunk;
        for (int i = 0; i < tbl.n; ++i) {
            memcpy(tbl.f[i].xf, cams[first + i].transform, sizeof(tbl.f[i].xf));
            if (!frames) continue;
            tbl.f[i].rgba = static_cast<uint8_t*>(frames[first + i].rgba);
            tbl.f[i].accum = frames[first + i].accum;
            tbl.f[i].depth = frames[first + i].depth;
            tbl.f[i].counters = reinterpret_cast<VrCounters*>(frames[first + i].counters);
        }
        HIP_TRY(vr::launch_prepare(k, tbl, hs));
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

// The same for a ray list: its one pseudo-frame (no pose; rgba / accum = the arrays ray i indexes, NULL for a
// leaf-weight or backward launch, which only needs the queue reset).
int enqueue_list_table(const vr::KParams& k, void* rgba, float* accum, hipStream_t hs) {
    vr::FrameTable tbl;
    memset(&tbl, 0, sizeof(tbl));
    tbl.n = 1;
    tbl.f[0].rgba = static_cast<uint8_t*>(rgba);
    tbl.f[0].accum = accum;
    HIP_TRY(vr::launch_prepare(k, tbl, hs));
    return VR_OK;
}

// waves per ray-generation workgroup: 16 (one atomic per 1024 pixels) -- except launches of one or
// two frames, the ones that run beside the tail of a neighbour on another stream: workgroups of
// 4 waves find room there much earlier (vr_render.hip raygen_kernel; profiles/r06_raygen_waves.jsonl:
// two streams -10 % / -6.5 % at one / two frames per launch, one stream +-0; from four frames on the
// 4x atomics cost a lone launch 3-4 %, and one-wave workgroups 35 %)
int raygen_waves(const Tuning& tn, int n_frames) {
    return tn.raygen_waves > 0 ? tn.raygen_waves : (n_frames <= 2 ? 4 : 16);
}
// A ray list: the same reasoning by ray count.  The frame rule was measured at 800 x 800 pixels, where "two
// frames" are 1 280 000 rays: lists up to kRayListSmall rays -- an optimiser's step, which runs beside the tail
// of the step before it -- generate in workgroups of 4 waves, larger ones in 16.  UNMEASURED for lists: the
// boundary is the frame rule's, restated in rays.  (List ray generation has no one-wave flavour.)
constexpr int64_t kRayListSmall = 2 * 800 * 800;
int raygen_waves_list(const Tuning& tn, int64_t n) {
    return tn.raygen_waves > 0 ? (tn.raygen_waves >= 16 ? 16 : 4) : (n <= kRayListSmall ? 4 : 16);
}

// vr_render_batch (aovs = NULL) and vr_render_aov: one launch, in steps.  Into the stream go, behind the slot's
// previous launch: the probe pre-kernel, the frame table (for an AOV launch also the plane table), ray
// generation + render.
int render_launch(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                  const VrFrame* frames, const VrAov* aovs, int depth_units, bool want_aov, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    vr::AovParams a;
    memset(&a, 0, sizeof(a));
    if (int rc = validate_batch(t, n_frames, cams, opt, frames, k)) return rc;
    if (want_aov)
        if (int rc = validate_aov(n_frames, cams, opt, frames, aovs, depth_units, a)) return rc;
    DeviceGuard device_guard(t->device);
    fill_caller_params(k, &cams[0], opt, &frames[0]);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::unique_lock<std::mutex> guard(t->launch_mutex);
    fill_tree_params(k, t);  // (under the mutex: vr_touch_enable / vr_touch_count (re)allocate the bitmaps)
    const Tuning tn = t->tn;  // (a copy: the mutex is dropped once in acquire_slot, while a slot grows)
    fill_tuning_params(k, t, tn, true);
    unsigned slot;
    if (int rc = acquire_slot(t, guard, hs, k, ray_buffer_bytes(k.total_rays, vr::kRayWords + k.ray_tail_words), slot)) return rc;
    a.planes = t->slot_aovs.get<vr::AovDesc>() + (size_t)slot * vr::kMaxBatch;
    SlotTurn turn;
    if (int rc = turn.begin(t->slots[slot], hs)) return rc;
    if (k.enable_probe)  // launch_renderer's pre-kernel, volrend.cu:202-209
        HIP_TRY(vr::launch_probe(k, opt->probe, const_cast<float*>(k.probe_coeffs), hs));
    if (int rc = enqueue_tables(k, cams, hs, frames, want_aov ? aovs : nullptr, a)) return rc;
    const int gen_waves = raygen_waves(tn, n_frames);
    if (want_aov)
        HIP_TRY(vr::launch_render_aov(k, a, frames[0].fp_mode, t->n_cus, tn.waves_per_cu, gen_waves, hs));
    else
        HIP_TRY(vr::launch_render(k, frames[0].fp_mode, t->n_cus, tn.waves_per_cu, gen_waves, hs));
    return VR_OK;  // (`turn` records the slot's event)
}

// ---- vr_accumulate_weights ----

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
    if (int rc = launch_geometry(cams[0].width, cams[0].height, 0, 0, 0, 1, n_frames, k)) return rc;
    if (int rc = check_focal(cams[0])) return rc;
    for (int i = 1; i < n_frames; ++i)
        if (int rc = check_intrinsics(cams, i)) return rc;
    k.n_frames = n_frames;
    return VR_OK;
}

// Everything that can be refused without following the tree handle.
int validate_weights(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt, int fp_mode,
                     const VrLeafWeights* out, vr::KParams& k) {
    if (!t || !opt || !out || (n_frames > 0 && !cams)) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!out->max_weight && !out->hits) return fail(VR_ERR_INVALID_ARGUMENT, "both outputs are NULL");
    return validate_march(n_frames, cams, opt, fp_mode, k);
}

// The device copy of the tree's device-node -> file-node table, made on the first call (under the launch
// mutex; the call's one host-blocking step).
int ensure_file_nodes(VrTreeOpaque* t) {
    if (t->file_node_dev) return VR_OK;
    const size_t bytes = t->file_node.size() * sizeof(int32_t);
    if (bytes != (size_t)t->desc.capacity * sizeof(int32_t))
        return fail(VR_ERR_HIP, "the tree carries no file-order table");
    hipError_t e = t->file_node_dev.alloc(bytes);
    if (e == hipSuccess) e = hipMemcpy(t->file_node_dev.get(), t->file_node.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)t->file_node_dev.reset();
        return fail(hip_code(e), "file-order table of %zu bytes: %s", bytes, hipGetErrorString(e));
    }
    t->device_bytes += bytes;
    return VR_OK;
}

// What a leaf-weight launch and a backward launch share once their arguments are checked: the file-order
// table, an offscreen frame without mesh depth, probe, depth mode or view-direction rotation, a slot for rays
// of `ray_words` words, the pose table (cams = NULL, a ray list: `rays`, the pseudo-frame), and then
// launch(k, tuning, waves per ray-generation workgroup, stream).
template <typename Launch>
int march_launch(vr_tree_t t, int n_frames, const VrCamera* cams, const vr::RayList* rays, const VrRenderOptions* opt,
                 vr::KParams& k, int ray_words, void* stream, Launch&& launch) {
    DeviceGuard device_guard(t->device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::unique_lock<std::mutex> guard(t->launch_mutex);
    if (int rc = ensure_file_nodes(t)) return rc;
    if (n_frames == 0) return VR_OK;  // the warm-up call (a ray list: n == 0)
    fill_march_params(k, cams ? &cams[0] : nullptr, opt);  // (cams = NULL: a ray list, `k` holds list_geometry's frame)
    k.offscreen = 1;
    k.layout = VR_LAYOUT_FRAME;
    k.pitch = (int64_t)k.width * 4;
    fill_tree_params(k, t);
    const Tuning tn = t->tn;  // (a copy: the mutex is dropped once in acquire_slot, while a slot grows)
    fill_tuning_params(k, t, tn, false);
    unsigned slot;
    if (int rc = acquire_slot(t, guard, hs, k, ray_buffer_bytes(k.total_rays, ray_words), slot)) return rc;
    SlotTurn turn;
    if (int rc = turn.begin(t->slots[slot], hs)) return rc;
    if (int rc = cams ? enqueue_tables(k, cams, hs) : enqueue_list_table(k, nullptr, nullptr, hs)) return rc;
    HIP_TRY(launch(k, tn, rays ? raygen_waves_list(tn, rays->n) : raygen_waves(tn, n_frames), hs));
    return VR_OK;  // (`turn` records the slot's event)
}

// The checks of a ray list that need no tree, in front of the function's own: the list itself, the FP model, the
// count and the step.  Leaves the list's geometry in `k` and the list in `rl`.
int validate_rays(const char* what, vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt,
                  int fp_mode, const void* out, vr::KParams& k, vr::RayList& rl) {
    if (!t || !rays || !rays->origins || !rays->dirs || !opt || !out)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (fp_mode != VR_FP_STRICT && fp_mode != VR_FP_FMA)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: unknown fp_mode %d", what, fp_mode);
    if (int rc = list_geometry(what, n, k)) return rc;
    if (int rc = check_step_size(opt)) return rc;
    rl.origins = rays->origins;
    rl.dirs = rays->dirs;
    rl.n = n;
    return VR_OK;
}

// vr_accumulate_weights (rays = NULL) and vr_accumulate_weights_rays (cams = NULL; n_frames = 1, or 0 for an
// empty list): `k` holds the checked geometry.
int accumulate_weights(vr_tree_t t, int n_frames, const VrCamera* cams, const vr::RayList* rays,
                       const VrRenderOptions* opt, int fp_mode, const VrLeafWeights* out, vr::KParams& k, void* stream) {
    return march_launch(t, n_frames, cams, rays, opt, k, vr::kWeightRayWords, stream,
                        [&](const vr::KParams& kp, const Tuning& tn, int gen, hipStream_t hs) {
                            vr::WeightParams w;
                            w.max_weight = reinterpret_cast<uint32_t*>(out->max_weight);
                            w.hits = out->hits;
                            w.file_node = t->file_node_dev.get<int32_t>();
                            return vr::launch_weights(kp, w, fp_mode, t->n_cus, tn.waves_per_cu, gen,
                                                      tn.weights_check != 0, hs, rays);
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
int validate_backward(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt, int fp_mode,
                      const float* grad_accum, const float* grad_data, vr::KParams& k) {
    if (!t || !opt || !grad_accum || !grad_data || (n_frames > 0 && !cams))
        return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int rc = validate_march(n_frames, cams, opt, fp_mode, k)) return rc;
    return check_backward_options("vr_render_backward", opt);
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

// vr_render_backward (rays = NULL) and vr_render_backward_rays (cams = NULL), as accumulate_weights.
int render_backward(vr_tree_t t, int n_frames, const VrCamera* cams, const vr::RayList* rays,
                    const VrRenderOptions* opt, int fp_mode, const float* grad_accum, float* grad_data,
                    vr::KParams& k, void* stream) {
    if (int rc = check_backward_tree(t, opt, rays ? "vr_render_backward_rays" : "vr_render_backward")) return rc;
    return march_launch(t, n_frames, cams, rays, opt, k, vr::kGradRayWords, stream,
                        [&](const vr::KParams& kp, const Tuning& tn, int gen, hipStream_t hs) {
                            vr::GradParams g;
                            g.grad_accum = grad_accum;
                            g.grad_data = grad_data;
                            g.file_node = t->file_node_dev.get<int32_t>();
                            return vr::launch_grad(kp, g, fp_mode, t->n_cus, tn.waves_per_cu, gen, hs, rays);
                        });
}

// ---- vr_render_rays ----

// One colour launch of a ray list: render_launch's steps with the list's pseudo-frame for the frame table.  A
// call without rgba still has the march store a pixel word per ray: 4 bytes per ray of the slot's ray buffer,
// behind the records.
int render_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                const VrRayOut* out, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    vr::RayList rl;
    if (int rc = validate_rays("vr_render_rays", t, n, rays, opt, fp_mode, out, k, rl)) return rc;
    if (!out->rgba && !out->accum) return fail(VR_ERR_INVALID_ARGUMENT, "vr_render_rays: both outputs are NULL");
    if (opt->render_depth)
        return fail(VR_ERR_UNSUPPORTED, "vr_render_rays with render_depth: the depth visualisation is not what a ray list is for");
    if (opt->enable_probe)
        return fail(VR_ERR_UNSUPPORTED, "vr_render_rays with enable_probe: the probe disc is a set of pixel positions");
    if (n == 0) return VR_OK;
    DeviceGuard device_guard(t->device);
    VrFrame f;
    memset(&f, 0, sizeof(f));
    f.offscreen = 1;
    f.layout = VR_LAYOUT_FRAME;
    f.fp_mode = fp_mode;
    fill_caller_params(k, nullptr, opt, &f);
    k.any_accum = out->accum ? 1 : 0;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::unique_lock<std::mutex> guard(t->launch_mutex);
    fill_tree_params(k, t);  // (under the mutex: vr_touch_enable / vr_touch_count (re)allocate the bitmaps)
    const Tuning tn = t->tn;  // (a copy: the mutex is dropped once in acquire_slot, while a slot grows)
    fill_tuning_params(k, t, tn, true);
    const size_t records = ray_buffer_bytes(k.total_rays, vr::kRayWords + k.ray_tail_words);
    unsigned slot;
    if (int rc = acquire_slot(t, guard, hs, k, records + (out->rgba ? 0 : list_pixel_bytes(k.total_rays)), slot)) return rc;
    void* const rgba = out->rgba ? out->rgba : static_cast<void*>(t->slots[slot].rays.get<char>() + records);
    SlotTurn turn;
    if (int rc = turn.begin(t->slots[slot], hs)) return rc;
    if (int rc = enqueue_list_table(k, rgba, out->accum, hs)) return rc;
    HIP_TRY(vr::launch_render(k, fp_mode, t->n_cus, tn.waves_per_cu, raygen_waves_list(tn, n), hs, &rl));
    return VR_OK;  // (`turn` records the slot's event)
}

// ---- vr_tree_update_data / vr_tree_read_data ----

// The device copy of the brick-root table (brick -> its node), which the refresh of the bricks reads: made
// like the file-order table, on the first call, under the launch mutex.  Trees without bricks have none.
int ensure_brick_roots(VrTreeOpaque* t) {
    if (t->brick_root_dev || t->top_levels <= 0 || t->n_bricks <= 0) return VR_OK;
    const size_t bytes = t->brick_root.size() * sizeof(int32_t);
    if (bytes != (size_t)t->n_bricks * sizeof(int32_t)) return fail(VR_ERR_HIP, "the tree carries no brick-root table");
    hipError_t e = t->brick_root_dev.alloc(bytes);
    if (e == hipSuccess) e = hipMemcpy(t->brick_root_dev.get(), t->brick_root.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)t->brick_root_dev.reset();
        return fail(hip_code(e), "brick-root table of %zu bytes: %s", bytes, hipGetErrorString(e));
    }
    t->device_bytes += bytes;
    return VR_OK;
}

// Both value passes: the refusals that need no tree, the two tables (the call's one host-blocking step), the
// values pass and -- after an update of a tree with a lookup structure -- the refresh of its sigma fields
// behind it on the same stream.  No launch slot: the passes hold no per-call scratch.
int tree_data_pass(vr_tree_t t, void* data_dev, int dtype, void* stream, bool update) {
    if (!t || !data_dev) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (dtype != VR_DATA_F16 && dtype != VR_DATA_F32) return fail(VR_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
    DeviceGuard device_guard(t->device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> guard(t->launch_mutex);  // (also orders an update among the launches of other host threads)
    if (int rc = ensure_file_nodes(t)) return rc;
    if (int rc = ensure_brick_roots(t)) return rc;
    vr::UpdateArgs a;
    a.nodes = t->arrays[kNodes].get<uint32_t>();
    a.leaves = t->arrays[kLeaves].get<uint16_t>();
    a.file_node = t->file_node_dev.get<int32_t>();
    a.data = data_dev;
    a.capacity = t->desc.capacity;
    a.N3 = t->desc.N * t->desc.N * t->desc.N;
    a.data_dim = t->desc.data_dim;
    a.stride_h = t->leaf_stride_h;
    a.f32 = dtype == VR_DATA_F32;
    if (!update) {
        HIP_TRY(vr::launch_read_values(a, t->n_cus, hs));
        return VR_OK;
    }
    HIP_TRY(vr::launch_update_values(a, t->n_cus, hs));
    if (t->top_levels > 0)
        HIP_TRY(vr::launch_refresh_lookup(a.nodes, t->brick_root_dev.get<int32_t>(), t->n_bricks,
                                          t->arrays[kTop].get<uint2>(), t->arrays[kBricks].get<uint32_t>(),
                                          t->top_levels, t->brick_levels, hs));
    return VR_OK;
}

// vr_reserve_tiles / vr_reserve_rays: the ray buffers of the first n_slots slots hold `need` bytes.
int reserve_slots(VrTreeOpaque* t, int n_slots, size_t need) {
    DeviceGuard device_guard(t->device);
    std::lock_guard<std::mutex> guard(t->launch_mutex);
    for (int i = 0; i < n_slots; ++i) {
        LaunchSlot& ls = t->slots[i];
        if (ls.growing || ls.rays.bytes() >= need) continue;
        const hipError_t e = replace_ray_buffer(ls, need);
        if (e != hipSuccess) return fail(hip_code(e), "ray buffer of %zu bytes: %s", need, hipGetErrorString(e));
    }
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_tree_update_data(vr_tree_t t, const void* data_dev, int dtype, void* stream) {
    return tree_data_pass(t, const_cast<void*>(data_dev), dtype, stream, true);
}

int vr_tree_read_data(vr_tree_t t, void* data_dev, int dtype, void* stream) {
    return tree_data_pass(t, data_dev, dtype, stream, false);
}

int vr_render_backward(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt, int fp_mode,
                       const float* grad_accum, float* grad_data, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    if (int rc = validate_backward(t, n_frames, cams, opt, fp_mode, grad_accum, grad_data, k)) return rc;
    return render_backward(t, n_frames, cams, nullptr, opt, fp_mode, grad_accum, grad_data, k, stream);
}

int vr_render_backward_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                            const float* grad_accum, float* grad_data, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    vr::RayList rl;
    if (!grad_accum) return fail(VR_ERR_INVALID_ARGUMENT, "vr_render_backward_rays: NULL argument");
    if (int rc = validate_rays("vr_render_backward_rays", t, n, rays, opt, fp_mode, grad_data, k, rl)) return rc;
    if (int rc = check_backward_options("vr_render_backward_rays", opt)) return rc;
    return render_backward(t, k.n_frames, nullptr, &rl, opt, fp_mode, grad_accum, grad_data, k, stream);
}

int vr_accumulate_weights(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                          int fp_mode, const VrLeafWeights* out, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    if (int rc = validate_weights(t, n_frames, cams, opt, fp_mode, out, k)) return rc;
    return accumulate_weights(t, n_frames, cams, nullptr, opt, fp_mode, out, k, stream);
}

int vr_accumulate_weights_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                               const VrLeafWeights* out, void* stream) {
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    vr::RayList rl;
    if (int rc = validate_rays("vr_accumulate_weights_rays", t, n, rays, opt, fp_mode, out, k, rl)) return rc;
    if (!out->max_weight && !out->hits)
        return fail(VR_ERR_INVALID_ARGUMENT, "vr_accumulate_weights_rays: both outputs are NULL");
    return accumulate_weights(t, k.n_frames, nullptr, &rl, opt, fp_mode, out, k, stream);
}

int vr_render_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                   const VrRayOut* out, void* stream) {
    return render_rays(t, n, rays, opt, fp_mode, out, stream);
}

// the slots sized for the largest ray call of n rays: colour records plus the pixel words of a call without rgba
int vr_reserve_rays(vr_tree_t t, int64_t n, int n_slots) {
    if (!t) return fail(VR_ERR_INVALID_ARGUMENT, "vr_reserve_rays: tree is NULL");
    if (n_slots < 1 || n_slots > (int)kLaunchSlots)
        return fail(VR_ERR_INVALID_ARGUMENT, "vr_reserve_rays: n_slots=%d outside [1,%u]", n_slots, kLaunchSlots);
    vr::KParams geo;
    if (int rc = list_geometry("vr_reserve_rays", n, geo)) return rc;
    return reserve_slots(t, n_slots, ray_buffer_bytes(geo.total_rays, vr::kRayWords + ray_tail_words_of(t)) +
                                         list_pixel_bytes(geo.total_rays));
}

int vr_render_batch(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                    const VrFrame* frames, void* stream) {
    return render_launch(t, n_frames, cams, opt, frames, nullptr, 0, false, stream);
}

int vr_render_aov(vr_tree_t t, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                  const VrFrame* frames, const VrAov* aovs, int depth_units, void* stream) {
    return render_launch(t, n_frames, cams, opt, frames, aovs, depth_units, true, stream);
}

int vr_reserve_tiles(vr_tree_t t, int width, int height, int n_frames, int tile_w, int tile_h,
                     int world, int n_slots) {
    if (!t) return fail(VR_ERR_INVALID_ARGUMENT, "tree is NULL");
    if (n_frames < 1 || n_frames > VR_MAX_BATCH)
        return fail(VR_ERR_INVALID_ARGUMENT, "vr_reserve(%d x %d, %d frames) out of range", width,
                    height, n_frames);
    if (n_slots < 1 || n_slots > (int)kLaunchSlots)
        return fail(VR_ERR_INVALID_ARGUMENT, "n_slots=%d outside [1,%u]", n_slots, kLaunchSlots);
    // exactly the ray count vr_render_batch computes, for rank 0 (which holds the most tiles)
    vr::KParams geo;
    if (int rc = launch_geometry(width, height, tile_w, tile_h, 0, world, n_frames, geo)) return rc;
    return reserve_slots(t, n_slots, ray_buffer_bytes(geo.total_rays, vr::kRayWords + ray_tail_words_of(t)));
}

// two slots of whole frames: what a render loop on one stream (one slot) or on two alternating
// streams needs
int vr_reserve(vr_tree_t t, int width, int height, int n_frames) {
    return vr_reserve_tiles(t, width, height, n_frames, 0, 0, 1, 2);
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

int vr_render(vr_tree_t t, const VrCamera* cam, const VrRenderOptions* opt, const VrFrame* f,
              void* stream) {
    return vr_render_batch(t, 1, cam, opt, f, stream);
}

}  // extern "C"
