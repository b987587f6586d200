// vr_internal.h -- shared between the C-ABI host layer (vr_api.cpp, vr_upload.cpp, vr_launch.cpp, vr_slots.cpp, vr_values.cpp) and
// the gfx950 kernels (vr_render.hip, vr_weights.hip, vr_grad.hip, vr_fit.hip, vr_update.hip, vr_tree_kernels.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "volrend_hip.h"

namespace vr {

constexpr int kMaxBatch = 512;   // frames per launch (VR_MAX_BATCH)
constexpr int kTableChunk = 48;  // frames per prepare_launch_kernel call (4 KB kernarg limit)
constexpr int kTouchLeafShift = 7;  // log2 of the bytes one bit of the records' distinct-line bitmap stands for
                                    // (layout studies patch it: 6 = one bit per 64-byte SH9 record slot)

// ---------------------------------------------------------------------------
// The launch contract: what the host sizes and the kernels of a launch write and read.
// ---------------------------------------------------------------------------
// Basis flavour of a tree: the render_kernel<BASIS> instantiation that shades it, and with it what
// a ray carries.  The reference's switch only knows 25/16/9/4 (rt_core.cuh:132-160); every other
// basis size reads the first coefficient of each channel.
enum { BASIS_RGBA = -1, BASIS_1 = 1, BASIS_4 = 4, BASIS_9 = 9, BASIS_16 = 16, BASIS_25 = 25 };
__host__ __device__ inline int basis_flavour(int format, int basis_dim) {
    if (format == VR_FORMAT_RGBA || basis_dim < 0) return BASIS_RGBA;
    switch (basis_dim) {
        case 25: return BASIS_25;
        case 16: return BASIS_16;
        case 9: return BASIS_9;
        case 4: return BASIS_4;
        default: return BASIS_1;
    }
}
// basis_fn values the kernel flavour reads per ray (KParams.basis_words)
__host__ __device__ inline int basis_words(int flavour) { return flavour == BASIS_RGBA ? 0 : flavour; }
// SH trees with a basis size the kernel knows: the ray record carries the view direction (3 words)
// and the lane that takes the ray evaluates the basis; everything else carries the basis values
__host__ __device__ inline bool ray_vdir(int format, int flavour) {
    return format == VR_FORMAT_SH && basis_words(flavour) > 3;
}
__host__ __device__ inline int ray_tail_words(int format, int flavour) {
    return ray_vdir(format, flavour) ? 3 : basis_words(flavour);
}

// Ray record: the words of a ray in the ray buffer (written by raygen_kernel, read by render_kernel;
// blocked structure of arrays, vr_dev_rays.h ray_slot).  The pixel travels as the 64-bit address of
// its RGBA8, so that retiring a ray needs no frame-table lookup.
enum {
    kRayCen = 0,      // 3 words
    kRayDir = 3,      // 3 words
    kRayInvDir = 6,   // 3 words
    kRayT = 9,
    kRayTmax = 10,
    kRayDeltaScale = 11,
    kRayXy = 12,      // x | y << 16
    kRayPixelLo = 13,
    kRayPixelHi = 14,
    kRayFrame = 15,
    kRayWords = 16,   // the head; behind it ray_tail_words(): the view direction or basis_fn[0..nb)
    kRayTail = kRayWords,
};
// The ray queues own whole groups of 16 blocks of 64 rays ("Ray queues", vr_dev_rays.h): the
// number of such groups of a launch, and the ray slots its buffer holds.
__host__ __device__ inline uint32_t ray_groups16(uint32_t total_rays) { return ((total_rays >> 6) + 15u) >> 4; }
__host__ __device__ inline size_t ray_slots(uint32_t total_rays) { return (size_t)ray_groups16(total_rays) * 16 * 64; }

// Ray queues of a launch slot (device words, KParams.queue_head points at queue 0): queue x sits
// kQueueStride words behind queue x - 1 -- a 64-byte line each -- and uses two of them.
constexpr int kMaxQueues = 8;        // one per XCD (KParams.n_queues is 1 or kMaxQueues)
constexpr int kMaxQueuesShift = 3;
constexpr int kQueueStride = 16;
constexpr int kQueueHead = 0;        // rays handed out (render_kernel)
constexpr int kQueueCount = 1;       // rays stored (raygen_kernel)
constexpr int kSlotHeaderWords = 16; // the line in front of a slot's queues
constexpr int kSlotWords = 160;      // allocated per launch slot
static_assert(kMaxQueues == 1 << kMaxQueuesShift, "queues are picked with shifts and masks");
static_assert(kSlotWords >= kSlotHeaderWords + kMaxQueues * kQueueStride, "a slot holds its header and every queue");

// Scheduling tallies of the instrumented flavours: the words of KParams.sched_stats, in the order
// vr_sched_stats documents them.
enum {
    kStatMarchRounds = 0,
    kStatMarchLanes,
    kStatShadeRounds,
    kStatShadeLanes,
    kStatDistinctLeaves,
    kStatRetireRounds,
    kStatRetiredRays,
    kStatIterations,
    kSchedStats
};
static_assert(kSchedStats == 8, "vr_sched_stats(out[8]) is public ABI");

// Per-frame part of a launch: pose and buffers.  Lives in device memory (one
// small table per launch slot) because lanes of one wave may hold rays of
// different frames.
struct FrameDesc {
    float xf[12];  // column-major 4x3 c2w (CameraSpec.transform)
    uint8_t* rgba;
    float* accum;
    const float* depth;
    VrCounters* counters;  // optional
};

struct FrameTable {
    int32_t first;  // index of f[0] in the device table
    int32_t n;
    FrameDesc f[kTableChunk];
};

// Everything else the render kernel needs, passed BY VALUE as the kernel argument
// (the reference passes CameraSpec + TreeSpec + RenderOptions by value and the
// 12-float pose through a 48-byte H2D copy per frame, src/camera.cpp:67-75).
struct KParams {
    // ---- tree (TreeSpec, data_spec.hpp:23-50), device layout ----
    const uint32_t* nodes;    // one word per child slot (vr_dev_layout.h)
    const uint16_t* leaves;   // padded coefficient records
    const uint2* top;         // N == 2: 8^top_levels cells, see "Lookup structure" in vr_dev_layout.h
    const uint32_t* bricks;   // N == 2: n_bricks * 8^brick_levels entries
    const float* extra;
    float offset[3];
    float scale[3];
    int32_t N, N3;
    int64_t capacity;         // nodes
    int32_t data_dim;
    int32_t format;
    int32_t basis_dim;
    int32_t leaf_stride_h;    // fp16 elements between padded records
    int32_t max_depth;        // deepest leaf level (child words read - 1)
    int32_t top_levels;       // G0: the top grid has 2^G0 cells per axis (0 = no lookup structure)
    int32_t brick_levels;     // BL: a brick has 2^BL entries per axis (0 = no bricks)
    int32_t brick_blocked;    // 8^3 bricks stored in 4 x 4 x 2 line blocks (per tree, fixed at upload)
    float ndc_width, ndc_height, ndc_focal;
    // ---- camera intrinsics (CameraSpec, data_spec.hpp:11-22); poses are per frame ----
    int32_t width, height;
    float fx, fy;
    // ---- options (RenderOptions, render_options.hpp:11-53) ----
    float step_size, sigma_thresh, stop_thresh, background_brightness;
    float bbox[6];
    int32_t basis_min, basis_max;
    int32_t render_depth;
    int32_t enable_probe;
    int32_t probe_disp_size;
    const float* probe_coeffs;
    // rodrigues(opt.rot_dirs): the per-frame uniform part (angle, axis, cos, sin)
    // is evaluated once on the host (volrend.cu:59-64), the per-ray part on device
    int32_t rot_enabled;
    float rot_k[3];
    float rot_cos, rot_sin;
    // ---- frames / sharding ----
    const FrameDesc* frames;     // device table, n_frames entries
    int32_t n_frames;
    int64_t pitch;
    int32_t offscreen;
    int32_t layout;
    int32_t tile_w, tile_h;      // multiples of 8
    int32_t tiles_x, tiles_y;
    int32_t rank, world;
    int32_t n_local_tiles;
    int32_t wblocks_per_tile_x;  // tile_w / 8
    int32_t wblocks_per_tile;    // (tile_w/8)*(tile_h/8)
    int64_t n_wave_blocks;       // per frame: n_local_tiles * wblocks_per_tile
    uint32_t total_rays;         // n_frames * n_wave_blocks * 64
    // ---- persistent scheduling ----
    uint32_t* queue_head;        // kMaxQueues x (head, count), kQueueStride words apart, reset by prepare_launch_kernel
    int32_t n_queues;            // 1 or kMaxQueues (one ray-id range per XCD)
    int32_t chunk_max;           // largest ray-id chunk a wave takes at once (multiple of 64)
    const uint32_t* ray_buf;     // rays (written by raygen_kernel), blocked SoA; queue x's rays compacted to the
    uint32_t* ray_buf_rw;        // front of its region (vr_dev_rays.h "Ray queues")
    int32_t basis_words;         // basis_fn values a ray carries in registers (0 for RGBA)
    int32_t ray_tail_words;      // words of a ray record behind its kRayWords head: the 3 words of the
                                 // view direction (ray_vdir) or the basis_words basis values
    int32_t ray_vdir;            // SH trees: the record carries the view direction, the basis is
                                 // evaluated when a lane takes the ray
    int32_t refill_min;          // refill once this many lanes are idle
    int32_t march_max;           // march steps per lane between two shade checks
    int32_t drain_flush;         // drain phase: a ray blocked by its full colour queue gets a partial shade round
                                 // at once when at most this many lanes of the wave still march (0 = never)
    int32_t max_iter;            // guard: march rounds of a wave without a retired ray before it cuts its rays
    int32_t instrumented;        // any frame carries counters -> FULL flavour
    int32_t any_accum;           // some frame of the launch asks for its fp32 accumulators
    int32_t records_nt;          // record DMA loads carry the non-temporal hint (large lookup structures)
    int32_t frame_group;         // ray-id order: frames per group (block major, frame minor inside)
    int32_t super_block;         // ray-id order: blocks of a tile visited in SxS super-blocks
    uint32_t* status;            // device word: bit0 = iteration cap hit
    unsigned long long* sched_stats;  // kSchedStats scheduling tallies (instrumented flavours)
    // distinct-line meter (instrumented flavours, vr_touch_enable): one bit per 128-byte line of
    // leaves / nodes / top / bricks, set by every access; NULL when off
    uint32_t* touch[4];
};

// The tree takes the N == 2 lookup (top grid + bricks, built at upload when the tree qualifies) and not
// the literal descent: the launchers of vr_render.hip, vr_weights.hip and vr_query.hip pick their flavour by it.
inline bool uses_lookup(const KParams& p) { return p.N == 2 && p.top_levels > 0; }
// Which launches leave FAST for the FULL flavour (render_kernel MODE_FULL, raygen_kernel FULL): SG / ASG
// lobes, the access counters, and the depth visualisation.
inline bool needs_full(const KParams& p) {
    return p.format == VR_FORMAT_SG || p.format == VR_FORMAT_ASG || p.instrumented || p.render_depth;
}

// The grid of a persistent march kernel (render_kernel, weights_kernel, backward_kernel; one wave per workgroup) over
// total_blocks blocks of 64 rays: enough waves to fill the chip -- waves_per_cu of the flavour on each of
// n_cus -- but no more than about one per 128 pixels (one per 64 rays that enter the volume), so that
// small launches still rebalance through the ray queue.
inline unsigned persistent_grid(int64_t total_blocks, int n_cus, int waves_per_cu) {
    int64_t want = total_blocks / 2;
    if (want < 256) want = 256;
    if (want > total_blocks) want = total_blocks;
    const int64_t cap = (int64_t)n_cus * waves_per_cu;
    return (unsigned)(want < cap ? want : cap);
}

// ---------------------------------------------------------------------------
// AOV launches (vr_render_aov): extra per-pixel float planes next to the colour.  The AOV kernel
// flavours take KParams unchanged plus this second argument; the per-frame plane pointers sit in a
// table of their own in the launch slot (entry i = frame i), written by prepare_aov_kernel.
// ---------------------------------------------------------------------------
struct AovDesc {
    float* depth;          // NULL = not wanted
    float* transmittance;  // NULL = not wanted
};
struct AovParams {
    const AovDesc* planes;  // device table, n_frames entries
    int64_t pitch;          // bytes per row of both planes (always frame position, whatever the layout)
    int32_t depth_world;    // VR_DEPTH_WORLD: the depth plane holds D * delta_scale
};
struct AovTable {
    int32_t first;  // index of f[0] in the device table
    int32_t n;
    AovDesc f[kTableChunk];
};

// ---------------------------------------------------------------------------
// Block cull (colour and AOV frame launches of trees on the N == 2 lookup path): ray generation sends the 64 rays
// of an 8x8 pixel block that provably meets no density down the path of a ray that misses the volume -- a ray
// without a hit sample leaves trace_ray with the same values (out = 0, light = 1).
//   * Occupancy, built at upload and rebuilt behind every call that writes node words (vr_tree_kernels.hip): a
//     bitmap of 2^g cells per axis, g = min(kOccMaxLevels, depth of the deepest leaf), cell index x << 2g | y << g | z;
//     a cell is set when a leaf that overlaps it has sigma > 0.  From it the list of the set cells with an unset or
//     out-of-grid face neighbour: a line that meets a set cell runs through the closure of a listed one.
//     One buffer (VrTreeOpaque.occ): kOccHeaderWords words (word 0 = the length of the list), the bitmap, the list
//     (sized for every cell).
//   * Per launch, block_mask_kernel (vr_render.hip) splats every listed cell into every frame: one bit per 8x8
//     block of the FRAME (block (bx, by) = bit by * nbx + bx of the frame's words, whatever the tile shard), in the
//     launch slot behind the ray records, zeroed by prepare_launch_kernel.
//   * The FAST flavours of raygen_kernel, colour and AOV, read their block's bit (CullParams, their last
//     argument; mask = NULL: no cull) and count blocks seen / culled.
// KParams does not change: the march kernels keep their kernel descriptors (tools/kernel_digest.py).
// ---------------------------------------------------------------------------
constexpr int kOccMaxLevels = 7;
constexpr int kOccHeaderWords = 4;
constexpr int kCullStatLines = 16;        // the counters are spread over this many 64-byte lines (by workgroup)
constexpr int kCullStatStride = 8;        // u64 words per line: [0] = blocks seen, [1] = blocks culled
constexpr int kMaskMaxWords = 4096;       // words of one frame's mask that block_mask_kernel holds in LDS: larger frames
                                          // (> 131072 blocks) are not culled
__host__ __device__ inline size_t occ_bitmap_words(int g) { return g >= 2 ? ((size_t)1 << (3 * g)) / 32 : 1; }
__host__ __device__ inline size_t occ_words(int g) { return kOccHeaderWords + occ_bitmap_words(g) + ((size_t)1 << (3 * g)); }
struct CullParams {
    const uint32_t* mask;            // n_frames x words_per_frame; NULL = no cull
    uint32_t words_per_frame;        // (a multiple of 4)
    uint32_t nbx;                    // 8x8 blocks per row of the frame
    unsigned long long* stats;       // kCullStatLines x kCullStatStride
};
// ---------------------------------------------------------------------------
// Lead-in march (the FAST flavours of raygen_kernel, colour and AOV; tuning key head_march): the 64 rays of a block
// run the sample recurrence of the march round (march_sample, vr_dev_march.h) right behind setup_ray, side by side,
// while their samples are no hits.  A sample with sigma <= sigma_thresh changes nothing of a ray but t, so the
// record's kRayT simply holds a later t of the same sequence and render_kernel computes the bits it would have
// computed from the box entry; a ray that reaches tmax without a hit takes the path of a ray without a sample.
// A lane stops, t unchanged, at its first hit sample; the wave stops when fewer than min_lanes lanes march or
// after max_rounds rounds, and whoever still marches is handed over at the t it has.
// HeadParams is raygen_kernel's own (last) argument: KParams does not change.  max_rounds = 0: no lead-in march.
// ---------------------------------------------------------------------------
constexpr int kHeadStatWords = 3;         // words of a kCullStatStride line: rays entered, rays retired, samples marched
struct HeadParams {
    int32_t max_rounds;              // rounds a wave marches at most; 0 = off
    int32_t min_lanes;               // the wave hands over once fewer lanes march (1..64)
    unsigned long long* stats;       // kCullStatLines x kCullStatStride (vr_tree_head_stats)
};
// What block_mask_kernel reads beside KParams (frames, n_frames, offset, scale, width, height, fx, fy).
struct MaskParams {
    uint32_t* mask;
    uint32_t words_per_frame, nbx, nby;
    const uint32_t* occ;             // VrTreeOpaque.occ
    int32_t levels;                  // g
    int32_t groups_per_frame;        // workgroups that share the list for one frame
};
hipError_t launch_block_mask(const KParams& p, const MaskParams& m, hipStream_t stream);
// the occupancy bitmap and boundary list of a tree from its node words (vr_tree_kernels.hip)
hipError_t launch_build_occupancy(const uint32_t* nodes, int levels, uint32_t* occ, hipStream_t stream);

// ---------------------------------------------------------------------------
// Leaf-weight launches (vr_accumulate_weights): the march without records or shading.  The kernels of
// vr_weights.hip take KParams unchanged plus this second argument.  Their ray record is the march state
// alone -- the words kRayCen .. kRayDeltaScale of the colour record, nothing behind them.
// ---------------------------------------------------------------------------
constexpr int kWeightRayWords = kRayDeltaScale + 1;  // 12: cen, dir, invdir, t, tmax, delta_scale
static_assert(kWeightRayWords <= kRayWords, "a slot reserved for colour rays holds the weight rays of the same shape");
struct WeightParams {
    uint32_t* max_weight;       // [capacity * N3] bit patterns of non-negative floats, file order; NULL = not wanted
    uint32_t* hits;             // [capacity * N3], file order; NULL = not wanted
    const int32_t* file_node;   // device node -> the file's node (VrTreeOpaque.file_node)
};

// ---------------------------------------------------------------------------
// Ray lists (vr_render_rays, vr_accumulate_weights_rays, vr_render_backward_rays): the rays of a launch come
// from two caller arrays and not from locate() and a pose.  Only ray generation differs -- the kernels
// raygen_rays_kernel (vr_render.hip) and march_raygen_rays_kernel (vr_dev_march.h) take KParams unchanged plus this
// second argument and write the records of their frame siblings into the same queues; the march kernels are
// the frame launches'.  To them a list is ONE offscreen pseudo-frame kRayListWidth pixels wide whose pixel
// y * width + x is ray i: x = i & (kRayListWidth - 1), y = i >> kRayListShift (both below 2^15: i < 2^30),
// frames[0].rgba / .accum = the arrays of the call.  That is all the colour march reads of a frame's geometry
// (finish_ray: KParams.width, and the record's pixel address); the other two read none of it.
// ---------------------------------------------------------------------------
constexpr int kRayListShift = 15;
constexpr int kRayListWidth = 1 << kRayListShift;
struct RayList {
    const float* origins;  // device, [n][3], world space
    const float* dirs;     // device, [n][3], world space, any finite non-zero length
    int64_t n;
};
// whole blocks of 64 rays: what KParams.total_rays holds for a list (lanes with id >= n stay idle)
__host__ __device__ inline uint32_t ray_list_slots(int64_t n) { return (uint32_t)(((n + 63) >> 6) << 6); }

// vr_weights.hip: ray generation + the persistent march of a leaf-weight launch (the frame table and the
// queue reset are launch_prepare's).  check_first: the max reads the word before it issues the atomic.
// rays: the launch marches this list (its ray generation reads it) and not the pixels of the frame table.
hipError_t launch_weights(const KParams& p, const WeightParams& w, int fp_mode, int n_cus, int waves_override,
                          int gen_waves, bool check_first, hipStream_t stream, const RayList* rays = nullptr);

// ---------------------------------------------------------------------------
// Backward launches (vr_render_backward): the march of a leaf-weight launch that shades inline and scatters
// float sums.  The kernels of vr_grad.hip take KParams unchanged plus this second argument.  Their ray
// record is the weight record plus the view direction and the pixel's index into grad_accum: the length of
// a colour ray's head, so a slot reserved for colour rays of the same shape holds them.
// ---------------------------------------------------------------------------
enum {
    kGradRayVdir = kWeightRayWords,     // 3 words
    kGradRayPixel = kGradRayVdir + 3,   // (frame * height + y) * width + x
    kGradRayWords = kGradRayPixel + 1,
};
static_assert(kGradRayWords <= kRayWords, "a slot reserved for colour rays holds the backward rays of the same shape");
struct GradParams {
    const float* grad_accum;    // [n_frames][height][width][4]: dL / d out[0..3]
    float* grad_data;           // [capacity * N3 * data_dim], file order; added into
    const int32_t* file_node;   // device node -> the file's node (VrTreeOpaque.file_node)
    uint32_t* touched;          // marked calls: one bit per slot, file order, ORed into; NULL = the unmarked kernels
};

// vr_grad.hip: ray generation + the persistent two-phase march of a backward launch
// (rays: as launch_weights; GradParams.grad_accum is then [n][4], row i for ray i)
hipError_t launch_grad(const KParams& p, const GradParams& g, int fp_mode, int n_cus, int waves_override,
                       int gen_waves, hipStream_t stream, const RayList* rays = nullptr);

// ---------------------------------------------------------------------------
// Fused loss and backward of a ray list (vr_fit_rays, vr_fit.hip): the backward list's records and queues, and
// a march that forms out[], the L2 loss head and its gradient itself instead of reading grad_accum.
// ---------------------------------------------------------------------------
struct FitParams {
    const float* target;        // [n][3]: the colour ray i should have
    float* grad_data;           // as GradParams
    const int32_t* file_node;
    uint32_t* touched;          // ORed into; NULL = not wanted (a run-time test, one set of kernels)
    float* sq_err;              // [n]; NULL = not wanted
    float* accum;               // [n][4]: trace_ray's out[]; NULL = not wanted
    float bg, grad_scale;       // background_brightness; g_ch = grad_scale * r_ch
};
// vr_fit.hip: ray generation (which also writes the outputs of the rays that never enter the volume) + the
// persistent march.  `rays` is required: the call exists for lists only.
hipError_t launch_fit(const KParams& p, const FitParams& f, int fp_mode, int n_cus, int waves_override, int gen_waves,
                      hipStream_t stream, const RayList* rays);

// ---------------------------------------------------------------------------
// Value passes (vr_tree_update_data / vr_tree_read_data, vr_update.hip): the tree's values between the file's
// array and the device layout.  No launch slot, no KParams: the passes do not march.
// ---------------------------------------------------------------------------
struct UpdateArgs {
    uint32_t* nodes;            // device layout (vr_dev_layout.h); the read-back only reads both
    uint16_t* leaves;
    const int32_t* file_node;   // device node -> the file's node (VrTreeOpaque.file_node)
    void* data;                 // [capacity * N3 * data_dim], file order: read by the update, written by the read-back
    int64_t capacity;
    int32_t N3, data_dim;
    int32_t stride_h;           // fp16 elements between padded records
    int32_t f32;                // `data` is binary32 (VR_DATA_F32), else binary16
};
hipError_t launch_update_values(const UpdateArgs& a, int n_cus, hipStream_t stream);
hipError_t launch_read_values(const UpdateArgs& a, int n_cus, hipStream_t stream);
// the sigma fields of the leaf entries of top grid and bricks, from the node words (after an update)
hipError_t launch_refresh_lookup(const uint32_t* nodes, const int32_t* brick_root, int n_bricks, uint2* top,
                                 uint32_t* bricks, int top_levels, int brick_levels, hipStream_t stream);

// The sparse step (vr_tree_step, vr_update.hip): an optimiser step over the slots of a bitmap, written into master,
// moments and tree.  The scalars are what the host formed in binary64 and rounded once.
struct StepArgs {
    uint32_t* nodes;            // device layout (vr_dev_layout.h)
    uint16_t* leaves;
    const int32_t* node_of_file;  // the file's node -> device node (the inverse of VrTreeOpaque.file_node)
    float* master;              // [capacity * N3 * data_dim], file order
    float* grad;
    float* m;                   // Adam; NULL for SGD
    float* v;
    uint32_t* touched;          // n_words words: read, then cleared
    int64_t n_words;
    int64_t n_slots;            // capacity * N3: bits at or beyond it are ignored
    int32_t N3, data_dim;
    int32_t stride_h;           // fp16 elements between padded records
    int32_t adam;
    float lr, lr_sigma;         // SGD: lr_e; Adam: a_e = lr_e / (1 - beta1^step)
    float beta1, beta2, omb1, omb2, sbc2, eps;
};
hipError_t launch_step_values(const StepArgs& a, int n_cus, hipStream_t stream);

// vr_render.hip: the kernels of a launch
hipError_t launch_prepare_aov(const AovParams& a, const AovTable& tbl, hipStream_t stream);
// (cull: the block masks of the launch, CullParams{} = none; a ray list never has one)
// (head: the lead-in march of ray generation, HeadParams{} = none)
hipError_t launch_render_aov(const KParams& p, const AovParams& a, const CullParams& cull, const HeadParams& head,
                             int fp_mode, int n_cus, int waves_override, int gen_waves, hipStream_t stream);
// (mask: the block masks of the launch, which the kernel clears for its frames; NULL = none)
hipError_t launch_prepare(const KParams& p, const FrameTable& tbl, hipStream_t stream, uint32_t* mask = nullptr,
                          uint32_t words_per_frame = 0);
// (rays: as launch_weights; the frame table then holds the list's one pseudo-frame)
hipError_t launch_render(const KParams& p, const CullParams& cull, const HeadParams& head, int fp_mode, int n_cus,
                         int waves_override, int gen_waves, hipStream_t stream, const RayList* rays = nullptr);
hipError_t launch_probe(const KParams& p, const float probe[3], float* out_dev,
                        hipStream_t stream);

// vr_tree_kernels.hip: upload, tile gather, touch meter
// upload-time re-layout of the reference arrays into the device layout
int leaf_stride_halfs(int data_dim);
hipError_t launch_relayout(const int32_t* child, const uint16_t* data, const int32_t* perm,
                           uint32_t* nodes, uint16_t* leaves, int64_t n_slots, int N3,
                           int data_dim, int stride_h, hipStream_t stream);
// codebook decode of a quantised tree.npz into the reference's flat data layout (device)
hipError_t launch_decode_quant(const uint16_t* colors, const uint16_t* map, const uint16_t* sigma,
                               const uint16_t* retained, uint16_t* data, int64_t n_slots,
                               int n_quant, int n_ret, int data_dim, hipStream_t stream);
// N == 2 lookup structure (top grid + bricks), built from the re-laid-out node words
hipError_t launch_build_lookup(const uint32_t* nodes, const int32_t* brick_root, int n_bricks,
                               uint2* top, uint32_t* bricks, int top_levels, int brick_levels,
                               int brick_blocked, uint32_t* error_flag, hipStream_t stream);
// number of set bits of a bitmap of n_words 32-bit words, added to *out
hipError_t launch_popcount(const uint32_t* words, uint64_t n_words, unsigned long long* out,
                           hipStream_t stream);
// de-interleave of `world` gathered COMPACT tile buffers into frames
hipError_t launch_assemble(uint8_t* frame, int64_t pitch, const uint8_t* gathered, int width,
                           int height, int tile_w, int tile_h, int world, int n_frames,
                           int64_t out_stride, int64_t rank_stride, int64_t in_stride,
                           hipStream_t stream);

}  // namespace vr
