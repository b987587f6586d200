/*
 * volrend_hip.h -- C ABI of the MI355X (gfx950) PlenOctree ray-march library
 * (libvolrend_hip.so).  Plain C: opaque handles, PODs, int error codes.
 *
 * This is the drop-in boundary for ONE path of sxyu/volrend: everything that
 * the reference does on the CUDA device for `volrend_headless`.  Each entry
 * point names the reference interface it replaces (paths relative to the
 * reference tree):
 *
 *   vr_tree_upload / vr_tree_free   N3Tree::load_cuda / free_cuda      src/cuda/n3tree.cu:9-49
 *   vr_tree_upload_quantized,       the codebook decode loop of
 *   vr_decode_quantized             N3Tree::load_npz                   src/n3tree.cpp:279-340
 *   vr_tree_update_data,            no counterpart: the reference's device tree is written once,
 *   vr_tree_read_data               by load_cuda                       src/cuda/n3tree.cu:9-41
 *   VrTreeDesc                      internal::TreeSpec                 include/volrend/internal/data_spec.hpp:23-50
 *   VrCamera                        internal::CameraSpec + the 48-byte
 *                                   Camera::_update upload             data_spec.hpp:11-22, src/camera.cpp:67-75
 *   VrRenderOptions                 volrend::RenderOptions             include/volrend/render_options.hpp:11-53
 *   vr_render                       volrend::launch_renderer +
 *                                   device::render_kernel              include/volrend/cuda/renderer_kernel.hpp:9-12,
 *                                                                      src/cuda/volrend.cu:78-173,195-245
 *   vr_probe_coeffs                 retrieve_cursor_lumisphere_kernel  src/cuda/volrend.cu:175-191
 *   vr_query_points / vr_query_grid the same for many points per launch
 *                                   (query_single_from_root + one
 *                                   sample's colour)                   include/volrend/internal/n3tree_query.hpp:13-48,
 *                                                                      include/volrend/cuda/rt_core.cuh:125-163
 *   vr_read_back                    cudaMemcpy2DFromArrayAsync         main_headless.cpp:217-219
 *   vr_last_error / return codes    cuda_assert (print+exit) becomes
 *                                   an error code, the library never
 *                                   exits the process                  src/cuda/common.cu:8-21
 *
 * Asynchrony matches the reference: vr_render only enqueues on `stream`
 * (a hipStream_t passed as void*, NULL = the null stream) and returns.
 * The library owns device copies of trees; callers own output buffers,
 * streams and events.  A tree belongs to the device it was uploaded (or cloned)
 * to; calls that take a tree run on that device whatever the calling thread's
 * current device is and leave the thread's device unchanged, so one host thread
 * may drive the trees of several devices.  Streams and buffers passed with a
 * tree must belong to the tree's device.
 *
 * Launches in flight.  Unlike the reference's launch_renderer, a launch here
 * carries per-launch scratch in device memory (frame table, ray queue, ray
 * buffer, probe coefficients).  The library keeps 8 such launch slots per
 * tree; each slot remembers the last launch that used it with an event, and a
 * later launch that lands on the slot makes ITS stream wait for that event (a
 * device-side wait -- the host never blocks).  A launch takes the slot its own
 * stream used last, else one whose launch has finished, else queues up behind
 * the oldest.  So any number of launches on any number of streams and host
 * threads is safe; more than 8 un-finished launches on more than 8 streams of
 * one tree simply serialise.  The one host-blocking
 * step is the (re)allocation of a slot's ray buffer the first time a slot sees
 * a batch larger than any before -- call vr_reserve() once to take that out of
 * the render loop.
 */
#ifndef VOLREND_HIP_H_
#define VOLREND_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_ABI_VERSION 3

/* ---- error codes ------------------------------------------------------ */
enum {
    VR_OK = 0,
    VR_ERR_INVALID_ARGUMENT = 1,
    VR_ERR_HIP = 2,          /* a HIP runtime call failed; see vr_last_error() */
    VR_ERR_NO_DEVICE = 3,
    VR_ERR_BAD_TREE = 4,     /* child links out of range / cyclic / too deep */
    VR_ERR_UNSUPPORTED = 5,
    VR_ERR_OUT_OF_MEMORY = 6
};

/* DataFormat::format, include/volrend/data_format.hpp:9-15 */
enum { VR_FORMAT_RGBA = 0, VR_FORMAT_SH = 1, VR_FORMAT_SG = 2, VR_FORMAT_ASG = 3 };

/* Floating-point evaluation model of the kernel (DESIGN.md "FP contract").
 * STRICT evaluates the reference source with one rounding per operator and is
 * what the parity pin (host build of the reference) verifies bit for bit;
 * FMA fuses a*b+c the way an nvcc -fmad=true build plausibly does. */
enum { VR_FP_STRICT = 0, VR_FP_FMA = 1 };

#define VR_MAX_BASIS 25 /* VOLREND_GLOBAL_BASIS_MAX, render_options.hpp:6 */

typedef struct VrTreeOpaque* vr_tree_t;

/* Host (or device, see `memory`) view of a loaded tree.npz -- the arguments of
 * N3Tree::load_cuda.  child/data use the reference's flat layout:
 *   child[capacity * N^3]            int32, relative node offsets, 0 = leaf
 *   data [capacity * N^3 * data_dim] IEEE fp16, record = [R..,G..,B.., sigma] */
typedef struct VrTreeDesc {
    const int32_t* child;
    const uint16_t* data;
    const float* extra;      /* SG: basis_dim*4, ASG: basis_dim*11 floats; else NULL */
    uint64_t extra_count;    /* number of floats in `extra` */
    float offset[3];
    float scale[3];
    int32_t N;               /* branching factor per axis */
    int64_t capacity;        /* nodes */
    int32_t data_dim;
    int32_t format;          /* VR_FORMAT_* */
    int32_t basis_dim;       /* -1 for RGBA */
    float ndc_width;         /* <= 0 disables the LLFF NDC warp (data_spec.hpp:47) */
    float ndc_height;
    float ndc_focal;
    int32_t memory;          /* 0: pointers are host memory, 1: device memory */
} VrTreeDesc;

/* Median-cut compressed tree.npz (scripts/compress_octree.py:106-119): instead of
 * `data`, per basis function a 65536-entry RGB codebook + a 16-bit index per slot,
 * the densities, and optionally the first basis functions uncompressed.  Pointers
 * are host or device memory according to VrTreeDesc.memory.  n_slots = capacity*N^3. */
typedef struct VrQuantDesc {
    const uint16_t* quant_colors;  /* fp16 [n_quant, 65536, 3] */
    const uint16_t* quant_map;     /* u16  [n_quant, n_slots] */
    const uint16_t* sigma;         /* fp16 [n_slots] */
    const uint16_t* data_retained; /* fp16 [n_retained, n_slots, 3], or NULL */
    int32_t n_quant;
    int32_t n_retained;
} VrQuantDesc;

typedef struct VrTreeInfo {
    int64_t capacity;
    int32_t N, data_dim, format, basis_dim;
    int32_t max_depth;       /* deepest leaf: child words read = max_depth + 1 */
    int32_t device;
    uint64_t device_bytes;   /* total HBM held for this tree */
    uint64_t leaf_stride;    /* bytes between SH records in the device layout */
    int32_t query_mode;      /* VR_QUERY_LOOKUP / VR_QUERY_DESCENT: how a sample finds its leaf (below) */
    int32_t top_levels;      /* lookup structure built at upload: 2^top_levels cells per axis (0 = none) */
    int32_t brick_levels;    /* 2^brick_levels entries per axis of a brick (0 = no bricks) */
    int32_t brick_blocked;   /* bricks stored in 4 x 4 x 2 line blocks */
} VrTreeInfo;

/* How the kernels resolve query_single_from_root (n3tree_query.hpp:13-48) for a tree:
 *   VR_QUERY_LOOKUP  : N == 2, every leaf within 24 levels and fewer than 2^27 nodes -- integer
 *                      digits of the binary32 coordinate index a top grid + bricks (bit-identical);
 *   VR_QUERY_DESCENT : anything else the format allows (N != 2, deeper trees, larger arrays) -- the
 *                      literal float descent of the reference, level by level.
 * vr_query_mode_for is the rule vr_tree_upload applies (pure host arithmetic; max_depth as in
 * VrTreeInfo: the deepest leaf reads max_depth + 1 child words). */
#define VR_QUERY_LOOKUP 0
#define VR_QUERY_DESCENT 1
int vr_query_mode_for(int N, int max_depth, int64_t capacity);

/* CameraSpec: column-major 4x3 camera-to-world (right, up, back, centre) */
typedef struct VrCamera {
    float transform[12];
    int32_t width, height;
    float fx, fy;
} VrCamera;

/* Field for field volrend::RenderOptions (bools widened to int32). */
typedef struct VrRenderOptions {
    float step_size;
    float sigma_thresh;
    float stop_thresh;
    float background_brightness;
    float render_bbox[6];
    int32_t basis_minmax[2];
    float rot_dirs[3];
    int32_t show_grid;
    int32_t grid_max_depth;
    int32_t render_depth;
    int32_t enable_probe;
    float probe[3];
    int32_t probe_disp_size;
} VrRenderOptions;

/* Which pixels one call renders and where they land.
 * The frame is cut into tile_w x tile_h tiles (row-major tile order; both
 * multiples of 8, or 0/0 for "whole frame is one tile"); this call renders the
 * tiles t with t % world == rank -- the multi-GPU screen-tile shard.
 *   VR_LAYOUT_FRAME  : pixels go to their frame position, rgba + y*pitch + 4*x
 *   VR_LAYOUT_COMPACT: the rank's k-th tile (k = t / world) is stored densely at
 *                      rgba + k*tile_w*tile_h*4, row pitch tile_w*4 (the buffer
 *                      a gather collective sends); use vr_assemble_tiles on the
 *                      gathered buffer. */
enum { VR_LAYOUT_FRAME = 0, VR_LAYOUT_COMPACT = 1 };

typedef struct VrFrame {
    void* rgba;             /* device RGBA8 (byte order R,G,B,A; A = 255) */
    int64_t pitch;          /* bytes per row (FRAME layout); 0 = width*4 */
    const float* depth;     /* device R32F W*H mesh depth, or NULL */
    float* accum;           /* optional device float4 per frame pixel: trace_ray's
                               out[] before the background composite; or NULL */
    int32_t offscreen;      /* 1: composite over background_brightness (headless)
                               0: composite over the RGBA8 already in `rgba` */
    int32_t layout;         /* VR_LAYOUT_* */
    int32_t tile_w, tile_h;
    int32_t rank, world;    /* world <= 1: render everything */
    int32_t fp_mode;        /* VR_FP_* */
    int32_t reserved;
    uint64_t* counters;     /* optional device VrCounters (7 x u64, caller zeroes it):
                               switches to the instrumented kernel flavour; NULL in
                               production */
} VrFrame;

/* Access counters of one or more vr_render calls -- the algorithmic-bytes meter
 * (SURVEY.md 8(d)): what the REFERENCE algorithm reads for these rays, i.e.
 * per sample 4 bytes per child word from the root + 2 (sigma) + 2*(data_dim-1)
 * when sigma > sigma_thresh, plus 4 per pixel written. */
typedef struct VrCounters {
    uint64_t rays, rays_hit_box, samples, child_reads, hit_samples, alg_bytes, early_stops;
} VrCounters;

/* ---- library / device ------------------------------------------------- */
int vr_abi_version(void);
/* Thread-local description of the most recent failure on this thread. */
const char* vr_last_error(void);
int vr_device_count(int* count);
/* Select the device for subsequent calls on this thread (cudaSetDevice,
 * main_headless.cpp:108-111).  device < 0 keeps the current device. */
int vr_set_device(int device);
/* Fills name (<= name_len bytes) with the gcnArchName, e.g. "gfx950:..." */
int vr_device_name(int device, char* name, size_t name_len);

/* ---- tree ------------------------------------------------------------- */
void vr_default_tree_desc(VrTreeDesc* desc);
int vr_tree_upload(const VrTreeDesc* desc, vr_tree_t* out);
/* Same, for a quantised file: desc->data is ignored, the codebooks are decoded on the
 * device (only ~(2*n_quant + 6*n_retained + 2) instead of 2*data_dim bytes per slot
 * cross PCIe and no host loop runs).  The resulting tree is identical to uploading
 * the host-decoded data array. */
int vr_tree_upload_quantized(const VrTreeDesc* desc, const VrQuantDesc* quant, vr_tree_t* out);
/* The decode alone: writes the reference's flat data array [n_slots * data_dim] fp16 to
 * data_out (host or device memory per desc->memory; desc->child/data are not read). */
int vr_decode_quantized(const VrTreeDesc* desc, const VrQuantDesc* quant, uint16_t* data_out);
/* A second copy of an uploaded tree on another (or the same) device of this process: the device
 * layout is copied device to device (hipMemcpyPeer: xGMI between two GPUs of a node), so the
 * file crosses PCIe and is re-laid-out once however many GPUs render it.  The multi-GPU screen
 * tile shard (VrFrame.rank / world) renders from one such replica per GPU.  Synchronous. */
int vr_tree_clone(vr_tree_t src, int device, vr_tree_t* out);
int vr_tree_free(vr_tree_t tree);
int vr_tree_info(vr_tree_t tree, VrTreeInfo* info);
/* ---- The values of an uploaded tree, in place ---- */
/* The step that follows vr_render_backward in an optimiser loop, and its inverse.  The topology of the tree
 * does not change, so neither call repeats any host work of an upload: each is a streaming pass on the device.
 *   data_dev  device memory on the tree's device, capacity * N^3 * data_dim elements of `dtype`, indexed exactly
 *             as VrTreeDesc.data and grad_data are: the file's node numbering, record [R.., G.., B.., sigma].
 *   dtype     VR_DATA_F16: IEEE binary16 bits, as the file holds them.
 *             VR_DATA_F32: binary32.  The update rounds to binary16 to nearest even (as numpy.astype(float16):
 *             subnormal halves are produced, overflow goes to +-inf, the sign of zero is kept, a NaN becomes a
 *             NaN with an unspecified payload); the read-back is the exact widening.
 * vr_tree_update_data: once the call has passed on `stream`, every device array of the tree holds, bit for bit,
 * what vr_tree_upload of the same child array with this data array would have built -- the coefficient records
 * (padding zero; those of internal slots are stored, as upload stores them), the sigma of the leaf words and of
 * the leaf entries of the top grid and the bricks.  So every output of the library (colour, accum, AOV planes,
 * queries, probe, leaf weights, backward) is that of the fresh upload: in both query modes, both brick orders,
 * every format, for trees uploaded from a quantised file and for clones.  The leaf bit of a node word decides
 * what a slot is, as it did at upload: the sigma of an internal slot in data_dev is ignored.  `extra` (SG / ASG
 * lobes) is not part of `data` and is not touched.
 * vr_tree_read_data: writes the tree's current values to data_dev -- the bits of what was uploaded or last
 * written, with the sigma of internal slots as +0.  update(read(tree)) changes nothing.  A slot of a node the root does
 * not reach whose link leaves [1, capacity) is a leaf to the upload (no topology check covers such a link, and it is
 * never followed): its node word carries the leaf bit, so it reads back its sigma, not +0, and an update writes it.
 * Contract: both calls only enqueue on `stream`, run on the tree's device whatever the calling thread's current
 * device is, and take no launch slot.  The first of them on a tree puts two tables on the device under the
 * tree's mutex -- the 4-bytes-per-node file-order table of vr_accumulate_weights (whose n_frames == 0 call is
 * the warm-up here too) and 4 bytes per brick of the lookup structure -- the call's one host-blocking step; from
 * then on they count in VrTreeInfo.device_bytes.  A tree that is never updated or read holds neither.
 * vr_tree_update_data WRITES the tree and is ordered like any write to a buffer that kernels read: launches,
 * queries and clones enqueued LATER ON THE SAME STREAM see the new values; work on other streams must be
 * ordered by the caller with events, both ways: nothing on the device may read the tree (no launch, query,
 * read-back or clone) while the update runs.  vr_tree_read_data only reads the tree and may run beside launches.
 * VR_ERR_INVALID_ARGUMENT, before the tree handle is followed or any device call: NULL tree, NULL data_dev,
 * unknown dtype.  Nothing is VR_ERR_UNSUPPORTED. */
enum { VR_DATA_F16 = 0, VR_DATA_F32 = 1 };
int vr_tree_update_data(vr_tree_t tree, const void* data_dev, int dtype, void* stream);
int vr_tree_read_data(vr_tree_t tree, void* data_dev, int dtype, void* stream);
/* ---- A sparse optimiser step, written into the tree in place ---- */
/* The step of an optimiser loop over ONLY the leaf slots a batch of rays hit: vr_render_rays -> (the caller's
 * loss) -> vr_render_backward_rays_touched -> vr_tree_step.  Its cost follows the rays and the slots they hit,
 * not the size of the tree: no dense gradient is zeroed, no dense optimiser pass runs, and the tree is not
 * rewritten whole (vr_tree_update_data).  All five arrays are device memory on the tree's device, indexed as
 * VrTreeDesc.data and grad_data are; `touched` is the bitmap the marked backward calls OR into: one bit per child
 * slot s = file node * N^3 + child slot, bit s & 31 of word s >> 5, ceil(capacity * N^3 / 32) words.
 * For every set bit s < capacity * N^3 and every e in [0, data_dim), with i = s * data_dim + e, g = grad[i],
 * lr_e = (e == data_dim - 1) ? lr_sigma : lr, in binary32 with one rounding per operator (no contraction, IEEE
 * divide and square root):
 *   VR_STEP_SGD   w = master[i] - lr_e * g
 *   VR_STEP_ADAM  m' = beta1 * m[i] + omb1 * g,  v' = beta2 * v[i] + (omb2 * g) * g,
 *                 w = master[i] - a_e * (m' / (sqrtf(v') / sbc2 + eps))
 *                 omb1 = 1 - beta1, omb2 = 1 - beta2, sbc2 = sqrt(1 - beta2^step), a_e = lr_e / (1 - beta1^step):
 *                 four scalars the host forms in binary64 and rounds once to binary32.  The moments of slots
 *                 whose bit is clear do not move (sparse-Adam semantics).
 * then master[i] = w (m[i] = m', v[i] = v'), grad[i] = +0, and the tree takes w rounded to binary16 to nearest
 * even -- the rounding of vr_tree_update_data(VR_DATA_F32): coefficient entries into the padded record of the
 * slot (the padding stays zero), the sigma entry into the slot's node word when the slot is a leaf; the sigma of
 * an internal slot is ignored and its coefficients are stored, as the dense update does.  Bits at or beyond
 * capacity * N^3 in the last word are ignored.  On completion every word of `touched` is 0.  Elements of slots
 * whose bit is clear are neither read nor written, in any of the five arrays or in the tree.
 * For a tree with a lookup structure the sigma fields of top grid and bricks are refreshed WHOLE behind the
 * values kernel (as vr_tree_update_data does), so every device array of the tree is, bit for bit, what
 * vr_tree_upload of the same child array would build from a data array that is binary16(master) in touched
 * slots and the old values elsewhere: in both query modes, both brick orders, for quantised uploads and clones.
 * Contract: that of vr_tree_update_data -- enqueue only on `stream`, on the tree's device whatever the thread's
 * device, no launch slot; it WRITES the tree: later work on the same stream sees it, other streams are the
 * caller's to order.  The first call puts three tables on the device under the tree's mutex (then counted in
 * VrTreeInfo.device_bytes): a 4-bytes-per-node table file node -> device node, the file-order table and the
 * brick-root table.
 * VR_ERR_INVALID_ARGUMENT, before the tree handle is followed or any device call: NULL tree / s / master / grad /
 * touched, unknown kind, VR_STEP_ADAM with NULL m or v, with step < 1 or with a beta outside [0, 1), non-finite
 * lr, lr_sigma or eps.  Nothing is VR_ERR_UNSUPPORTED. */
enum { VR_STEP_SGD = 0, VR_STEP_ADAM = 1 };
typedef struct VrStep {
    float*    master;    /* [capacity*N^3*data_dim] float32, file order: the values the tree's binary16 are rounded from */
    float*    grad;      /* same shape: read, then set to +0 in every touched slot */
    uint32_t* touched;   /* the bitmap of the marked backward calls: read, then cleared */
    float*    m;         /* Adam moments, same shape; NULL for SGD */
    float*    v;
    int32_t   kind;      /* VR_STEP_SGD / VR_STEP_ADAM */
    float     lr, lr_sigma;  /* coefficient entries / the sigma entry of a record */
    float     beta1, beta2, eps;
    int32_t   step;      /* Adam: 1, 2, ... for the bias correction */
} VrStep;
int vr_tree_step(vr_tree_t tree, const VrStep* s, void* stream);
/* ---- Refining a tree: subdividing selected leaves, on the device ---- */
/* The calls above work on the topology fixed at upload.  These two restate a tree with SELECTED LEAVES SUBDIVIDED,
 * as arrays IN THE FILE'S LAYOUT (VrTreeDesc.child / .data) in device memory, together with any companion arrays
 * that are indexed the same way (a float32 master, Adam moments, leaf weights); vr_tree_upload with memory = 1
 * then takes the new arrays without a host round trip.  The restatement is APPEND-ONLY in the file's node
 * numbering: every old node and slot keeps its index and the new nodes follow behind the old ones, so everything
 * indexed by slot stays valid and only grows at the end.  They take no tree handle and work on the calling thread's
 * current device, as vr_decode_quantized does.  With N3 = N^3 and n_slots = capacity * N3, in plain integers:
 *   - slot s < n_slots is REFINED iff bit s & 31 of sel[s >> 5] is set and child[s] == 0.  Bits of internal slots
 *     and bits at or beyond n_slots are ignored.  n_new = the number of refined slots.
 *   - the r-th refined slot in ascending s (r = 0, 1, ...) becomes node capacity + r: unique and bit-reproducible
 *     (the order in which svox's refine appends).
 *   - child_out[s] = capacity + r - s / N3 for a refined slot, child[s] for every other old slot, and 0 for all N3
 *     slots of every new node (they are leaves).  src_slot[r] = s.
 *   - per companion array: the first n_slots * dim elements of dst are the bits of src (a refined slot keeps its
 *     values: it is an internal slot from now on); for each of the N3 slots of node capacity + r the dim elements
 *     are those of src slot s (VR_REFINE_COPY) or zero bits (VR_REFINE_ZERO).  Elements move as bits.
 * vr_refine_plan forms the effective mask words (sel AND leaf, tail bits cleared), their popcounts and an exclusive
 * scan of those in the workspace, copies the total to *n_new and waits for `stream`: the call's one host-blocking
 * step.  capacity + n_new > INT32_MAX is VR_ERR_UNSUPPORTED (child words are int32 node offsets), and so is a
 * src_slot array for more than 2^31 slots.
 * vr_refine_apply only enqueues on `stream`.  It takes the workspace of a plan of the same child and sel,
 * unchanged, and that plan's n_new, and writes child_out, src_slot (when not NULL) and every dst; the old part of
 * each array is one device-to-device copy.  Every store is bounded by capacity + n_new and a rank >= n_new writes
 * nothing, so a caller's mistake (another n_new, a workspace that was written in between) gives wrong contents and
 * never an out-of-range store.  n_new == 0 is legal: the outputs are copies of the inputs.
 * The workspace is the caller's: at least vr_refine_workspace(N, capacity) bytes (-1 for arguments the calls
 * refuse; no device call), 256-byte aligned, free again once apply's work on `stream` is done.  Of VrRefine, plan
 * reads child, sel, workspace, workspace_bytes, capacity and N; apply reads everything.
 * VR_ERR_INVALID_ARGUMENT, before any device call: NULL r, child, sel, workspace or n_new (plan) or child_out
 * (apply); child_out == child; N outside what vr_tree_upload accepts (2..16); capacity < 1 or beyond INT32_MAX; n_new < 0;
 * workspace_bytes too small or a misaligned workspace; n_arrays outside 0..VR_REFINE_MAX_ARRAYS, or arrays NULL
 * when n_arrays > 0; per array elem_bytes not 2 or 4, dim < 1, an unknown fill, NULL src or dst, dst == src.
 * Merging leaves back into their parent slot and compacting the node array is vr_collapse_plan / vr_collapse_apply
 * below (that changes the numbering, and the calls hand out the maps).  Not offered: refining the device layout of
 * an uploaded tree without a re-upload, quantised inputs, `extra` (it is not indexed by slot), and choosing what to
 * refine: max_weight, hits and grad_data are already in the file's indexing, so a threshold is the caller's one
 * line. */
enum { VR_REFINE_COPY = 0, VR_REFINE_ZERO = 1 };
#define VR_REFINE_MAX_ARRAYS 8
typedef struct VrRefineArray {   /* one companion array, indexed as VrTreeDesc.data: slot * dim + e */
    const void* src;             /* device, capacity * N^3 * dim elements */
    void*       dst;             /* device, (capacity + n_new) * N^3 * dim elements, != src */
    int32_t elem_bytes;          /* 2 or 4: elements move as bits, no conversion */
    int32_t dim;                 /* elements per slot, >= 1 */
    int32_t fill;                /* the slots of NEW nodes: VR_REFINE_COPY = the refined slot's elements,
                                    VR_REFINE_ZERO = zero bits */
    int32_t reserved;
} VrRefineArray;
typedef struct VrRefine {
    const int32_t*  child;       /* device [capacity * N^3], the file's relative offsets, 0 = leaf */
    const uint32_t* sel;         /* device, the `touched` bitmap format: bit s & 31 of word s >> 5 */
    int32_t* child_out;          /* device [(capacity + n_new) * N^3], != child            (apply) */
    int32_t* src_slot;           /* device [n_new]: the slot new node capacity + r came from; or NULL (apply) */
    const VrRefineArray* arrays; /* HOST array of n_arrays entries                          (apply) */
    void*   workspace;
    int64_t workspace_bytes;
    int64_t capacity;
    int64_t n_new;               /* what plan returned                                      (apply) */
    int32_t N;
    int32_t n_arrays;            /* 0..VR_REFINE_MAX_ARRAYS */
} VrRefine;
int64_t vr_refine_workspace(int N, int64_t capacity);
int vr_refine_plan(const VrRefine* r, int64_t* n_new, void* stream);
int vr_refine_apply(const VrRefine* r, void* stream);
/* ---- Collapsing nodes and compacting a tree, on the device ---- */
/* The opposite direction (svox's `merge`): selected nodes all of whose slots are leaves are merged into the parent
 * slot that links to them, and the node array is COMPACTED, so the numbering changes; the calls hand out the maps
 * between the two numberings and carry companion arrays through them.  Conventions as vr_refine_*: no tree handle,
 * arrays in the FILE's layout in device memory, the calling thread's current device, the caller's workspace, plan
 * has the one host-blocking step and apply only enqueues.  With N3 = N^3, in plain integers:
 * Which nodes collapse
 *   - node m is a FRONTIER node iff child[m*N3 + j] == 0 for all j.
 *   - node m is COLLAPSED iff 1 <= m < capacity, bit m & 31 of sel[m >> 5] is set and m is a frontier node.  The
 *     selection is per NODE (a threshold of max_weight.view(capacity, N3).amax(1) is the caller's one line).
 *   - bit 0 is ignored (the root has no slot to collapse into), and so are bits at or beyond capacity and bits of
 *     nodes that are not frontier nodes.
 * One level per call: a collapsed node has no links, so nothing below it exists; collapsing deeper is done by
 * repeating the call, as svox's merge does.
 * New numbering
 *   - the kept nodes (not collapsed) keep their relative order: the p-th kept node in ascending old index is new
 *     node p.  src_node[p] is the old index of new node p, node_map[src_node[p]] = p, node_map[m] = -1 for a
 *     collapsed m.  n_keep = capacity - n_collapsed >= 1.  Unique and bit-reproducible.
 *   - nodes that no slot links to are kept like any other: the calls do not walk the tree.
 * New child array, for a kept node n with p = node_map[n] and slot j
 *   - child[n*N3 + j] == 0: child_out[p*N3 + j] = 0.
 *   - otherwise let m = n + child[n*N3 + j].  If m is collapsed: child_out[p*N3 + j] = 0; this slot is the MERGED
 *     SLOT of m, and into_slot[m] = p*N3 + j.  Otherwise child_out[p*N3 + j] = node_map[m] - p.
 *   - into_slot is -1 for kept nodes and for collapsed nodes nobody links to.
 * Companion arrays, each indexed slot * dim + e as VrRefineArray is
 *   - dst[(p*N3 + j)*dim + e] = src[(src_node[p]*N3 + j)*dim + e], moved as bits; a merged slot follows the array's
 *     rule instead:
 *       VR_COLLAPSE_KEEP  the bits the slot already held (after a refine with COPY: the pre-refine values);
 *       VR_COLLAPSE_ZERO  zero bits;
 *       VR_COLLAPSE_MEAN  per element e, the mean over the N3 slots of m: the elements of slots k = 0..N3-1 of m
 *                         are read as floats (elem_bytes 2: binary16, 4: binary32) and summed in binary32 in
 *                         ASCENDING k, one rounding per add, starting from the k = 0 element; the sum is divided by
 *                         (float)N3, correctly rounded; for binary16 the result is rounded to nearest even, by the
 *                         rule of vr_tree_update_data(VR_DATA_F32): subnormals are produced, overflow goes to
 *                         +-inf.  A NaN result has an unspecified payload.
 * Contract: child is a tree vr_tree_upload accepts.  A link outside [1, capacity) is never followed (no
 * out-of-range load); it leaves that one child_out word unspecified and nothing else.  A node linked from two slots
 * collapses into both; into_slot names one of them, and ZERO / MEAN reach that one.
 * vr_collapse_plan forms the collapse words (sel AND frontier, bit 0 and the tail bits cleared), the popcounts of
 * the keep words and an exclusive scan of those in the workspace, copies the total to *n_keep and waits for
 * `stream`.  vr_collapse_apply takes the unchanged workspace of a plan of the same child and sel, and that plan's
 * n_keep, and writes child_out, the maps that are not NULL and every dst.  Every store is bounded by the n_keep it
 * was TOLD: a new index >= n_keep writes nothing, so a caller's mistake gives wrong contents, never an out-of-range
 * store.  n_collapsed == 0 is legal: the outputs are copies of the inputs.
 * The workspace: at least vr_collapse_workspace(N, capacity) bytes (-1 for arguments the calls refuse; no device
 * call), 256-byte aligned, free again once apply's work on `stream` is done.  Of VrCollapse, plan reads child, sel,
 * workspace, workspace_bytes, capacity and N; apply reads everything.
 * VR_ERR_INVALID_ARGUMENT, before any device call: NULL c, child, sel, workspace or n_keep (plan) or child_out
 * (apply); child_out == child; N outside 2..16; capacity outside [1, INT32_MAX]; n_keep outside [1, capacity]
 * (apply); workspace_bytes too small or a misaligned workspace; n_arrays outside 0..VR_COLLAPSE_MAX_ARRAYS, or
 * arrays NULL when n_arrays > 0; per array elem_bytes not 2 or 4, dim < 1, an unknown rule, NULL src or dst,
 * dst == src.  VR_ERR_UNSUPPORTED: into_slot, or an array with ZERO / MEAN (they go by an into_slot of the
 * workspace), for more than 2^31 slots.
 * Not offered: removing whole subtrees in one call, dropping unreachable nodes, a max or sum rule (weights, hits),
 * quantised inputs, changing the device layout of an uploaded tree without the re-upload, `extra`. */
enum { VR_COLLAPSE_KEEP = 0, VR_COLLAPSE_ZERO = 1, VR_COLLAPSE_MEAN = 2 };
#define VR_COLLAPSE_MAX_ARRAYS 8
typedef struct VrCollapseArray {  /* one companion array, indexed as VrTreeDesc.data: slot * dim + e */
    const void* src;              /* device, capacity * N^3 * dim elements */
    void*       dst;              /* device, n_keep * N^3 * dim elements, != src */
    int32_t elem_bytes;           /* 2 or 4: elements move as bits; MEAN reads binary16 / binary32 */
    int32_t dim;                  /* elements per slot, >= 1 */
    int32_t rule;                 /* what a merged slot gets: VR_COLLAPSE_KEEP / _ZERO / _MEAN */
    int32_t reserved;
} VrCollapseArray;
typedef struct VrCollapse {
    const int32_t*  child;        /* device [capacity * N^3], the file's relative offsets, 0 = leaf */
    const uint32_t* sel;          /* device bitmap over NODES: bit m & 31 of word m >> 5, ceil(capacity / 32) words */
    int32_t* child_out;           /* device [n_keep * N^3], != child                                     (apply) */
    int32_t* node_map;            /* device [capacity]: new index of an old node, -1 if collapsed; or NULL (apply) */
    int32_t* src_node;            /* device [n_keep]: old index of a new node; or NULL                    (apply) */
    int32_t* into_slot;           /* device [capacity]: the merged slot of a collapsed node, else -1; or NULL (apply) */
    const VrCollapseArray* arrays;  /* HOST array of n_arrays entries                                     (apply) */
    void*   workspace;
    int64_t workspace_bytes;
    int64_t capacity;
    int64_t n_keep;               /* what plan returned                                                  (apply) */
    int32_t N;
    int32_t n_arrays;             /* 0..VR_COLLAPSE_MAX_ARRAYS */
} VrCollapse;
int64_t vr_collapse_workspace(int N, int64_t capacity);
int vr_collapse_plan(const VrCollapse* c, int64_t* n_keep, void* stream);
int vr_collapse_apply(const VrCollapse* c, void* stream);
/* ---- Slot geometry: where a slot is, on the device ---- */
/* Everything above addresses the tree by SLOT (s = node * N3 + (ix*N + iy)*N + iz, N3 = N^3); these two calls say
 * where a slot is: the slot that links to its node, its depth, its cell in space, and points inside that cell.
 * Conventions as vr_refine_*: no tree handle, arrays in the FILE's layout in device memory, the calling thread's
 * current device.  Both calls ONLY ENQUEUE on `stream`: no host-blocking step, no caller's workspace, no launch slot.
 * Every output is optional (NULL = not wanted); at least one must be wanted.  In plain integers:
 * vr_tree_geometry, per NODE m of child [capacity * N3]
 *   - parent_slot[m] = the slot s with child[s] != 0 and s / N3 + child[s] == m; -1 for node 0 and for a node no slot
 *     links to.  A link outside [1, capacity) is never followed: there is no out-of-range store.  Contract: child is a
 *     tree vr_tree_upload accepts; a node linked from two slots gets one of them.  vr_tree_upload also accepts files
 *     in which a node the root does not reach links into the tree: for those files the row of the doubly linked node,
 *     and the depth and origin of everything below it, are unspecified.
 *   - node_depth[m] = the number of links from node 0 (the root is 0): what VrQueryOut.depth reports for a leaf slot
 *     of m.  -1 for a node whose parent chain does not reach node 0 within VR_GEOM_MAX_DEPTH links.  The walk up the
 *     chain is a counted loop of at most VR_GEOM_MAX_DEPTH steps, whatever the input holds (cycles among unreachable
 *     nodes included).
 *   - node_origin[m][a] = the integer coordinate, on axis a, of the node's lower corner in the N^depth grid of its
 *     level: the sum over the links of the chain of digit_a(link slot) * N^(links below it), accumulated in uint64
 *     and stored modulo 2^32; exact for N^depth <= 2^32 (N = 2: 32 levels).  digit_x(j) = j / N^2, digit_y(j) =
 *     j / N % N, digit_z(j) = j % N for j = s % N3.  Unspecified where node_depth is -1.
 *   The parent pass is a fill with -1 and one scatter over the slots; when parent_slot is NULL and a walked output is
 *   wanted it goes into capacity * 4 bytes taken from and returned to the device's stream-ordered pool on `stream`:
 *   no wait, but the pool hands memory back at a synchronise, so such a call can pay an allocation on the host
 *   (measured: 0.34 ms against 0.08 ms for call + wait on 2 M nodes).  A caller in a loop passes parent_slot.
 * vr_slot_points, per entry i of slots [n] and q = 0..k-1, with s = slots[i] = m * N3 + j and L = node_depth[m] + 1
 *   - I = node_origin[m][a] * N + digit_a(j) in uint64; D = N^L as L binary64 multiplications of 1.0 by N in turn
 *     (exact below 2^53, always for a power of two); u = 0.5 (VR_POINTS_CENTER) or (double)(h >> 8) * 2^-24
 *     (VR_POINTS_JITTER) with h = mix(mix(mix(seed + 0x9e3779b9u * (uint32_t)s) + q) + a) in uint32 arithmetic, mix
 *     being x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   - points[i][q][a] = ((double)I + u) / D: one binary64 add, one correctly rounded binary64 divide, converted to
 *     binary32 TOWARD ZERO.  TREE coordinates.  depth[i] = node_depth[m]; side[i] = 1.0 / D in binary64, converted to
 *     binary32 to nearest.
 *   - a slot index outside [0, capacity * N3), or one whose node has a depth outside 0..VR_GEOM_MAX_DEPTH, gives
 *     NaN points, depth -1 and side NaN, and reads nothing out of range.  An internal slot is defined like a leaf:
 *     the points lie in that slot's cell.
 *   The results are a pure function of (s, q, a, seed): independent of n, of the order of slots and of how a list is
 *   split into calls.  n == 0 enqueues nothing.
 *   Guarantee: for N a power of two and N^L <= 2^24 the lower bound I / D of the cell is a binary32 number, and the
 *   truncation puts every point into [I / D, (I + 1) / D) of its own cell; vr_query_points(VR_SPACE_TREE) at the point
 *   then finds slot s when s is a leaf, as long as the cell lies below the query's clamp at 1 - 1e-6f.  Beyond these
 *   limits (other N, deeper cells) a point may round onto a cell boundary; its value is still the one defined above,
 *   bit for bit.
 * VR_ERR_INVALID_ARGUMENT, before any device call: NULL g / p; NULL child; NULL node_depth, node_origin, or slots
 * with n > 0; every output NULL; N outside 2..16; capacity outside [1, INT32_MAX]; n outside [0, 2^31); k outside
 * 1..VR_POINTS_MAX_K; an unknown mode.  VR_ERR_UNSUPPORTED: more than 2^31 slots (slot indices are int32).
 * Not offered: world-space points (the caller applies (p - offset) / scale), dense per-slot outputs, neighbour
 * finding, a `slot` output of the point queries, trees deeper than VR_GEOM_MAX_DEPTH levels. */
#define VR_GEOM_MAX_DEPTH 64
#define VR_POINTS_MAX_K 64
enum { VR_POINTS_CENTER = 0, VR_POINTS_JITTER = 1 };
typedef struct VrGeometry {
    const int32_t* child;        /* device [capacity * N^3], the file's relative offsets, 0 = leaf */
    int32_t*  parent_slot;       /* device [capacity], or NULL */
    int32_t*  node_depth;        /* device [capacity], or NULL */
    uint32_t* node_origin;       /* device [capacity][3], or NULL */
    int64_t capacity;
    int32_t N;
    int32_t reserved;
} VrGeometry;
typedef struct VrSlotPoints {
    const int32_t*  node_depth;  /* device [capacity]: of vr_tree_geometry of the same tree */
    const uint32_t* node_origin; /* device [capacity][3] */
    const int32_t*  slots;       /* device [n]: the caller's list of slot indices */
    float*   points;             /* device [n][k][3] TREE coordinates, or NULL */
    int32_t* depth;              /* device [n], or NULL */
    float*   side;               /* device [n]: the edge of the slot's cell, or NULL */
    int64_t capacity;
    int64_t n;                   /* 0 <= n < 2^31 */
    int32_t N;
    int32_t k;                   /* points per slot, 1..VR_POINTS_MAX_K */
    int32_t mode;                /* VR_POINTS_CENTER / VR_POINTS_JITTER */
    uint32_t seed;               /* JITTER */
} VrSlotPoints;
int vr_tree_geometry(const VrGeometry* g, void* stream);
int vr_slot_points(const VrSlotPoints* p, void* stream);

/* ---- quantise a tree on the device ------------------------------------- *
 * vr_quantize is the encoder of the format vr_tree_upload_quantized / vr_decode_quantized read: the median cut of
 * scripts/compress_octree.py (unweighted), per basis function, on a data array in the FILE's layout in device memory.
 * The four outputs are exactly the arrays of VrQuantDesc with n_quant = n_basis - n_retained.  Conventions as
 * vr_decode_quantized and vr_refine_*: no tree handle, the calling thread's current device, the workspace is the
 * caller's (vr_quantize_workspace bytes, 256-byte aligned, free again once the work on `stream` is done).  The call
 * ONLY ENQUEUES on `stream`: it has no host-blocking step.
 * Basis function j, channel c of slot s is data[s * data_dim + j + c * n_basis]; sigma_s is data[s * data_dim +
 * data_dim - 1].  The definition, which the result meets bit for bit:
 *   - Kept slots.  Slot s is kept iff (float)sigma_s > sigma_thresh.  A NaN sigma is not kept.  Internal slots take
 *     part, as they do in the reference script.
 *   - sigma[s] = the bits of sigma_s if kept, else +0.
 *   - data_retained[r][s][c] = the bits of basis r, channel c if kept, else +0.
 *   - quant_map[j][s] = 0 for a slot that is not kept.
 *   - Median cut, per quantised basis function b = n_retained + j, independently.  The points are p_s = (R, G, B) of
 *     b over the kept slots.  All points start in box 0.  For every level l = 0 .. bits-1 and every non-empty box
 *     k < 2^l with n points: per axis, the range is max - min of the box's values, computed in binary64 (exact for
 *     binary16 inputs); the split axis is the one with the largest range, ties to the lowest axis; the points are
 *     ordered by their value on that axis in the total order of the binary16 bit patterns (sign-magnitude, so -0
 *     comes before +0), ties by ASCENDING SLOT INDEX; the first ceil(n/2) points go to box 2k, the rest to box 2k+1.
 *     A box is always split, even when all its points are equal.  After the last level quant_map[j][s] = the box of
 *     p_s, which is below 2^bits.
 *   - Codebook.  Per box k with cnt > 0 points and per channel: S = the exact sum of the values as int64 multiples of
 *     2^-24 (every finite binary16 is one; integer adds make the sum independent of order); quant_colors[j][k][c] =
 *     ((double)S / (double)cnt) * 2^-24, converted to binary32 to nearest even, then to binary16 to nearest even.
 *     Rows of empty boxes, and rows at or beyond 2^bits, are zero bits.
 *   - Every element of all four outputs is written by the call.
 * Consequences: an entry lies within [min, max] of its box on every axis; if at most 2^bits slots are kept, every box
 * holds at most one point and decoding returns each kept value exactly, as a value (a -0 comes back as +0).
 * Contract on values: the coefficients of kept slots are finite and the sum of |x| within any box is below 2^39
 * (true for 2^23 points of any finite binary16 values).  Outside it the codebook and map of that basis function are
 * unspecified; every code is still below 2^bits and nothing is stored out of range.
 * The result is unique and bit-reproducible: it does not depend on the stream, the workspace contents, or repeats.
 * VR_ERR_INVALID_ARGUMENT, before any device call: NULL q, data, quant_colors, quant_map, sigma or workspace;
 * data_retained present while n_retained == 0, or absent while it is not; n_slots outside [1, 2^31); data_dim < 4 or
 * (data_dim - 1) % 3 != 0; n_retained outside 0 .. n_basis - 1; bits outside 1..16; a NaN sigma_thresh; a workspace
 * smaller than vr_quantize_workspace says or not 256-byte aligned; an output equal to `data`.  Nothing is
 * VR_ERR_UNSUPPORTED.
 * Not offered: the script's --weighted cut; deflate (the caller's file writer compresses); `extra`; quantising an
 * uploaded tree's device layout in place (the caller does vr_tree_read_data -> vr_quantize). */
typedef struct VrQuantize {
    const uint16_t* data;          /* device [n_slots][data_dim] binary16, file layout (VrTreeDesc.data) */
    uint16_t* quant_colors;        /* device [n_quant][65536][3] binary16 */
    uint16_t* quant_map;           /* device [n_quant][n_slots] */
    uint16_t* sigma;               /* device [n_slots] binary16 */
    uint16_t* data_retained;       /* device [n_retained][n_slots][3]; NULL iff n_retained == 0 */
    void*   workspace; int64_t workspace_bytes;
    int64_t n_slots;               /* capacity * N^3, 1 .. 2^31-1 */
    int32_t data_dim;              /* (data_dim - 1) % 3 == 0; n_basis = (data_dim - 1) / 3 */
    int32_t n_retained;            /* 0 .. n_basis - 1; n_quant = n_basis - n_retained >= 1 */
    int32_t bits;                  /* 1..16 */
    float   sigma_thresh;          /* not NaN */
} VrQuantize;
int64_t vr_quantize_workspace(int64_t n_slots, int data_dim);   /* -1 for refused arguments; no device call */
int vr_quantize(const VrQuantize* q, void* stream);

/* ---- render ----------------------------------------------------------- */
void vr_default_options(VrRenderOptions* opt);
void vr_default_frame(VrFrame* frame);
/* Number of bytes of the COMPACT buffer of one rank for the given sharding. */
int64_t vr_compact_bytes(int width, int height, int tile_w, int tile_h, int world);
int vr_render(vr_tree_t tree, const VrCamera* cam, const VrRenderOptions* opt,
              const VrFrame* frame, void* stream);
/* Several poses in ONE launch (the volrend_headless pose loop, main_headless.cpp:207-225,
 * known up front): cams[i] -> frames[i].  All entries must share image size,
 * intrinsics, layout, sharding and fp_mode; only the pose and the buffers differ.
 * A single 800x800 frame cannot fill 256 CUs; a batch can.  1 <= n <= VR_MAX_BATCH. */
#define VR_MAX_BATCH 512
int vr_render_batch(vr_tree_t tree, int n_frames, const VrCamera* cams,
                    const VrRenderOptions* opt, const VrFrame* frames, void* stream);
/* ---- AOV planes: depth and transmittance from the colour launch ---------- */
/* vr_render_batch that ALSO writes, per pixel, two float planes ("AOV" = an extra per-pixel plane
 * of a render launch) from the same march -- no second pass.  With t, weight, light_intensity and
 * delta_scale exactly as trace_ray (rt_core.cuh:66-196) forms them, in the launch's FP model:
 *   D = sum over the samples with sigma > sigma_thresh, in order, of weight * t: D = weight * t + D
 *       (STRICT: two roundings; FMA: one fused operation) -- what the reference's depth mode holds in
 *       out[0] BEFORE its min(. * 0.3f, 1) and before the early-stop rescale.  t is the distance
 *       along the normalised tree-space direction.
 *   T = light_intensity when the ray leaves the loop, through t >= tmax or through stop_thresh (it
 *       is NOT forced to 0 or 1 at an early stop).
 * A ray that takes no sample -- it misses render_bbox, a mesh depth in VrFrame.depth (offscreen = 0)
 * cuts it off in front of the box, or the tree has N <= 0 -- gives D = 0, T = 1.
 *   depth plane          VR_DEPTH_TREE : D
 *                        VR_DEPTH_WORLD: D * delta_scale (one more rounding): the length the
 *                        attenuation uses (rt_core.cuh:119).  For an NDC tree (ndc_width > 0) that is a
 *                        length in NDC space, not in the scene's world space.
 *   transmittance plane  T
 * The expected depth of what the ray hit is depth / (1 - T) (undefined where T == 1); the library
 * does not form it.
 * Colour, accum and everything else are exactly what vr_render_batch produces for the same
 * arguments, and the contract is the same: enqueue only, launch slots, one frame size / intrinsics /
 * layout / sharding / fp_mode (and one AOV pitch) per launch, <= VR_MAX_BATCH frames, vr_reserve*
 * covers it (the launch's table of plane pointers lives in the launch slot from upload on).
 * The planes are ALWAYS addressed in frame position, plane + y * pitch + 4 * x, whatever
 * VrFrame.layout says; a tile-sharded rank writes only the pixels of its own tiles.
 * VR_ERR_INVALID_ARGUMENT: everything vr_render_batch refuses, NULL aovs, an entry with both planes
 * NULL, unknown depth_units, a pitch below width * 4 or not a multiple of 4 (or differing within the
 * batch).  VR_ERR_UNSUPPORTED: opt->render_depth (the depth visualisation already is that launch),
 * opt->enable_probe (pixels under the probe disc are not traced), a frame with counters (the
 * instrumented flavour).  All checked before any device work. */
enum { VR_DEPTH_TREE = 0, VR_DEPTH_WORLD = 1 };
typedef struct VrAov {        /* device pointers of ONE frame; NULL = not wanted, at least one non-NULL */
    float*  depth;            /* [height] rows of width floats */
    float*  transmittance;
    int64_t pitch;            /* bytes per row of both planes; 0 = width*4 */
} VrAov;
int vr_render_aov(vr_tree_t tree, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                  const VrFrame* frames, const VrAov* aovs, int depth_units, void* stream);
/* ---- Leaf weights: per leaf, the largest ray weight over a set of views ---- */
/* What PlenOctree extraction and pruning threshold on (svox: accumulate_weights): for every pixel of
 * every camera the ray of trace_ray (rt_core.cuh:66-196) is marched exactly as vr_render_batch marches
 * it, in FP model fp_mode, as an offscreen frame (no mesh depth: tmax comes from render_bbox alone), and
 * for each sample with sigma > sigma_thresh, in the leaf slot s the point query returns:
 *   hits[s] += 1 (modulo 2^32);
 *   if weight > 0: max_weight[s] = max(max_weight[s], weight)   (weight <= 0 or NaN only counts in hits)
 * with weight = light_intensity * (1.f - att) as the reference forms it -- the sample that then trips
 * stop_thresh included.  No colour is formed: the tree's format and basis do not matter.
 * The call accumulates INTO the buffers; the caller zeroes them once.  A maximum and a count are
 * order-independent: any split of a pose set into calls, batches, streams or devices (followed by an
 * element-wise max / sum) gives the same bits.  On entry max_weight must hold non-negative, non-NaN
 * floats (on that domain the float maximum is the unsigned maximum of the bit patterns).
 * Of opt only step_size, sigma_thresh, stop_thresh and render_bbox are read.
 * Contract: that of vr_render_batch -- enqueue only, one image size and one set of intrinsics per call,
 * <= VR_MAX_BATCH frames, a launch slot (the ray record is shorter than a colour ray's: vr_reserve of the
 * same shape covers it), step_size <= 0 / NaN refused, the sample guard reports through vr_tree_status.
 * The first call of a tree uploads a 4-bytes-per-node table (device node -> file node) under the tree's
 * mutex -- the call's one host-blocking step; from then on it counts in VrTreeInfo.device_bytes.
 * n_frames == 0 does just that and launches nothing (the warm-up call).  Apart from that table the call
 * only reads the tree: any number of calls may run beside each other, render launches and queries.
 * VR_ERR_INVALID_ARGUMENT, before the tree handle is followed or any device call: NULL tree / cams (when
 * n_frames > 0) / opt / out, both outputs NULL, unknown fp_mode, n_frames < 0 or > VR_MAX_BATCH, cameras
 * that differ in size or intrinsics. */
typedef struct VrLeafWeights {  /* device pointers; NULL = not wanted; at least one non-NULL.
                                   Both [capacity * N^3], indexed as VrTreeDesc.child / data are:
                                   node * N^3 + child slot IN THE FILE'S node numbering */
    float*    max_weight;
    uint32_t* hits;
} VrLeafWeights;
int vr_accumulate_weights(vr_tree_t tree, int n_frames, const VrCamera* cams,
                          const VrRenderOptions* opt, int fp_mode, const VrLeafWeights* out, void* stream);
/* ---- Backward: gradients of a rendered batch with respect to the tree's values ---- */
/* The step that follows pruning when a PlenOctree is optimised against its training images.
 *   grad_accum  device, float32 [n_frames][height][width][4], tightly packed: dL / d out[0..3], out[] being
 *               trace_ray's output (rt_core.cuh:66-196) for the pixel -- the four numbers VrFrame.accum
 *               receives.  (The background composite is the caller's to differentiate.)
 *   grad_data   device, float32 [capacity * N^3 * data_dim], indexed exactly as VrTreeDesc.data is (the file's
 *               node numbering, record order [R.., G.., B.., sigma]).  The call ADDS into it; the caller
 *               zeroes it once.  Elements that no hit sample of the call touches are not written at all.
 * The frame is marched as vr_accumulate_weights marches it (offscreen, no mesh depth, tmax from render_bbox
 * alone, FP model fp_mode).  The march geometry -- which samples exist, their leaves, delta_t, delta_scale,
 * whether and where the ray stops -- has the colour kernels' bits and is a CONSTANT of the differentiation;
 * only sigma and the record entries are variables.  Per ray, hit samples i = 1..K (sigma_i > sigma_thresh):
 *   d_i = delta_t_i * delta_scale, a_i = exp(-d_i sigma_i), T_1 = 1, T_{i+1} = T_i a_i, w_i = T_i - T_{i+1}
 *   c_{i,ch} = 1 / (1 + exp(-u)), u = sum_b B_b k_{i,ch,b} over the basis functions the renderer uses (all
 *   of them for basis_dim 4 / 9 / 16 / 25, else b = 0 only); RGBA trees: c_{i,ch} = the record entry
 *   s = 1 / (1 - T_{K+1}) when stop_thresh ended the ray at sample K, else 1
 *   G_i = sum_ch g_ch c_{i,ch}, R_i = sum_{j>i} w_j G_j, C^ = sum_j w_j G_j, g = the pixel's grad_accum
 *   SH coefficient (ch, b) of slot s_i += g_ch s w_i c_{i,ch} (1 - c_{i,ch}) B_b       (used b only)
 *   RGBA entry ch of slot s_i          += g_ch s w_i
 *   sigma of slot s_i                  += d_i (T_{i+1} G_i - R_i + g_3 T_{K+1})               (not stopped)
 *                                      += d_i (s (T_{i+1} G_i - R_i) - s^2 T_{K+1} C^)        (stopped)
 * summed over all rays of all frames, in binary32 (the running sum behind R_i in binary64) with float
 * atomic adds: THE ORDER OF THE SUM IS NOT DEFINED, so two runs may differ in the last bits.  This is the
 * library's one output that is not bit-reproducible; every other output stays bit-exact.
 * Non-finite values.  A ray is outside the formulas if a slot one of its hit samples falls into holds a
 * non-finite value (any entry of the record, sigma included), if its grad_accum pixel holds one, or if its
 * binary32 forward output -- out[0..3] or the transmittance T_{K+1} as the colour kernels compute them -- is
 * itself non-finite, even when every record it meets is finite (a_i = inf from a large negative sigma under a
 * negative sigma_thresh; s = 1 / 0 when stop_thresh >= 1 meets an a_K that rounds to 1).  Such a ray leaves
 * unspecified values in every element of the slots its hit samples fall into, and only there: the call
 * returns, nothing faults, every other ray's contribution to every other slot is what the formulas say, and
 * elements no ray touches keep their bits.  Which samples are hits depends on sigma_i > sigma_thresh alone (a
 * NaN sigma is never a hit, +inf is one), for these rays as for all others.
 * Contract: that of vr_accumulate_weights -- enqueue only, on a launch slot (vr_reserve of the same shape
 * covers it), <= VR_MAX_BATCH frames of one size and one set of intrinsics, step_size <= 0 / NaN refused,
 * the sample guard reports through vr_tree_status, n_frames == 0 uploads the file-order table and launches
 * nothing; the tree is only read.
 * VR_ERR_INVALID_ARGUMENT, before the tree handle is followed or any device call: NULL tree / opt /
 * grad_accum / grad_data / cams (when n_frames > 0), unknown fp_mode, n_frames outside 0..VR_MAX_BATCH,
 * cameras that differ in size or intrinsics, a bad step_size.  VR_ERR_UNSUPPORTED: render_depth,
 * enable_probe, non-zero rot_dirs (before the handle is followed); SG / ASG trees and a basis_minmax that
 * leaves out a basis function of the tree (right after, before any device work). */
int vr_render_backward(vr_tree_t tree, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                       int fp_mode, const float* grad_accum, float* grad_data, void* stream);
/* ---- Ray lists: render, weigh and differentiate caller-supplied rays ---- */
/* The three calls above take their rays from the pixels of VrCameras; an optimiser draws its rays at random
 * from many images of different size and intrinsics.  These take n rays as two device arrays.  Ray i is THE RAY
 * OF A PIXEL, ENTERED BEHIND screen2worlddir's MATRIX PRODUCT (volrend.cu:29-31):
 *   dir = dirs[i], normalised as screen2worlddir normalises (in FP model fp_mode); cen = origins[i]
 * and from there on exactly what a pixel's ray goes through, as an OFFSCREEN frame without mesh depth
 * (t_max = 1e9): maybe_world2ndc, offset + scale * cen, the rot_dirs rotation of the view direction,
 * _get_delta_scale, the ray/box test, trace_ray.  Consequences:
 *   - a list built from a camera -- origin transform[9..11], direction the product of the 3x3 part of
 *     transform with the pixel's (x, y, -1) as screen2worlddir forms it -- gives bit for bit what the frame
 *     call gives for that pixel: RGBA8, accumulators, leaf weights;
 *   - results do not depend on the order of the rays, on n, or on how a list is split into calls (the backward
 *     sum is the exception, exactly as for frames);
 *   - 64 consecutive rays share a wave.  The library does not reorder them: coherence is the caller's business
 *     (vr_order_rays, below, computes an order the caller can apply);
 *   - finite origins and finite non-zero directions are the contract; anything else is outside it, as a
 *     non-finite pose is for frames.
 * Each call keeps the contract of its frame sibling: enqueue only, on a launch slot, on the tree's device
 * whatever the thread's current device is, step_size <= 0 / NaN refused, the sample guard reports through
 * vr_tree_status, the tree is only read.  0 <= n < 2^30; n == 0 is VR_OK and launches nothing (for the weights
 * and backward calls it still uploads the file-order table, as their n_frames == 0 does).
 * VR_ERR_INVALID_ARGUMENT, before the tree handle is followed or any device call: NULL tree / rays / origins /
 * dirs / opt / out, every output NULL, unknown fp_mode, n outside the range, a bad step_size.
 * Not offered for lists: a per-ray t_max / mesh depth, AOV planes, tile sharding, any reordering of the rays
 * by these calls (vr_order_rays is a call of its own), gradients with respect to the rays. */
typedef struct VrRays {       /* device, [n][3] float32 each, tightly packed, world space */
    const float* origins;
    const float* dirs;        /* any finite non-zero length */
} VrRays;
typedef struct VrRayOut {     /* device; NULL = not wanted, at least one non-NULL */
    void*  rgba;              /* [n] RGBA8: the offscreen composite over background_brightness */
    float* accum;             /* [n][4] float32: trace_ray's out[] before the composite (what VrFrame.accum receives) */
} VrRayOut;
/* Colour.  All of opt is honoured as an offscreen frame honours it (basis_minmax, rot_dirs, render_bbox, SG / ASG
 * trees); VR_ERR_UNSUPPORTED: render_depth (not what a ray list is for) and enable_probe (the probe disc is a
 * set of pixel positions).  A call without rgba uses 4 bytes per ray of its launch slot as scratch. */
int vr_render_rays(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                   const VrRayOut* out, void* stream);
/* vr_accumulate_weights over the rays of a list: its outputs, the file's node numbering, the accumulate-into
 * rule and its refusals. */
int vr_accumulate_weights_rays(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt,
                               int fp_mode, const VrLeafWeights* out, void* stream);
/* vr_render_backward over the rays of a list: grad_accum is [n][4], row i for ray i; grad_data, the formulas
 * and the refusals (render_depth, enable_probe, rot_dirs, a narrowed basis_minmax, SG / ASG trees) are its. */
int vr_render_backward_rays(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt,
                            int fp_mode, const float* grad_accum, float* grad_data, void* stream);
/* vr_render_backward / vr_render_backward_rays that ALSO mark the slots they add into.  `touched`: device, one
 * bit per child slot in the indexing of VrTreeDesc.child, grad_data / data_dim and VrLeafWeights (s = file node *
 * N^3 + child slot; bit s & 31 of word s >> 5; ceil(capacity * N^3 / 32) words).  The call ORs into it; the
 * caller zeroes it once.  A bit is set exactly for every slot that receives a hit sample's contributions, i.e.
 * whose run of grad_data the call adds into: a set that does not depend on any order, so the bitmap IS
 * bit-reproducible although grad_data is not.  Everything else -- contract, launch slot, refusals, the n == 0
 * behaviour, the formulas -- is that of the unmarked sibling; NULL touched is VR_ERR_INVALID_ARGUMENT, refused
 * before the tree handle is followed.  What vr_tree_step consumes. */
int vr_render_backward_touched(vr_tree_t tree, int n_frames, const VrCamera* cams, const VrRenderOptions* opt,
                               int fp_mode, const float* grad_accum, float* grad_data, uint32_t* touched,
                               void* stream);
int vr_render_backward_rays_touched(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt,
                                    int fp_mode, const float* grad_accum, float* grad_data, uint32_t* touched,
                                    void* stream);
/* ---- Fused L2 loss and backward of a ray list ---- */
/* What every optimiser loop over ray batches writes as vr_render_rays(accum) -> composite, residual against a
 * target colour, grad_accum -> vr_render_backward_rays_touched, in ONE launch: the march forms out[], the loss
 * head and its gradient itself, and no [n][4] array travels between kernels.  For ray i:
 *   out[0..3]  trace_ray's output for the ray exactly as vr_render_rays forms it in FP model fp_mode (what
 *              VrRayOut.accum receives), the early-stop rescale and out[3] = 1 on a stop included.
 *   The loss head is not part of trace_ray: uncontracted binary32 in BOTH FP models, one rounding per operator,
 *   in this order, with bg = opt->background_brightness:
 *     na = 1.f - out[3]
 *     pred_ch = out[ch] + bg * na
 *     r_ch = pred_ch - target[i][ch]
 *     sq_err[i] = (r_0 * r_0 + r_1 * r_1) + r_2 * r_2
 *     g_ch = grad_scale * r_ch
 *     g_3 = -(bg * ((g_0 + g_1) + g_2))
 *   i.e. the gradient of L = grad_scale / 2 * sum_i sum_ch r_{i,ch}^2 with respect to out[]; grad_scale =
 *   2 / (3 n) makes L the mean squared error.
 *   grad_data  receives what vr_render_backward_rays adds for grad_accum[i] = (g_0, g_1, g_2, g_3): the same
 *              formulas, the same "the order of the sum is not defined", the same rule for non-finite values
 *              (a non-finite target or grad_scale * r puts the ray outside the formulas as a non-finite
 *              grad_accum pixel does) and the same untouched-elements rule.
 *   touched    receives what vr_render_backward_rays_touched ORs in: a slot is marked when a hit sample falls
 *              into it, whatever the value added -- a batch whose residual is zero still marks.
 * accum and sq_err are bit-reproducible; grad_data is reproducible up to its summation order, as for the
 * backward calls.  A ray that never enters the volume has out[] = 0: it gets its sq_err / accum and adds nothing.
 * Contract: that of vr_render_backward_rays -- enqueue only, on a launch slot (vr_reserve_rays of the same n
 * covers it), on the tree's device, 0 <= n < 2^30, n == 0 uploads the file-order table and launches nothing, the
 * sample guard reports through vr_tree_status, the tree is only read.
 * VR_ERR_INVALID_ARGUMENT, before the tree handle is followed: NULL tree / rays / origins / dirs / opt / fit /
 * target / grad_data, unknown fp_mode, n outside the range, a bad step_size, a non-finite grad_scale.
 * VR_ERR_UNSUPPORTED: what vr_render_backward_rays refuses -- render_depth, enable_probe, non-zero rot_dirs, a
 * narrowed basis_minmax, SG / ASG trees -- with vr_fit_rays named in the message.
 * Not offered: frame (camera) siblings, losses other than L2, per-ray weights, a background other than
 * background_brightness, gradients with respect to the rays. */
typedef struct VrFit {       /* device pointers on the tree's device */
    const float* target;     /* [n][3] float32: the colour ray i should have */
    float        grad_scale; /* finite; L = grad_scale / 2 * sum_i sum_ch r_{i,ch}^2.  2 / (3 n) for the mean */
    float*       grad_data;  /* as vr_render_backward_rays: ADDED into, required */
    uint32_t*    touched;    /* as vr_render_backward_rays_touched: ORed into; NULL = not wanted */
    float*       sq_err;     /* [n]: r_0^2 + r_1^2 + r_2^2 of ray i; NULL = not wanted */
    float*       accum;      /* [n][4]: what vr_render_rays gives in VrRayOut.accum; NULL = not wanted */
} VrFit;
int vr_fit_rays(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt,
                int fp_mode, const VrFit* fit, void* stream);
/* ---- Ordering a ray list for coherence ---- */
/* The march calls above take the rays in the caller's order, 64 consecutive rays to a wave, and rays drawn at
 * random are the order the march likes least.  vr_order_rays computes, on the device, the order that puts rays
 * with neighbouring segments through the volume next to each other, and gathers the list (and one payload array,
 * e.g. VrFit.target) into that order; the caller then hands the gathered arrays to any ray-list call and takes
 * per-ray outputs back through `order`.  It rests on "results do not depend on the order of the rays".
 *   Setup: ray i is set up exactly as the ray-list launches set it up in FP model fp_mode (direction normalised,
 *     maybe_world2ndc, offset + scale * cen, _get_delta_scale, the ray/box test against opt->render_bbox; step_size
 *     is not read and rot_dirs does not matter), which leaves cen, dir, tmin, tmax in tree coordinates.
 *   Key: a ray that does not enter the volume (the ray/box test fails, or tree N <= 0) has key 0xFFFFFFFF.
 *     Otherwise e[c] = madd(tmin, dir[c], cen[c]) and x[c] = madd(tmax, dir[c], cen[c]) -- the march's position
 *     formula, madd that of the FP model -- and each of the six coordinates v = (e0, e1, e2, x0, x1, x2)[c] is
 *     quantised to `bits` bits: q = (uint32_t)min(max(v * 2^bits, 0.f), 2^bits - 1), truncating, NaN -> 0.  Bit
 *     6 * b + c of the key is bit b of coordinate c: a 6-D Morton code in 6 * bits bits, the higher bits zero.
 *   Result: order = the STABLE sort of 0 .. n-1 by key (ties in increasing index): unique and bit-reproducible.
 *     keys[j] = key(order[j]); rays that miss come last.  The gathered arrays are bit copies: origins_out[j] =
 *     origins[order[j]], dirs_out[j] = dirs[order[j]] (as given, NOT normalised), payload_out[j] =
 *     payload[order[j]].  Nothing but the named outputs and the workspace is written; the inputs are not modified.
 *   bits == 0 selects the library's default, 2 (12 key bits): the value with the cheapest order + march on the
 *     bench tree.  Whether ordering pays at all depends on the tree and on the batch -- it did NOT for 65,536 rays
 *     drawn from 64 frames (README.md "Ordering ray batches" has what was measured).
 * Contract: that of the point queries -- enqueue only, on the tree's device, the tree is only read, no launch
 * slot, no library-owned scratch, no mutex: safe beside any launch.  The caller owns `workspace`: at least
 * vr_order_rays_workspace(n) bytes, 256-byte aligned, usable again once the call's work on `stream` is done.
 * 0 <= n < 2^30; n == 0 is VR_OK and enqueues nothing.
 * VR_ERR_INVALID_ARGUMENT, before the tree handle is followed or any device call: NULL tree / rays / origins /
 * dirs / opt / out / order, unknown fp_mode, n outside the range, bits outside 0..5, payload without payload_out
 * or the reverse, payload_dim outside 1..8 with a payload (or non-zero without), a NULL, misaligned or too small
 * workspace when n > 0, an output equal to its input (origins_out == origins, dirs_out == dirs, payload_out ==
 * payload). */
typedef struct VrRayOrder {         /* device pointers on the tree's device */
    int          bits;              /* 1..5 key bits per coordinate; 0 = the library's default (2) */
    uint32_t*    order;             /* [n], required: order[j] = index of the ray at sorted position j */
    uint32_t*    keys;              /* [n] sorted keys; NULL = not wanted */
    float*       origins_out;       /* [n][3]: origins[order[j]]; NULL = not wanted */
    float*       dirs_out;          /* [n][3]: dirs[order[j]] (as given, NOT normalised); NULL = not wanted */
    const float* payload;           /* [n][payload_dim], e.g. VrFit.target; NULL = none */
    float*       payload_out;       /* [n][payload_dim]: payload[order[j]]; required iff payload */
    int          payload_dim;       /* 1..8 when payload is given, else 0 */
} VrRayOrder;
/* Bytes of workspace a vr_order_rays of n rays needs: 0 for n <= 0, non-decreasing in n; makes no device call.
 * (A byte count as int64_t, like vr_compact_bytes.) */
int64_t vr_order_rays_workspace(int64_t n);
int vr_order_rays(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                  const VrRayOrder* out, void* workspace, size_t workspace_bytes, void* stream);
/* Sizes n_slots (1..8) launch slots so that no later ray call of <= n rays on them allocates or blocks (the
 * colour record plus the scratch of a call without rgba: 80-232 bytes per ray).  Optional; synchronous. */
int vr_reserve_rays(vr_tree_t tree, int64_t n, int n_slots);
/* Pre-allocates the ray buffers of two launch slots for batches of up to n_frames whole
 * width x height frames (128-228 bytes per ray): a render loop on one stream lives in one slot,
 * two alternating streams in two, so no later vr_render / vr_render_batch of that size (or
 * smaller, or tile-sharded) on them allocates or blocks.  Optional; synchronous. */
int vr_reserve(vr_tree_t tree, int width, int height, int n_frames);
/* The same for a tile-sharded render loop: the ray buffer of a launch holds its rank's tiles
 * rounded up to WHOLE tiles (tile_w x tile_h as in VrFrame; 0, 0 = whole-frame tiles), which
 * can exceed the frame-rounded size vr_reserve assumes when tile_h does not divide the height.
 * n_slots launch slots are sized (1..8: one per stream that renders this tree concurrently). */
int vr_reserve_tiles(vr_tree_t tree, int width, int height, int n_frames, int tile_w, int tile_h,
                     int world, int n_slots);
/* Sticky device status word of the tree's launches: bit 0 = some ray hit the sample guard (a
 * wave marched 2^22 rounds -- tuning key "max_iter" -- since the last retire / refill pass in
 * which one of its rays retired; the reference would still be looping).  Synchronous; reset != 0 clears it.
 * vr_render* refuses step_size <= 0 / NaN (VR_ERR_INVALID_ARGUMENT), where the reference
 * hangs, so the bit only ever fires on pathological step_size / scene combinations.  A launch
 * that set it has WRONG pixels (the wave's marching rays were cut; which rays share a wave
 * depends on the scheduling knobs, so such a frame is not tuning-independent either): vr_render*
 * is enqueue-only and cannot report it, so every render loop checks this word once its last
 * launch has finished -- volrend_headless, TileShardRenderer::sync, VolumeRenderer::read_frame
 * and bench.py do, and fail loudly (the reference's abort-on-error convention,
 * src/cuda/common.cu:8-21). */
int vr_tree_status(vr_tree_t tree, uint32_t* status, int reset);
/* The same word read ON A STREAM: the copy (into pinned memory of the library) and, with
 * reset != 0, the clear are enqueued on `stream`; then THAT stream is waited for and the value
 * returned.  No other stream is waited for -- vr_tree_status copies on the legacy stream and so
 * waits for every blocking stream of the device: a render loop on two alternating streams that
 * checks frame k would wait for frame k + 1 as well.  The word is the TREE's: launches of the same
 * tree on other streams set the same bits, and whichever check comes first reports them. */
int vr_tree_status_on(vr_tree_t tree, uint32_t* status, int reset, void* stream);
/* Scheduling / layout knobs ("march_max", "refill_min", "waves_per_cu", "records_nt", "raygen_waves",
 * "top_levels", "brick_levels", "brick_blocked", ...); results never depend on them ("max_iter", the sample
 * guard above, is the exception by design: a launch that trips it says so in vr_tree_status).  Every tree carries its own
 * copy, taken at upload (or from the source of a clone) from the process defaults:
 *   vr_set_tuning       changes the DEFAULTS of trees uploaded afterwards (serialised);
 *   vr_tree_set_tuning  changes one tree (not the upload-time keys top_levels / brick_levels /
 *                       brick_blocked: VR_ERR_INVALID_ARGUMENT);
 *                       takes effect with that tree's next launch, any thread. */
int vr_set_tuning(const char* key, int value);
int vr_tree_set_tuning(vr_tree_t tree, const char* key, int value);
/* Scheduling tallies accumulated by instrumented launches (frames with counters):
 * [0] march rounds [1] lanes busy in them [2] shade rounds [3] lanes busy in them
 * [4] distinct leaves summed over shade rounds [5] retire rounds [6] rays retired in them [7] scheduler iterations.
 * Synchronous (copies from the device); reset != 0 clears them. */
int vr_sched_stats(vr_tree_t tree, uint64_t out[8], int reset);
/* Block cull (tuning key "block_cull", default 1): in colour and AOV frame launches of a tree on the N == 2
 * lookup path, ray generation skips the 8x8 pixel blocks whose rays provably meet no cell with sigma > 0 -- they
 * get the pixel of a ray without a hit sample, which is the pixel they would have got.  Not with sigma_thresh < 0,
 * NDC trees, a render_bbox outside the unit cube, counters / render_depth / SG / ASG, or a camera whose plane cuts an
 * occupied cell.  out[0] = blocks that launches with the cull on have generated or skipped, out[1] = the skipped
 * ones among them.  Synchronous (copies from the device); reset != 0 clears them. */
int vr_tree_cull_stats(vr_tree_t tree, uint64_t out[2], int reset);
/* Lead-in march (tuning key "head_march", default 1): in colour and AOV frame launches of a tree on the N == 2
 * lookup path, ray generation takes a ray's samples in front of its first sample with sigma > sigma_thresh -- they
 * change nothing of the ray but t -- and hands the ray over at the t it has reached; a ray that reaches its tmax
 * without such a sample gets the pixel of a ray without a hit sample there.  The sample sequence is the march
 * kernel's own: no pixel and no plane changes.  Not with counters / render_depth / SG / ASG, ray lists, or
 * "max_iter" below its default.  "head_min_lanes" (1..64) and "head_max" say when the 64 rays of a block are
 * handed over: once fewer of them still march, or after that many rounds; 0 = the library's choice.
 * out[0] = rays that entered the lead-in march, out[1] = those that ended in it, out[2] = samples marched there.
 * Synchronous (copies from the device); reset != 0 clears them. */
int vr_tree_head_stats(vr_tree_t tree, uint64_t out[3], int reset);
/* Distinct-line meter (SURVEY.md 8(d) "B_unique", the compulsory-traffic lower bound): with
 * enable != 0 the tree gets one bit per 128-byte line of its device arrays, and every
 * INSTRUMENTED launch (frames with counters) sets the bits of the lines its accesses touch.
 * vr_touch_count returns the number of distinct lines touched since the last reset in
 * out[0..3] = coefficient records, child words, top grid, bricks (x 128 = bytes).  Both calls
 * are synchronous (device-wide).  Production launches never see the bitmaps. */
int vr_touch_enable(vr_tree_t tree, int enable);
int vr_touch_count(vr_tree_t tree, uint64_t out[4], int reset);
/* The bitmap of array `which` (0 records, 1 child words, 2 top grid, 3 bricks) itself, copied to
 * host memory: bit b of word w = granule 32 w + b of the array was touched; *granule_bytes (if
 * not NULL) receives the bytes one bit stands for (128; layout studies build the library with
 * a finer grain for the records).  Copies min(n_words, size of the bitmap) words and returns
 * the size of the bitmap in *bitmap_words (if not NULL).  Synchronous. */
int vr_touch_read(vr_tree_t tree, int which, uint32_t* host_words, uint64_t n_words,
                  uint64_t* bitmap_words, uint64_t* granule_bytes);
/* gathered = world consecutive COMPACT buffers (rank-major), all device memory
 * on the current device.  Writes the W x H frame. */
int vr_assemble_tiles(void* frame_rgba, int64_t pitch, const void* gathered, int width,
                      int height, int tile_w, int tile_h, int world, void* stream);
/* The same for n_frames at once (one launch): frame i is written at
 * frames_rgba + i*frame_stride; rank r's COMPACT buffer of frame i is read at
 * gathered + r*rank_stride + i*in_frame_stride -- e.g. a [world][n_frames][compact_bytes]
 * gather result has rank_stride = n_frames*compact_bytes, in_frame_stride = compact_bytes. */
int vr_assemble_tiles_batch(void* frames_rgba, int64_t frame_stride, int64_t pitch,
                            const void* gathered, int64_t rank_stride, int64_t in_frame_stride,
                            int n_frames, int width, int height, int tile_w, int tile_h, int world,
                            void* stream);
/* out_dev: device float[data_dim-1]; the lumisphere at opt->probe. */
int vr_probe_coeffs(vr_tree_t tree, const VrRenderOptions* opt, float* out_dev, void* stream);

/* ---- bulk point queries ------------------------------------------------ */
/* What the uploaded tree holds at many points at once: query_single_from_root
 * (n3tree_query.hpp:13-48) per point, the record of the leaf it finds, and the colour a sample
 * there has along a direction (rt_core.cuh:125-163) -- vr_probe_coeffs for n points in one launch,
 * through the lookup structure of the tree where upload built one.  Every output is a pure
 * function of one point (and one direction), bit-identical to the reference's arithmetic.
 *
 * Both calls only enqueue on `stream`, run on the tree's device whatever the thread's current
 * device is, take no launch slot, hold no per-call scratch and only read the tree: any number of
 * them may run beside each other and beside vr_render* launches, on any streams and host threads.
 *
 * Position.  VR_SPACE_WORLD: tree coordinate = offset + scale * x (one rounding per operator, as
 * vr_probe_coeffs); VR_SPACE_TREE: x is a tree coordinate already.  The tree coordinate is clamped
 * as the reference writes it, max(min(x, 1 - 1e-6f), 0), so every input is defined: NaN goes to
 * 1 - 1e-6f, -0 to +0, +-inf to the ends.  (The render kernels clamp with one median instruction,
 * which sends NaN to 0; a point query pays the second instruction.)
 *
 * rgb.  SH trees: 1 / (1 + exp(-tmp)) per channel, tmp the basis-weighted sum of the channel's
 * coefficients in the reference's association (groups 25, 16, 9, 4, each left to right), over
 * the whole basis (no basis_minmax, no rot_dirs); basis sizes other than 4 / 9 / 16 / 25 use the
 * first coefficient of each channel, as vr_render does.  RGBA trees: the first three entries of
 * the record.  The basis is evaluated at dirs[i] AS GIVEN: the library does not normalise it (the
 * reference normalises a ray's direction before it becomes the view direction; pass a unit vector
 * to get a sample's colour).  Evaluated in the VR_FP_STRICT model only, independent of sigma (no
 * sigma_thresh).  SG / ASG trees: VR_ERR_UNSUPPORTED when rgb is asked for; the other outputs work. */
enum { VR_SPACE_WORLD = 0, VR_SPACE_TREE = 1 };

typedef struct VrQueryOut {   /* device pointers; NULL = not wanted; at least one non-NULL */
    float* sigma;    /* [n]             density of the leaf (fp16 -> fp32, exact) */
    int32_t* depth;  /* [n]             depth of the leaf as VrTreeInfo.max_depth counts it (child words read - 1) */
    float* local;    /* [n][3]          leaf-local coordinate: xyz as query_single_from_root leaves it */
    float* coeffs;   /* [n][data_dim-1] the record (fp16 -> fp32, exact): what vr_probe_coeffs gives */
    float* rgb;      /* [n][3]          colour of a sample at the point along dirs[i]; needs directions */
} VrQueryOut;

/* xyz_dev [n][3], dirs_dev [n][3] or NULL: device float32.  n == 0 is VR_OK and launches nothing.
 * VR_ERR_INVALID_ARGUMENT: NULL tree / xyz / out, every output NULL, rgb without dirs, n < 0,
 * unknown space. */
int vr_query_points(vr_tree_t tree, int64_t n, const float* xyz_dev, const float* dirs_dev, int space,
                    const VrQueryOut* out, void* stream);
/* The same for the res[0] * res[1] * res[2] cell centres of the box lo..hi (host arrays), generated
 * on the device: cell (i, j, k) has output index (i * res[1] + j) * res[2] + k and per axis the
 * coordinate lo + ((float)i + 0.5f) * ((hi - lo) / (float)res) in binary32, one rounding per
 * operator.  dir: one direction for all cells, or NULL.  Also VR_ERR_INVALID_ARGUMENT: NULL lo /
 * hi / res, a res[i] < 1, more than 2^40 cells. */
int vr_query_grid(vr_tree_t tree, const float lo[3], const float hi[3], const int32_t res[3],
                  const float dir[3], int space, const VrQueryOut* out, void* stream);

/* Async D2H of a pitched RGBA8 frame into tightly packed host memory. */
int vr_read_back(void* host_rgba, const void* dev_rgba, int64_t pitch, int width, int height,
                 void* stream);
int vr_stream_sync(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VOLREND_HIP_H_ */
