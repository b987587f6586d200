// vr_host.h -- shared by the host sources of libvolrend_hip.so (vr_api.cpp, vr_upload.cpp, vr_launch.cpp,
// vr_slots.cpp, vr_values.cpp, vr_query.cpp, vr_order.cpp, vr_refine.cpp, vr_collapse.cpp, vr_geometry.cpp, vr_quantize.cpp).  Host only (not for the .hip units); nothing here is exported
// from the library.  Three host units stand beside it with headers of their own: vr_tree_walk.{h,cpp} (the walks
// of an upload over the child array; no HIP), vr_launch_plan.{h,cpp} (struct Tuning and the scheduling rules of a
// launch; no HIP) and vr_h2d.{h,cpp} (the upload's staged copy pipeline).
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <mutex>
#include <vector>

#include "vr_internal.h"
#include "vr_launch_plan.h"  // struct Tuning, and the scheduling rules of a launch

#pragma GCC visibility push(hidden)

// DeviceGuard, DeviceBuffer, DeviceEvent (inside the hidden region: they are not exported either).
// A tree lives on ONE device; its calls run there under a DeviceGuard whatever the calling thread's
// current device is (one host thread may drive the trees of several devices), and leave the
// thread's device as they found it.
#include "volrend/internal/hip_owners.hpp"
using volrend::internal::DeviceBuffer;
using volrend::internal::DeviceEvent;
using volrend::internal::DeviceGuard;

// Formats the message vr_last_error() returns (one buffer per thread, vr_api.cpp); returns `code`.
int fail(int code, const char* fmt, ...);
inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? VR_ERR_OUT_OF_MEMORY : VR_ERR_HIP; }

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(hip_code(e_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                    \
    } while (0)

Tuning default_tuning();  // the process defaults, for a tree being uploaded

constexpr unsigned kLaunchSlots = 8;

// Per-launch scratch that a kernel reads while it runs: frame table, queue heads, ray count,
// ray buffer, probe coefficients.  `done` is recorded on the launch's stream behind its last
// kernel and the next user of the slot makes ITS stream wait for it (device-side wait, the host
// never blocks), so any number of launches on any number of streams may be in flight -- beyond
// kLaunchSlots they simply serialise.  A launch prefers the slot its own stream used last (the
// stream orders the two launches anyway), then a slot whose last launch has finished, and only
// then the next slot of the ring: a render loop on one stream lives in ONE slot and one ray
// buffer however far the host runs ahead, two alternating streams in two.
struct LaunchSlot {
    DeviceEvent done;
    bool used = false;          // `done` has been recorded at least once
    hipStream_t last_stream = nullptr;  // the stream of that launch
    bool growing = false;       // its ray buffer is being reallocated outside the launch mutex: skip it (all growing: wait)
    DeviceBuffer rays;          // ray buffer, grown on demand (or up front by vr_reserve)
};

// The tree arrays in device layout (vr_dev_layout.h), in the order of the touch bitmaps.
enum TreeArray { kLeaves = 0, kNodes = 1, kTop = 2, kBricks = 3 };

// What a tree is apart from its device memory: vr_tree_clone copies it in one assignment.
struct TreeShape {
    VrTreeDesc desc{};  // pointers cleared; scalars kept
    int32_t max_depth = 0;
    int leaf_stride_h = 0;
    int top_levels = 0, brick_levels = 0, n_bricks = 0;  // lookup structure (N == 2), see vr_dev_layout.h
    int brick_blocked = 0;  // entry order of the bricks (vr_dev_layout.h), fixed at upload
    int occ_levels = -1;    // g of the block cull's occupancy (vr_internal.h "Block cull"); -1: the tree has none
    uint64_t device_bytes = 0;
};

struct VrTreeOpaque : TreeShape {
    int device = 0;
    DeviceBuffer arrays[4];      // TreeArray: leaves (uint16_t), nodes (uint32_t), top (uint2), bricks (uint32_t)
    DeviceBuffer extra, status, sched_stats;  // float, uint32_t, vr::kSchedStats x u64 (vr_sched_stats)
    DeviceBuffer occ;            // vr::occ_words(occ_levels) uint32_t: length, bitmap and boundary list of the block cull
    DeviceBuffer cull_stats;     // vr::kCullStatLines x vr::kCullStatStride u64 (vr_tree_cull_stats)
    DeviceBuffer head_stats;     // the same shape, vr::kHeadStatWords words of a line in use (vr_tree_head_stats)
    DeviceBuffer touch[4];       // distinct-line bitmaps of the arrays (vr_touch_enable)
    DeviceBuffer touch_out;      // 4 x u64
    DeviceBuffer probe_buf;      // kLaunchSlots x data_dim floats: the lumisphere at opt.probe
    DeviceBuffer slot_frames;    // kLaunchSlots x kMaxBatch vr::FrameDesc
    DeviceBuffer slot_heads;     // kLaunchSlots x vr::kSlotWords uint32_t
    DeviceBuffer slot_aovs;      // kLaunchSlots x kMaxBatch vr::AovDesc: the plane pointers of an AOV launch
    std::vector<int32_t> file_node;  // device node -> the file's node: the inverse of the upload's renumbering (host)
    DeviceBuffer file_node_dev;  // its device copy, made by the first vr_accumulate_weights (then in device_bytes)
    std::vector<int32_t> brick_root;  // n_bricks: the node of each brick, ascending (host; empty without bricks)
    DeviceBuffer brick_root_dev;  // its device copy, made by the first vr_tree_update_data / vr_tree_read_data (then in device_bytes)
    DeviceBuffer node_of_file_dev;  // file node -> device node, the inverse of file_node: made by the first vr_tree_step (then in device_bytes)
    LaunchSlot slots[kLaunchSlots];
    unsigned launch_seq = 0;
    std::mutex launch_mutex;  // slot bookkeeping + enqueue order of one launch; guards `tn`
    std::condition_variable slot_grown;  // a slot stopped `growing`: a launch that found all of them growing chooses again
    Tuning tn;                // this tree's knobs (vr_tree_set_tuning)
    int n_cus = 256;
};

void fill_tree_params(vr::KParams& k, const VrTreeOpaque* t);  // the tree's part (vr_launch.cpp)

// The launch geometry, into the sharding fields of `k` (tile_w .. n_wave_blocks): the tile grid of the
// frame and the share of `rank` (tiles are dealt round-robin: rank 0 holds the most).  launch_geometry
// adds total_rays and checks the limits of one launch; tile_geometry sizes compact buffers / assembly.
int tile_geometry(int width, int height, int tile_w, int tile_h, int rank, int world, vr::KParams& k);
int launch_geometry(int width, int height, int tile_w, int tile_h, int rank, int world, int n_frames,
                    vr::KParams& k);
// launch_geometry for a list of n rays (vr::RayList): the one pseudo-frame of vr::kRayListWidth pixels a row
// whose pixel y * width + x is ray i, as whole blocks of 64 rays.  `what` names the function in the refusal.
int list_geometry(const char* what, int64_t n, vr::KParams& k);

// What a launch needs of its slot's ray buffer: the records, and behind them the pixel words the march stores
// for a vr_render_rays without an rgba array.
inline size_t ray_buffer_bytes(uint32_t total_rays, int words_per_ray) {
    return vr::ray_slots(total_rays) * (size_t)words_per_ray * sizeof(uint32_t);
}
inline size_t list_pixel_bytes(uint32_t total_rays) { return (size_t)total_rays * 4; }
// The block masks of a frame launch (vr_internal.h "Block cull"), behind the ray records of its slot: one bit per
// 8x8 block of the frame's tile grid (`k`: tile_geometry), whole groups of four words per frame.
inline uint32_t block_mask_words(const vr::KParams& k) {
    const uint64_t blocks = (uint64_t)k.tiles_x * (uint64_t)(k.tile_w / 8) * (uint64_t)k.tiles_y * (uint64_t)(k.tile_h / 8);
    return (uint32_t)(((blocks + 127) / 128) * 4);
}
inline size_t block_mask_bytes(const vr::KParams& k, int n_frames) {
    return (size_t)block_mask_words(k) * sizeof(uint32_t) * (size_t)n_frames;
}
// Rebuilds the tree's occupancy from its node words, on `hs` (a tree without one: nothing).  Behind every call
// that writes node words, before it returns.  (vr_upload.cpp)
hipError_t refresh_occupancy(const VrTreeOpaque* t, hipStream_t hs);

// Launch slot: per-launch scratch in device memory (ring, see LaunchSlot).  Picks the slot of this
// launch, points `k` at its scratch and makes its ray buffer large enough (`need` bytes).  `guard` holds the
// launch mutex on entry and on return, and is dropped in between while a slot grows -- this launch's, or, when every
// slot is growing under another thread, until one of them is done: the launch waits, it is not refused.  (vr_slots.cpp)
int acquire_slot(VrTreeOpaque* t, std::unique_lock<std::mutex>& guard, hipStream_t hs, vr::KParams& k,
                 size_t need, unsigned& slot);

// A launch's turn at its slot; begin() is the only way to take one.  Whoever used the slot last (any stream)
// must have finished before its scratch is rewritten: begin() makes the stream wait for it (a failed wait
// leaves the slot as it was).  From then on kernels of the launch may be in the stream: whatever happens
// afterwards (a later enqueue failing), the slot's event is recorded behind them and the slot is marked used,
// so that the next user of the slot -- any stream -- waits for whatever did get enqueued.
class SlotTurn {
    LaunchSlot* slot_ = nullptr;
    hipStream_t stream_ = nullptr;
public:
    int begin(LaunchSlot& ls, hipStream_t hs);
    ~SlotTurn();
};

// The device copy `dev` of a host table of the tree (`entries` words; `name` for the messages), made on the
// first call that needs it -- under the launch mutex, that call's one host-blocking step -- and then counted in
// device_bytes.  ensure_file_nodes: the device-node -> file-node table of the leaf-weight, backward and value
// calls.  (vr_values.cpp)
int ensure_device_table(VrTreeOpaque* t, DeviceBuffer& dev, const std::vector<int32_t>& host, size_t entries,
                        const char* name);
int ensure_file_nodes(VrTreeOpaque* t);

#pragma GCC visibility pop
