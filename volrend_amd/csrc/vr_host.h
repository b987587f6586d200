// vr_host.h -- shared by the host sources of libvolrend_hip.so (vr_api.cpp, vr_upload.cpp,
// vr_launch.cpp, vr_query.cpp).  Host only (not for the .hip units); nothing here is exported from the
// library.  Two host units stand beside it with headers of their own: vr_tree_walk.{h,cpp} (the walks
// of an upload over the child array; no HIP) and vr_h2d.{h,cpp} (the upload's staged copy pipeline).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "vr_internal.h"

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

// Scheduling / layout knobs.  They never change results.  Every tree carries its OWN copy
// (vr_tree_set_tuning), taken at upload from the process defaults; the defaults come from
// the environment (VR_MARCH_MAX, VR_REFILL_MIN, VR_WAVES_PER_CU, ... read once) and
// vr_set_tuning, which only affects trees uploaded afterwards.  vr_api.cpp keeps the table of
// keys, variables and clamps.
struct Tuning {
    int march_max = 12;
    int refill_min = 20;
    int drain_flush = 16;  // drain phase: partial round for a blocked ray when <= this many lanes march (0 = off;
                           // measured 4..64, profiles/r05_experiments.jsonl: one frame per launch -13 %, two / four -5 %)
    int waves_per_cu = 0;   // 0: what the kernel flavour fits (vr_render.hip waves_per_cu<>)
    int frame_group = 0;   // poses per ray-order group (0 = all poses of the launch, 1 = frame-major)
    int super_block = 0;   // 8x8 blocks per super-block edge in the ray order (1 = row-major); 0 = auto: by the kind and
                           // size of the launch (auto_super_block, vr_launch.cpp)
    int records_nt = -1;   // record stream non-temporal: -1 = by lookup-structure size, 0 / 1 = forced
    int xcd_queues = 1;
    int chunk_max = 0;     // cap of the guided chunk a wave takes from its queue at once (multiple of 64); 0 = auto:
                           // by the kind of launch (auto_chunk_max, vr_launch.cpp)
    int raygen_waves = 0;  // waves per ray-generation workgroup: 16 / 4 / 1; 0 = by launch size (vr_render_batch)
    int top_levels = 0;    // lookup structure built at upload (vr_dev_layout.h); 0 = auto
    int brick_levels = 3;
    int brick_blocked = -1;  // 8^3 bricks in 4 x 4 x 2 line blocks: -1 = when the lookup structure exceeds 128 MB, 0 / 1 = forced
    int max_iter = 1 << 22;  // the sample guard (vr_render.hip); the one knob that is NOT scheduling-only:
                             // a launch that trips it reports through vr_tree_status (tests lower it)
    int weights_check = 1;   // vr_accumulate_weights: read max_weight[slot] first and issue the atomic max only
                             // for a larger weight (0: one atomic per positive weight; vr_weights.hip, EXPERIMENTS.md)
};
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
    bool growing = false;       // its ray buffer is being reallocated outside the launch mutex: skip it
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
    uint64_t device_bytes = 0;
};

struct VrTreeOpaque : TreeShape {
    int device = 0;
    DeviceBuffer arrays[4];      // TreeArray: leaves (uint16_t), nodes (uint32_t), top (uint2), bricks (uint32_t)
    DeviceBuffer extra, status, sched_stats;  // float, uint32_t, vr::kSchedStats x u64 (vr_sched_stats)
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
    LaunchSlot slots[kLaunchSlots];
    unsigned launch_seq = 0;
    std::mutex launch_mutex;  // slot bookkeeping + enqueue order of one launch; guards `tn`
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

#pragma GCC visibility pop
