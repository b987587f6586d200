// vr_launch_plan.h -- the scheduling rules of a march launch: what the knobs that are "auto" by default resolve
// to for one launch.  They never change a pixel or a gradient, so no parity test sees them move:
// tests/cpp/launch_plan_check.cpp pins them.  Standard C++ only (no HIP header, no vr_host.h), built by a plain
// host compiler there.  Nothing here is exported from the library.
#pragma once
#include <cstdint>

#pragma GCC visibility push(hidden)

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
                           // size of the launch (plan_launch)
    int records_nt = -1;   // record stream non-temporal: -1 = by lookup-structure size, 0 / 1 = forced
    int xcd_queues = 1;
    int chunk_max = 0;     // cap of the guided chunk a wave takes from its queue at once (multiple of 64); 0 = auto:
                           // by the kind of launch (plan_launch)
    int raygen_waves = 0;  // waves per ray-generation workgroup: 16 / 4 / 1; 0 = by launch size (plan_launch)
    int top_levels = 0;    // lookup structure built at upload (vr_dev_layout.h); 0 = auto
    int brick_levels = 3;
    int brick_blocked = -1;  // 8^3 bricks in 4 x 4 x 2 line blocks: -1 = when the lookup structure exceeds 128 MB, 0 / 1 = forced
    int max_iter = 1 << 22;  // the sample guard (vr_render.hip); the one knob that is NOT scheduling-only:
                             // a launch that trips it reports through vr_tree_status (tests lower it)
    int weights_check = 1;   // vr_accumulate_weights: read max_weight[slot] first and issue the atomic max only
                             // for a larger weight (0: one atomic per positive weight; vr_weights.hip, EXPERIMENTS.md)
    int block_cull = 1;      // colour / AOV frame launches: ray generation culls the 8x8 pixel blocks that meet no
                             // occupied cell (vr_internal.h "Block cull"; 0: every block generates its rays)
    int head_march = 1;      // colour / AOV frame launches: ray generation marches a ray's samples in front of its first
                             // hit sample (vr_internal.h "Lead-in march"; 0: every ray is handed over at the box entry)
    int head_min_lanes = 0;  // the wave hands its rays over once fewer lanes march (1..64); 0 = auto (plan_launch)
    int head_max = 0;        // lead-in rounds of a wave at most; 0 = auto (plan_launch)
};

// The march kernel of a launch, and what its rays come from: the pixels of n_frames poses, or a list of rays
// (which the kernels see as ONE pseudo-frame, vr_internal.h).
enum class LaunchKind { kColour, kAov, kWeights, kBackward };
enum class RaySource { kFrames, kList };

constexpr int kPlanQueues = 8;  // vr::kMaxQueues, one per XCD (vr_launch.cpp asserts that they agree)

struct LaunchPlan {
    int chunk_max, super_block, records_nt, frame_group, n_queues;  // the KParams fields of these names
    int raygen_waves;                                               // waves per ray-generation workgroup
    int head_max, head_min_lanes;  // the lead-in march of ray generation: rounds (0 = none) and the hand-over bound
};

// n_frames: the poses of the launch (a list: its one pseudo-frame); list_rays: the rays of a list (frames:
// not read); lookup_bytes: the tree's lookup structure, top grid plus bricks.
// lead_in: the tree and the kernel flavour of the launch admit the lead-in march of ray generation (vr_launch.cpp
// lead_in_applies; the plan then says whether the launch runs it).
LaunchPlan plan_launch(LaunchKind kind, RaySource source, int n_frames, int64_t list_rays, const Tuning& tn,
                       uint64_t lookup_bytes, bool lead_in = false);

#pragma GCC visibility pop
