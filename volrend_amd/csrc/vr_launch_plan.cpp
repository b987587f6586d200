// vr_launch_plan.cpp -- the scheduling rules of a march launch (vr_launch_plan.h).  Standard C++ only.
#include "vr_launch_plan.h"

namespace {

// The knobs that are "auto" (0) by default, resolved for one launch.  `colour`: a colour or AOV launch
// (render_kernel, with or without AovParams); the leaf-weight and backward launches keep the values they were
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
constexpr uint64_t kBigLookup = 128ull << 20;  // lookup structure (top + bricks) beyond 4x the aggregate L2
// The lead-in march of ray generation (vr_internal.h "Lead-in march"): a wave marches while at least
// kAutoHeadMinLanes of its 64 rays have not met density yet, kAutoHeadMax rounds at most.  On the C1 bench orbit the
// rays of an 8x8 block need 21-23 lockstep rounds to their first hits.  The rounds beyond the bounds are the long
// tails of a few rays: each costs a round of ray generation, and the persistent kernel marches them beside other
// rays.  Measured on C1 at 64 frames per launch (EXPERIMENTS.md "Lead-in march"): 32 / 32 and 32 / 16 are the
// fastest, 16 / 64 is 1 % behind them, marching every ray to its first hit (1 / unbounded) gains nothing.
constexpr int kAutoHeadMinLanes = 32, kAutoHeadMax = 32;

// waves per ray-generation workgroup: 16 (one atomic per 1024 pixels) -- except launches of one or
// two frames, the ones that run beside the tail of a neighbour on another stream: workgroups of
// 4 waves find room there much earlier (vr_render.hip raygen_kernel; profiles/r06_raygen_waves.jsonl:
// two streams -10 % / -6.5 % at one / two frames per launch, one stream +-0; from four frames on the
// 4x atomics cost a lone launch 3-4 %, and one-wave workgroups 35 %)
// With the lead-in march (head) the waves of a workgroup run for as long as their blocks' lead-ins take, 0 to
// head_max rounds: a workgroup of 16 waves waits at its barrier for the slowest of them, and its successor needs four
// free wave slots on every SIMD at once.  Workgroups of 4 waves for every launch size then: a 64-frame C1 launch takes
// 0.218 ms per frame against 0.237 with 16 (and 0.224 without the lead-in; EXPERIMENTS.md "Lead-in march").
int raygen_waves(const Tuning& tn, int n_frames, bool head) {
    return tn.raygen_waves > 0 ? tn.raygen_waves : (head || n_frames <= 2 ? 4 : 16);
}
// A ray list: the same reasoning by ray count.  The frame rule was measured at 800 x 800 pixels, where "two
// frames" are 1 280 000 rays: lists up to kRayListSmall rays -- an optimiser's step, which runs beside the tail
// of the step before it -- generate in workgroups of 4 waves, larger ones in 16.  UNMEASURED for lists: the
// boundary is the frame rule's, restated in rays.  (List ray generation has no one-wave flavour.)
constexpr int64_t kRayListSmall = 2 * 800 * 800;
int raygen_waves_list(const Tuning& tn, int64_t n) {
    return tn.raygen_waves > 0 ? (tn.raygen_waves >= 16 ? 16 : 4) : (n <= kRayListSmall ? 4 : 16);
}

}  // namespace

LaunchPlan plan_launch(LaunchKind kind, RaySource source, int n_frames, int64_t list_rays, const Tuning& tn,
                       uint64_t lookup_bytes, bool lead_in) {
    const bool colour = kind == LaunchKind::kColour || kind == LaunchKind::kAov;
    const bool list = source == RaySource::kList;
    LaunchPlan p;
    p.chunk_max = tn.chunk_max > 0 ? tn.chunk_max : colour ? kColourChunkCap : kGuidedChunkCap;
    p.super_block = tn.super_block > 0 ? tn.super_block : (colour && !list && n_frames > 2) ? 4 : 1;
    // the lead-in march: frame launches of the colour kernels whose tree and flavour admit it, and only under the
    // default sample guard -- a ray that a lowered max_iter cuts short must be cut, and reported, by the march kernel
    // Not on auto for a lookup structure beyond 4x the aggregate L2 (the records_nt bound below): the lead-in's loads
    // miss there as the march kernel's do, and C3 at 64 frames per launch is 2.3 % slower with it (one frame: even).
    // A head_max of the caller's asks for it all the same.
    const bool head = lead_in && tn.head_march && colour && !list && tn.max_iter >= Tuning().max_iter &&
                      (tn.head_max > 0 || lookup_bytes <= kBigLookup);
    p.head_max = !head ? 0 : tn.head_max > 0 ? tn.head_max : kAutoHeadMax;
    p.head_min_lanes = tn.head_min_lanes > 0 ? tn.head_min_lanes : kAutoHeadMinLanes;
    p.raygen_waves = list ? raygen_waves_list(tn, list_rays) : raygen_waves(tn, n_frames, head);
    // lookup structure (top + bricks) beyond 4x the aggregate L2 (8 x 4 MiB on MI355X): the record
    // stream would keep evicting it -- see the DMA loads in vr_render.hip
    p.records_nt = tn.records_nt >= 0 ? tn.records_nt : lookup_bytes > kBigLookup;
    p.frame_group = tn.frame_group < 1 || tn.frame_group > n_frames ? n_frames : tn.frame_group;
    p.n_queues = tn.xcd_queues ? kPlanQueues : 1;
    return p;
}
