// vr_weights.hip -- vr_accumulate_weights: per leaf, the largest compositing weight a sample in it received
// from any ray of a set of views, and how many hit samples fell into it (svox's accumulate_weights; what
// PlenOctree extraction and pruning threshold on).
//
// The march is render_kernel's march phase (vr_render.hip) without everything a colour needs: no records,
// no ring, no stage, no shade round, no basis, no pixel.  Ray generation, the point query, the step, the
// attenuation and the stop test are the device functions the colour kernels use (vr_dev_rays.h,
// vr_dev_query.h, vr_device_math.h), so weight = light_intensity * (1 - att) has the bits trace_ray
// (rt_core.cuh:66-196) gives it in either FP model.  Built with -ffp-contract=off; see vr_device_math.h.
//
// Outputs are indexed in the FILE's node numbering (VrTreeDesc.child / data): a device leaf id goes
// through WeightParams.file_node.  Both updates commute (an unsigned maximum over bit patterns of
// non-negative floats, a count modulo 2^32): any number of launches may run beside each other.
#include "vr_dev_march.h"

namespace vr {

namespace {

constexpr int kWeightWaves = 8;  // per SIMD: the march state fits 64 VGPRs (profiles/leaf_weights_kernel_resources.txt)

typedef __attribute__((address_space(1))) uint32_t vr_gu32_t;
typedef __attribute__((address_space(1))) const uint32_t vr_gcu32_t;
typedef __attribute__((address_space(1))) const int32_t vr_gci32_t;

// ---------------------------------------------------------------------------
// weights_kernel: the persistent march, over the frame of vr_dev_march.h (WeightRecord rays: the march words
// alone).
//
// The per-hit update.  The march leaves a leaf after every sample, so consecutive hits of a ray are in
// different leaves and the updates of a wave instruction scatter over 64 rows -- the access shape at
// which the chip's memory-side atomics run ~17x below their streaming rate.  So:
//   hits        one non-returning atomic add per hit sample: there is no way around it;
//   max_weight  (CHECK) the word is READ first and the atomic max only issued when the weight is larger.
//               A stale value (another XCD's L2, an update in flight) can only be too small, which costs
//               a redundant atomic and never loses an update: the atomic itself decides.
// Neither the file_node load nor the checking load may sit on the march's dependent chain, so the update
// runs as a three-stage pipeline BEHIND the march, one stage per march round:
//   stage 1 (the round of the hit)  remember (leaf, weight bits); request file_node[leaf / N3]
//   stage 2 (one round later)       slot = file node * N3 + leaf % N3; hits[slot] += 1; request max_weight[slot]
//   stage 3 (two rounds later)      weight bits > the word read ?  atomic max
// Each stage uses a value whose load was issued a whole round -- a tree lookup -- earlier; loads return
// in order, so the wait for the round's own lookup has already covered it.
// ---------------------------------------------------------------------------
template <int FMA, int QUERY, bool HITS, bool CHECK>
__global__ __launch_bounds__(kWave, kWeightWaves) void weights_kernel(const KParams p, const WeightParams wp) {
    constexpr bool N2 = QUERY != kQueryGeneric;
    const int lane = threadIdx.x & (kWave - 1);
    float cen[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f}, invdir[3] = {1.f, 1.f, 1.f};
    float t = 0.f, tmax = -1.f, delta_scale = 1.f, light = 1.f;
    bool active = false;  // the lane holds a ray (marching or finished)
    Cursor cur;
    uint32_t rounds = 0, progress_round = 0;
    bool exhausted = false;
    uint32_t chunk_next = 0, chunk_end = 0;
    // the update pipeline (see above); kNoLeaf / zero bits = an empty stage
    constexpr uint32_t kNoLeaf = 0xFFFFFFFFu;
    uint32_t s1_leaf = kNoLeaf, s1_bits = 0, s1_node = 0;
    uint32_t s2_slot = 0, s2_bits = 0, s2_seen = 0;
    vr_gu32_t* const g_max = (vr_gu32_t*)wp.max_weight;  // NULL: hits only (launch-uniform)
    vr_gu32_t* const g_hits = (vr_gu32_t*)wp.hits;
    vr_gci32_t* const g_file = (vr_gci32_t*)wp.file_node;

    // One turn of the pipeline.  (leaf, bits): the hit of this round, or (kNoLeaf, 0).
    auto update = [&](uint32_t leaf, uint32_t bits) {
        // stage 3
        if (CHECK && s2_bits > s2_seen)
            __hip_atomic_fetch_max(g_max + s2_slot, s2_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s2_bits = 0;
        // stage 2
        if (s1_leaf != kNoLeaf) {
            const uint32_t slot = file_slot<N2>(p, s1_node, s1_leaf);
            if (HITS) __hip_atomic_fetch_add(g_hits + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s1_bits != 0u) {  // (zero bits: max_weight not wanted, or a weight <= 0 / NaN)
                if (CHECK) {
                    s2_slot = slot;
                    s2_bits = s1_bits;
                    s2_seen = *(vr_gcu32_t*)(g_max + slot);
                } else {
                    __hip_atomic_fetch_max(g_max + slot, s1_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        // stage 1
        s1_leaf = leaf;
        s1_bits = bits;
        if (leaf != kNoLeaf) s1_node = (uint32_t)g_file[file_node_index<N2>(p, leaf)];
    };

    for (;;) {
        // ---- retire and refill: a weight ray is its march words, and there is no state per ray but the march's ----
        const MarchFeed feed = march_refill(
            p, lane, kWeightRayWords, rounds, MarchFeed{exhausted, chunk_next, chunk_end, progress_round}, active, cen,
            dir, invdir, t, tmax, delta_scale, light, cur, [](const uint32_t*, uint32_t) {}, [] {});
        // (into plain locals, never a kept struct: vr_dev_march.h "Retire and refill" -- ten VGPRs)
        exhausted = feed.exhausted;
        chunk_next = feed.chunk_next;
        chunk_end = feed.chunk_end;
        progress_round = feed.progress_round;
        if (!wave_any(active)) {
            if (exhausted) break;
            continue;
        }

        sample_guard(p, rounds, progress_round, t, tmax);
        int m = 0;
        for (; m < p.march_max; ++m) {
            if (__builtin_amdgcn_ballot_w64(t < tmax) == 0ull) break;
            uint32_t hit_leaf = kNoLeaf, hit_bits = 0;
            if (t < tmax) {
                float delta_t, sigma;
                const uint32_t leaf = march_sample<FMA, QUERY>(p, t, cen, dir, invdir, cur, delta_t, sigma);
                bool stop = false;
                if (sigma > p.sigma_thresh) {
                    float att;
                    const float weight = sample_weight(light, delta_t, delta_scale, sigma, att);
                    hit_leaf = leaf;
                    if (g_max && weight > 0.f) hit_bits = f2u(weight);  // (false for NaN)
                    light *= att;
                    stop = light < p.stop_thresh;
                }
                if (stop) tmax = -1.f;  // stopped (and no longer alive)
                else t += delta_t;
            }
            update(hit_leaf, hit_bits);
        }
        rounds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(rounds + (uint32_t)m));
    }
    // what is still in the pipeline
    update(kNoLeaf, 0u);
    update(kNoLeaf, 0u);
    update(kNoLeaf, 0u);
}

template <int FMA, int QUERY, bool HITS>
void launch_march_check(const KParams& p, const WeightParams& w, bool check_first, dim3 grid, hipStream_t s) {
    if (check_first) hipLaunchKernelGGL((weights_kernel<FMA, QUERY, HITS, true>), grid, dim3(kWave), 0, s, p, w);
    else hipLaunchKernelGGL((weights_kernel<FMA, QUERY, HITS, false>), grid, dim3(kWave), 0, s, p, w);
}

template <int FMA>
hipError_t launch_fp(const KParams& p, const WeightParams& w, int n_cus, int waves_override, int gen_waves,
                     bool check_first, hipStream_t s, const RayList* rays) {
    const int64_t total_blocks = p.n_wave_blocks * p.n_frames;
    launch_march_raygen<FMA, WeightRecord>(p, gen_waves, s, rays);
    const dim3 grid(persistent_grid(total_blocks, n_cus, waves_override > 0 ? waves_override : 4 * kWeightWaves));
    const bool hits = w.hits != nullptr;
    dispatch_query(query_kind(p), [&](auto query) {
        constexpr int Q = decltype(query)::value;
        if (hits) launch_march_check<FMA, Q, true>(p, w, check_first, grid, s);
        else launch_march_check<FMA, Q, false>(p, w, check_first, grid, s);
    });
    return hipGetLastError();
}

}  // namespace

hipError_t launch_weights(const KParams& p, const WeightParams& w, int fp_mode, int n_cus, int waves_override,
                          int gen_waves, bool check_first, hipStream_t stream, const RayList* rays) {
    if (p.n_wave_blocks <= 0 || p.n_frames <= 0) return hipSuccess;
    return fp_mode == VR_FP_FMA ? launch_fp<1>(p, w, n_cus, waves_override, gen_waves, check_first, stream, rays)
                                : launch_fp<0>(p, w, n_cus, waves_override, gen_waves, check_first, stream, rays);
}

}  // namespace vr
