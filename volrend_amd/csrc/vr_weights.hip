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
#include "vr_device_math.h"
#include "vr_internal.h"
#include "vr_dev_layout.h"
#include "vr_dev_query.h"
#include "vr_dev_rays.h"

namespace vr {

namespace {

// How a flavour finds the leaf: the lookup with x-major or blocked bricks (N == 2), or the literal descent.
enum { kQueryN2 = 0, kQueryN2Blocked = 1, kQueryGeneric = 2 };
constexpr int kWeightWaves = 8;  // per SIMD: the march state fits 64 VGPRs (profiles/leaf_weights_kernel_resources.txt)

typedef __attribute__((address_space(1))) uint32_t vr_gu32_t;
typedef __attribute__((address_space(1))) const uint32_t vr_gcu32_t;
typedef __attribute__((address_space(1))) const int32_t vr_gci32_t;

// ---------------------------------------------------------------------------
// weights_raygen_kernel: one lane per pixel of every frame.  setup_ray as raygen_kernel runs it (the frame
// is offscreen: tmax comes from render_bbox alone); a ray that misses the box is dropped -- there is no
// pixel to composite.  The others are compacted into their queue's region of the ray buffer by the function
// raygen_kernel compacts them with (reserve_ray_slots, vr_dev_rays.h), as records of kWeightRayWords words.
// ---------------------------------------------------------------------------
template <int FMA, int GW>
__global__ __launch_bounds__(kWave* GW) void weights_raygen_kernel(const KParams p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const uint32_t id = (uint32_t)(((int64_t)blockIdx.x * GW + wave) * kWave + lane);
    bool valid = false;
    Ray nr;
    nr.alive = false;
    if (id < p.total_rays) {
        const PixelRef r = locate(p, id);
        if (r.in_image) {
            float vdir[3];  // (the view direction: nothing here reads it)
            setup_ray<FMA>(p, r, nr, vdir);
            valid = nr.alive;
        }
    }
    const unsigned long long m_valid = __builtin_amdgcn_ballot_w64(valid);
    const uint32_t my_base = reserve_ray_slots<GW>(p, m_valid, lane, wave);
    if (!valid) return;
    const uint32_t slot = my_base + lane_rank(m_valid);
    uint32_t* rb = ray_slot(p.ray_buf_rw, kWeightRayWords, slot);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ray_word(rb, kRayCen + i) = f2u(nr.cen[i]);
        ray_word(rb, kRayDir + i) = f2u(nr.dir[i]);
        ray_word(rb, kRayInvDir + i) = f2u(nr.invdir[i]);
    }
    ray_word(rb, kRayT) = f2u(nr.t);
    ray_word(rb, kRayTmax) = f2u(nr.tmax);
    ray_word(rb, kRayDeltaScale) = f2u(nr.delta_scale);
}

// weights_raygen_rays_kernel: the same for a ray list (vr_accumulate_weights_rays): the ray is list_ray()'s.
template <int FMA, int GW>
__global__ __launch_bounds__(kWave* GW) void weights_raygen_rays_kernel(const KParams p, const RayList rl) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    uint32_t id;
    Ray nr;
    float vdir[3];  // (nothing here reads it)
    const bool valid = list_ray<FMA, GW>(p, rl, lane, wave, id, nr, vdir) && nr.alive;
    const unsigned long long m_valid = __builtin_amdgcn_ballot_w64(valid);
    const uint32_t my_base = reserve_ray_slots<GW>(p, m_valid, lane, wave);
    if (!valid) return;
    store_march_words(ray_slot(p.ray_buf_rw, kWeightRayWords, my_base + lane_rank(m_valid)), nr);
}

// ---------------------------------------------------------------------------
// weights_kernel: the persistent march.  One wave per workgroup; a wave owns a chunk of consecutive ray
// ids (grab_chunk) and refills its idle lanes once refill_min of them wait; the sample guard is
// render_kernel's.  A lane's ray is alive while t < tmax (a stopped ray gets tmax = -1, a lane without a
// ray has t = 0, tmax = -1).
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
    using P = Policy<FMA>;
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
            uint32_t slot;
            if (N2) slot = (s1_node << 3) | (s1_leaf & 7u);
            else slot = s1_node * (uint32_t)p.N3 + s1_leaf % (uint32_t)p.N3;
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
        if (leaf != kNoLeaf) s1_node = (uint32_t)g_file[N2 ? (leaf >> 3) : leaf / (uint32_t)p.N3];
    };

    for (;;) {
        // ---- retire finished rays and hand their lanes new ones, in batches (as render_kernel) ----
        const bool done = active && !(t < tmax);
        const unsigned long long m_done = __builtin_amdgcn_ballot_w64(done);
        const unsigned long long m_busy = __builtin_amdgcn_ballot_w64(t < tmax);
        const int n_avail = kWave - __builtin_popcountll(m_busy);
        if (n_avail > 0 && (m_busy == 0ull || (!exhausted && n_avail >= p.refill_min))) {
            if (m_done != 0ull) progress_round = (uint32_t)__builtin_amdgcn_readfirstlane((int)rounds);
            if (!exhausted && chunk_next >= chunk_end) {
                uint32_t lo, hi;
                grab_chunk(p, lane, lo, hi);
                lo = __builtin_amdgcn_readfirstlane(lo);
                hi = __builtin_amdgcn_readfirstlane(hi);
                if (hi == lo) {
                    exhausted = true;
                } else {
                    chunk_next = lo;
                    chunk_end = hi;
                }
            }
            const bool vacant = !(t < tmax);
            bool take = false;
            if (!exhausted) {
                const uint32_t r = chunk_next + lane_rank(~m_busy);
                const uint32_t c_end = chunk_end;
                const uint32_t left = chunk_end - chunk_next;
                chunk_next += (uint32_t)n_avail < left ? (uint32_t)n_avail : left;
                if (vacant && r < c_end) {
                    take = true;
                    const uint32_t* rs = ray_slot(p.ray_buf, kWeightRayWords, r);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        cen[i] = u2f(ray_word(rs, kRayCen + i));
                        dir[i] = u2f(ray_word(rs, kRayDir + i));
                        invdir[i] = u2f(ray_word(rs, kRayInvDir + i));
                    }
                    t = u2f(ray_word(rs, kRayT));
                    tmax = u2f(ray_word(rs, kRayTmax));
                    delta_scale = u2f(ray_word(rs, kRayDeltaScale));
                }
            }
            if (vacant) {
                active = take;
                if (!take) {  // (no ray: not alive)
                    t = 0.f;
                    tmax = -1.f;
                }
                light = 1.f;
                cur = Cursor();
            }
        }
        if (!wave_any(active)) {
            if (exhausted) break;
            continue;
        }

        // ---- the sample guard, as render_kernel's: wave-uniform, once per pass through here ----
        if (rounds - progress_round >= (uint32_t)p.max_iter) {
            if (t < tmax) {
                t = tmax;
                if (p.status) atomicOr(p.status, 1u);
            }
            progress_round = rounds;
        }
        int m = 0;
        for (; m < p.march_max; ++m) {
            if (__builtin_amdgcn_ballot_w64(t < tmax) == 0ull) break;
            uint32_t hit_leaf = kNoLeaf, hit_bits = 0;
            if (t < tmax) {
                float pos[3];
                pos[0] = P::madd(t, dir[0], cen[0]);
                pos[1] = P::madd(t, dir[1], cen[1]);
                pos[2] = P::madd(t, dir[2], cen[2]);
                float cube_sz = 0.f;
                int levels;
                uint32_t word, leaf;
                if (N2) leaf = query_n2<false, (QUERY == kQueryN2Blocked ? 1 : 0)>(p, pos, &levels, &word, cur);
                else leaf = (uint32_t)query_generic<FMA, false>(p, pos, &cube_sz, &levels, &word);
                // rt_core.cuh:116: dda / cube_sz (N2: cube_sz = 2^levels, x / 2^k == ldexp(x, -k))
                const float dda = dda_unit<FMA>(pos, invdir);
                const float t_subcube = N2 ? __builtin_amdgcn_ldexpf(dda, -levels) : dda / cube_sz;
                const float delta_t = t_subcube + p.step_size;
                const float sigma = h2f((uint16_t)(word & 0xFFFFu));
                bool stop = false;
                if (sigma > p.sigma_thresh) {
                    // rt_core.cuh:118-121,174 (the argument is never NaN: render_kernel says why)
                    const float att = vr_expf_nonan(-delta_t * delta_scale * sigma);
                    const float weight = light * (1.f - att);
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
    if (rays && gen_waves >= 16)
        hipLaunchKernelGGL((weights_raygen_rays_kernel<FMA, 16>), dim3((unsigned)((total_blocks + 15) / 16)),
                           dim3(kWave * 16), 0, s, p, *rays);
    else if (rays)
        hipLaunchKernelGGL((weights_raygen_rays_kernel<FMA, 4>), dim3((unsigned)((total_blocks + 3) / 4)),
                           dim3(kWave * 4), 0, s, p, *rays);
    else if (gen_waves >= 16)
        hipLaunchKernelGGL((weights_raygen_kernel<FMA, 16>), dim3((unsigned)((total_blocks + 15) / 16)),
                           dim3(kWave * 16), 0, s, p);
    else
        hipLaunchKernelGGL((weights_raygen_kernel<FMA, 4>), dim3((unsigned)((total_blocks + 3) / 4)),
                           dim3(kWave * 4), 0, s, p);
    const dim3 grid(persistent_grid(total_blocks, n_cus, waves_override > 0 ? waves_override : 4 * kWeightWaves));
    const bool hits = w.hits != nullptr;
    const int query = !uses_lookup(p) ? kQueryGeneric : (p.brick_blocked ? kQueryN2Blocked : kQueryN2);
#define VR_WEIGHTS(Q)                                                              \
    do {                                                                           \
        if (hits) launch_march_check<FMA, Q, true>(p, w, check_first, grid, s);    \
        else launch_march_check<FMA, Q, false>(p, w, check_first, grid, s);        \
    } while (0)
    if (query == kQueryGeneric) VR_WEIGHTS(kQueryGeneric);
    else if (query == kQueryN2Blocked) VR_WEIGHTS(kQueryN2Blocked);
    else VR_WEIGHTS(kQueryN2);
#undef VR_WEIGHTS
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
