// vr_dev_march.h -- the guided march frame: render_kernel's march phase (vr_render.hip) without records, as the
// consumers that need no colour pipeline run it -- weights_kernel (vr_weights.hip); backward_kernel
// (vr_dev_backward.h, the one march of vr_grad.hip and vr_fit.hip) takes its ray generation and query kind from here
// and keeps one written-out copy of the loop, which measured faster.
// One wave per workgroup; a wave owns a chunk of consecutive ray ids (grab_chunk) and refills its idle lanes once
// refill_min of them wait.  A lane's ray is alive while t < tmax (a stopped ray gets tmax = -1, a lane without a
// ray has t = 0, tmax = -1).  Stated once here: the query kind, retire and refill, the sample guard, the sample
// step, file-order addressing of a leaf slot, and ray generation for records that begin with the 12 march words.
// The point query, the step, the attenuation and the stop test are the device functions the colour kernels use,
// so a sample's leaf, delta_t and weight have the bits trace_ray (rt_core.cuh:66-196) gives them.
// The state stays in plain locals of the kernel: the per-lane part is handed in by reference, the wave-uniform
// part goes in and comes back by value (MarchFeed).  Other forms cost ten VGPRs (EXPERIMENTS.md "One march frame").
// For the .hip files only: device functions and kernels, and the host functions that pick among them
// (query_kind / dispatch_query, launch_raygen_waves / launch_march_raygen).
#pragma once
#include <type_traits>
#include "vr_device_math.h"
#include "vr_internal.h"
#include "vr_dev_layout.h"
#include "vr_dev_query.h"
#include "vr_dev_rays.h"

namespace vr {

namespace {

// How a flavour finds the leaf: the lookup with x-major or blocked bricks (N == 2), or the literal descent.
enum { kQueryN2 = 0, kQueryN2Blocked = 1, kQueryGeneric = 2 };
inline int query_kind(const KParams& p) {
    return !uses_lookup(p) ? kQueryGeneric : (p.brick_blocked ? kQueryN2Blocked : kQueryN2);
}
// f(std::integral_constant<int, the kind>): what a launcher instantiates its kernels over.
template <typename F>
void dispatch_query(int query, F&& f) {
    if (query == kQueryGeneric) f(std::integral_constant<int, kQueryGeneric>());
    else if (query == kQueryN2Blocked) f(std::integral_constant<int, kQueryN2Blocked>());
    else f(std::integral_constant<int, kQueryN2>());
}

// ---------------------------------------------------------------------------
// Ray generation.  A record is the 12 march words (kRayCen .. kRayDeltaScale) and, for a consumer that shades,
// the view direction and the ray's row of the per-pixel input behind them.
// ---------------------------------------------------------------------------
struct WeightRecord {
    static constexpr int kWords = kWeightRayWords;
    static constexpr bool kShade = false;
};
struct GradRecord {
    static constexpr int kWords = kGradRayWords;
    static constexpr bool kShade = true;  // kGradRayVdir, kGradRayPixel
};

// Every lane of the workgroup calls: compacts the rays that enter the volume into their queue's region of the
// ray buffer (reserve_ray_slots, as raygen_kernel does) and writes this lane's record.
template <int GW, typename Record>
__device__ __forceinline__ void store_march_record(const KParams& p, bool valid, int lane, int wave, const Ray& nr,
                                                   const float* vdir, uint32_t pixel) {
    const unsigned long long m_valid = __builtin_amdgcn_ballot_w64(valid);
    const uint32_t my_base = reserve_ray_slots<GW>(p, m_valid, lane, wave);
    if (!valid) return;
    uint32_t* rb = ray_slot(p.ray_buf_rw, Record::kWords, my_base + lane_rank(m_valid));
    store_march_words(rb, nr);
    if constexpr (Record::kShade) {
#pragma unroll
        for (int i = 0; i < 3; ++i) ray_word(rb, kGradRayVdir + i) = f2u(vdir[i]);
        ray_word(rb, kGradRayPixel) = pixel;
    }
}

// march_raygen_kernel: one lane per pixel of every frame.  setup_ray as raygen_kernel runs it (the frame is
// offscreen: tmax comes from render_bbox alone); a ray that misses the box is dropped -- there is no pixel to
// composite.  A shading record's pixel is its index into [n_frames][height][width].
template <int FMA, int GW, typename Record>
__global__ __launch_bounds__(kWave* GW) void march_raygen_kernel(const KParams p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const uint32_t id = (uint32_t)(((int64_t)blockIdx.x * GW + wave) * kWave + lane);
    bool valid = false;
    Ray nr;
    nr.alive = false;
    float vdir[3] = {0.f, 0.f, 0.f};
    uint32_t pixel = 0;
    if (id < p.total_rays) {
        const PixelRef r = locate(p, id);
        if (r.in_image) {
            setup_ray<FMA>(p, r, nr, vdir);
            valid = nr.alive;
            // (< 2^30: launch_geometry)
            pixel = ((uint32_t)r.frame * (uint32_t)p.height + (uint32_t)r.y) * (uint32_t)p.width + (uint32_t)r.x;
        }
    }
    store_march_record<GW, Record>(p, valid, lane, wave, nr, vdir, pixel);
}

// march_raygen_rays_kernel: the same for a ray list (vr_internal.h RayList): the ray is list_ray()'s, and its row
// of the per-pixel input is its index in the list.
template <int FMA, int GW, typename Record>
__global__ __launch_bounds__(kWave* GW) void march_raygen_rays_kernel(const KParams p, const RayList rl) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    uint32_t id;
    Ray nr;
    float vdir[3] = {0.f, 0.f, 0.f};
    const bool valid = list_ray<FMA, GW>(p, rl, lane, wave, id, nr, vdir) && nr.alive;
    store_march_record<GW, Record>(p, valid, lane, wave, nr, vdir, id);
}

// Ray generation of a march launch runs in workgroups of 16 or 4 waves (gen_waves: vr_launch.cpp raygen_waves), one
// wave per block of 64 ray ids: launch(std::integral_constant<int, GW>, grid, block) starts the kernel of that GW.
template <typename Launch>
void launch_raygen_waves(const KParams& p, int gen_waves, Launch&& launch) {
    const int gw = gen_waves >= 16 ? 16 : 4;
    const dim3 grid((unsigned)((p.n_wave_blocks * p.n_frames + gw - 1) / gw)), block(kWave * gw);
    if (gw == 16) launch(std::integral_constant<int, 16>(), grid, block);
    else launch(std::integral_constant<int, 4>(), grid, block);
}
// Records of `Record`, over the pixels of the frame table or over `rays`.
template <int FMA, typename Record>
void launch_march_raygen(const KParams& p, int gen_waves, hipStream_t s, const RayList* rays) {
    launch_raygen_waves(p, gen_waves, [&](auto gw, dim3 grid, dim3 block) {
        constexpr int GW = decltype(gw)::value;
        if (rays) hipLaunchKernelGGL((march_raygen_rays_kernel<FMA, GW, Record>), grid, block, 0, s, p, *rays);
        else hipLaunchKernelGGL((march_raygen_kernel<FMA, GW, Record>), grid, block, 0, s, p);
    });
}

// ---------------------------------------------------------------------------
// Retire and refill, in batches (as render_kernel): once per pass of the kernel's for(;;), in front of
//     if (!wave_any(active)) { if (exhausted) break; continue; }
// Finished rays leave their lanes; when no lane marches, or refill_min lanes wait and ids are left, the vacant
// lanes take the next ids of the wave's chunk (a new chunk when it is used up; `exhausted` once there is none).
// A taken ray's 12 march words are loaded here; load(rs, r) reads what follows them in record r (rs = its
// ray_slot of ray_words words).  reset() runs for every lane that was vacant, with or without a new ray, after
// t / tmax / light / cur are set: the caller's per-ray state starts over.
// The wave-uniform part of the state is passed in and returned as a MarchFeed; the kernel copies the result
// back into its locals (by reference, or kept as a struct in the kernel, the same code needs ten VGPRs more).
// ---------------------------------------------------------------------------
struct MarchFeed {
    bool exhausted;                  // no ids are left for this wave
    uint32_t chunk_next, chunk_end;  // the ids of its chunk not yet handed to a lane
    uint32_t progress_round;         // the round in which a ray last retired (sample_guard)
};
template <typename Load, typename Reset>
__device__ __forceinline__ MarchFeed march_refill(const KParams& p, int lane, int ray_words, uint32_t rounds,
                                                  MarchFeed feed, bool& active, float* cen, float* dir, float* invdir,
                                                  float& t, float& tmax, float& delta_scale, float& light, Cursor& cur,
                                                  Load&& load, Reset&& reset) {
    const bool done = active && !(t < tmax);
    const unsigned long long m_done = __builtin_amdgcn_ballot_w64(done);
    const unsigned long long m_busy = __builtin_amdgcn_ballot_w64(t < tmax);
    const int n_avail = kWave - __builtin_popcountll(m_busy);
    if (!(n_avail > 0 && (m_busy == 0ull || (!feed.exhausted && n_avail >= p.refill_min)))) return feed;
    if (m_done != 0ull) feed.progress_round = (uint32_t)__builtin_amdgcn_readfirstlane((int)rounds);
    if (!feed.exhausted && feed.chunk_next >= feed.chunk_end) {
        uint32_t lo, hi;
        grab_chunk(p, lane, lo, hi);
        lo = __builtin_amdgcn_readfirstlane(lo);
        hi = __builtin_amdgcn_readfirstlane(hi);
        if (hi == lo) {
            feed.exhausted = true;
        } else {
            feed.chunk_next = lo;
            feed.chunk_end = hi;
        }
    }
    const bool vacant = !(t < tmax);
    bool take = false;
    if (!feed.exhausted) {
        const uint32_t r = feed.chunk_next + lane_rank(~m_busy);
        const uint32_t c_end = feed.chunk_end;
        const uint32_t left = feed.chunk_end - feed.chunk_next;
        feed.chunk_next += (uint32_t)n_avail < left ? (uint32_t)n_avail : left;
        if (vacant && r < c_end) {
            take = true;
            const uint32_t* rs = ray_slot(p.ray_buf, ray_words, r);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                cen[i] = u2f(ray_word(rs, kRayCen + i));
                dir[i] = u2f(ray_word(rs, kRayDir + i));
                invdir[i] = u2f(ray_word(rs, kRayInvDir + i));
            }
            t = u2f(ray_word(rs, kRayT));
            tmax = u2f(ray_word(rs, kRayTmax));
            delta_scale = u2f(ray_word(rs, kRayDeltaScale));
            load(rs, r);
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
        reset();
    }
    return feed;
}

// The sample guard, as render_kernel's: wave-uniform, once per pass through the kernel's for(;;).  A wave that
// marched max_iter rounds without retiring a ray cuts the rays it holds (status bit 0) and counts anew.
// Returns whether this lane's ray was cut.
__device__ __forceinline__ bool sample_guard(const KParams& p, uint32_t rounds, uint32_t& progress_round, float& t,
                                             float tmax) {
    if (rounds - progress_round < (uint32_t)p.max_iter) return false;
    progress_round = rounds;
    if (!(t < tmax)) return false;
    t = tmax;
    if (p.status) atomicOr(p.status, 1u);
    return true;
}

// The sample at t: its leaf (a device leaf id), the step to the next sample and the density.
template <int FMA, int QUERY>
__device__ __forceinline__ uint32_t march_sample(const KParams& p, float t, const float* cen, const float* dir,
                                                 const float* invdir, Cursor& cur, float& delta_t, float& sigma) {
    using P = Policy<FMA>;
    constexpr bool N2 = QUERY != kQueryGeneric;
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
    delta_t = t_subcube + p.step_size;
    sigma = h2f((uint16_t)(word & 0xFFFFu));
    return leaf;
}

// The lead-in march of ray generation (vr_internal.h "Lead-in march"; every lane of the wave calls): the lanes
// whose ray is alive take march_sample's samples in lockstep while they are no hits -- what a march round does to
// such a ray is t += delta_t and nothing else.  A lane stops WITHOUT advancing t at its first sample with
// sigma > sigma_thresh (the march kernel takes that sample again, from the same t: the same bits), and stops as not
// alive once t >= tmax.  The wave stops when fewer than head.min_lanes (>= 1) lanes march or after head.max_rounds
// rounds; a ray that still marches then keeps the t it has.  The cursor is a cache and is dropped.
// Returns the samples the wave marched (wave-uniform).
template <int FMA, int QUERY>
__device__ __forceinline__ uint32_t head_march(const KParams& p, const HeadParams& head, Ray& nr) {
    Cursor cur;
    bool go = nr.alive;
    uint32_t samples = 0;
    for (int r = 0; r < head.max_rounds; ++r) {
        const unsigned long long m_go = __builtin_amdgcn_ballot_w64(go);
        if (__builtin_popcountll(m_go) < head.min_lanes) break;
        bool stepped = false;
        if (go) {
            float delta_t, sigma;
            march_sample<FMA, QUERY>(p, nr.t, nr.cen, nr.dir, nr.invdir, cur, delta_t, sigma);
            if (sigma > p.sigma_thresh) {
                go = false;
            } else {
                nr.t += delta_t;
                stepped = true;
                if (!(nr.t < nr.tmax)) go = nr.alive = false;
            }
        }
        samples += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(stepped));
    }
    return samples;
}

// A hit sample's compositing weight, and through `att` what it leaves of the light: rt_core.cuh:118-121,174
// (the argument is never NaN: render_kernel says why).  `light *= att` is the caller's.
__device__ __forceinline__ float sample_weight(float light, float delta_t, float delta_scale, float sigma, float& att) {
    att = vr_expf_nonan(-delta_t * delta_scale * sigma);
    return light * (1.f - att);
}

// A device leaf id in the FILE's node numbering (VrTreeDesc.child / data): file_node[file_node_index(leaf)] is
// the leaf's node there, file_slot() its slot of that node.
template <bool N2>
__device__ __forceinline__ uint32_t file_node_index(const KParams& p, uint32_t leaf) {
    return N2 ? (leaf >> 3) : leaf / (uint32_t)p.N3;
}
template <bool N2>
__device__ __forceinline__ uint32_t file_slot(const KParams& p, uint32_t node, uint32_t leaf) {
    return N2 ? ((node << 3) | (leaf & 7u)) : node * (uint32_t)p.N3 + leaf % (uint32_t)p.N3;
}

}  // namespace

}  // namespace vr
