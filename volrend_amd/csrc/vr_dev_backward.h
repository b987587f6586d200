// vr_dev_backward.h -- backward_kernel: the persistent march that carries dL / d out[0..3] of every ray back through
// trace_ray's compositing (rt_core.cuh:66-196) to the density and the record entries of every leaf slot a hit sample
// fell into, and ADDS the contributions into grad_data, which is indexed as the file's data array is.  One kernel
// template for its two callers: vr_render_backward (vr_grad.hip), whose g = dL / d out comes from grad_accum, and
// vr_fit_rays (vr_fit.hip), whose march forms out[], the L2 loss head and g itself.  ARGS (GradArgs<MARK> / FitArgs)
// carries the kernel arguments and the compile-time kind (ARGS::kFit, ARGS::kMark); what differs between the kinds
// stands under `if constexpr` at the place where it differs, and vr_fit.hip says why it differs.
// Where a kind-dependent statement could be folded further (a loop over NS sums with NS = 1, one spelling of the
// restart test, one tail of the emitting branch) and is not, the spelling is the one that gives the compiler the
// input it had when each kind was a kernel of its own: all 108 flavours are byte for byte what they were
// (EXPERIMENTS.md "One backward kernel").
//
// The march is weights_kernel's (vr_weights.hip): ray generation (vr_dev_march.h), the point query, the step, the
// attenuation and the stop test are the device functions the colour kernels use, so which samples exist, their
// leaves, delta_t and where the ray stops have the bits trace_ray gives them in either FP model.  Those are
// constants of the differentiation; only sigma and the record entries are variables (include/volrend_hip.h has the
// formulas).  Built with -ffp-contract=off; see vr_device_math.h.
//
// Two marches per ray.  The sigma contribution of sample i needs R_i = sum_{j > i} w_j G_j, a SUFFIX sum, and
// the totals T_{K+1} and C^ = sum_j w_j G_j; a ray has any number of samples, so nothing per sample can be
// kept.  A lane therefore marches its ray twice, shading inline both times:
//   phase 0  the totals: light at the end, whether the ray stopped, the sum behind the first sample
//   phase 1  the same march again; `sum` starts at that sum and loses w_i G_i at every hit, which leaves R_i
// `sum` is binary64: total - prefix cancels, and in binary32 the error would be 2^-24 of the WHOLE sum
// however little is left behind sample i.  Every product is binary32; only this running sum is wider (one
// add per hit; fit: one per channel, S_ch = sum_j w_j c_{j,ch}, because g is not known in the first march).
// Segments.  Even in binary64 the subtraction's error is relative to the total, and the contribution it goes
// into is of the size of the light that reaches the sample.  So the emitting march stops trusting `sum`
// once a sample would take the light below 2^-20 of what its segment began with: that sample becomes the
// first of a new segment -- a totals march from there to the end of the ray (phase 0 again), then the
// emitting march from there.  The sum of a segment leaves its first sample OUT (that sample's R is the sum
// itself, no subtraction: it may be the one that swallows the light), kept in `head` for C^.  With
// stop_thresh at its default a ray ends long before 2^-20 and has one segment; only rays marched deep into
// opaque matter (stop_thresh = 0) pay for more, a tail's march per 20 bits of attenuation.
//
// The scatter.  A hit's contributions are one run of the slot's data_dim floats; the hits of a wave's 64
// lanes lie in 64 different leaves.  Float atomic adds execute at the memory side at a rate that is only
// reached when one wave instruction covers about 256 contiguous bytes (one lane per row is ~17x slower), so
// the wave scatters ONE HIT AT A TIME ACROSS ITS LANES: the lanes that own a hit of this march round push
// (slot, three channel factors, the sigma term, owner) into a per-wave LDS table, and then, hit by hit, lane
// e adds element e of that hit's run -- channel factor times the owner's basis value, read from a per-wave
// LDS table of basis values written at refill.  SH16: 49 lanes cover 196 contiguous bytes; SH25: two
// instructions of 64 + 11 elements; records shorter than half a wave (SH9: 28 floats, SH4: 13, RGBA and the
// single-coefficient case: 4) pack 2 / 4 / 16 hits into one instruction, each lane group a run of its own.
//
// For the .hip files only: the kernel and the host function that picks its flavour.
#pragma once
#include "vr_dev_march.h"
#include "vr_dev_shade.h"

namespace vr {

namespace {

// per SIMD (profiles/render_backward_kernel_resources.txt, profiles/fit_rays_kernel_resources.txt)
constexpr int kBackwardWaves = 4;

typedef __attribute__((address_space(1))) float vr_gfloat_t;
typedef __attribute__((address_space(1))) const float vr_gcfloat_t;
typedef __attribute__((address_space(1))) const int32_t vr_gcint_t;
typedef __attribute__((address_space(1))) uint32_t vr_guint_t;

template <int BASIS>
struct GradTraits {
    static constexpr bool kSh = BASIS > 1;                       // per-ray basis values in LDS
    static constexpr int kRun = kSh ? 3 * BASIS + 1 : 4;         // floats a hit adds
    static constexpr int kPack = kRun >= kWave ? 1 : kWave / kRun;  // hits per wave instruction
    static constexpr int kChunks = (kRun + kWave - 1) / kWave;   // wave instructions per hit
    static constexpr int kBasisRows = kSh ? BASIS : 1;
};

// ---------------------------------------------------------------------------
// backward_kernel: the persistent march (weights_kernel's frame: one wave per workgroup, chunks of ray ids,
// batched refill, the sample guard), two phases per ray and the wave-wide scatter described at the top.
// The frame is WRITTEN OUT here, in plain locals of the kernel, and not taken from vr_dev_march.h, which states
// the same steps for weights_kernel: over march_refill / sample_guard / march_sample this kernel held two more
// VGPRs and ran 0.2-0.4 % slower (EXPERIMENTS.md "One march frame").  A change to the refill rule, the guard or
// the queue protocol there is made here too.  Rays are GradRecord records: the view direction and the ray's row
// of the per-ray input (grad_accum; fit: target, sq_err, accum) follow the march words.
// The mark (the lanes that own an emitting hit also set the slot's bit of `touched`, one vector atomic OR per
// march round in front of the scatter's n_emit * kChunks adds) is a compile-time flavour of the backward calls --
// the unmarked kernels hold no trace of it -- and a wave-uniform run-time test on a kernel argument for fit.
// ---------------------------------------------------------------------------
template <int FMA, int QUERY, int BASIS, typename ARGS>
__global__ __launch_bounds__(kWave, kBackwardWaves) void backward_kernel(const KParams p, const ARGS gp) {
    using P = Policy<FMA>;
    using GT = GradTraits<BASIS>;
    constexpr bool N2 = QUERY != kQueryGeneric;
    constexpr bool FIT = ARGS::kFit;
    constexpr int NS = FIT ? 3 : 1;  // running sums: fit one per channel (of w c_ch), the backward one (of w G)
    __shared__ float s_basis[GT::kBasisRows * kWave];  // [b][lane]: basis value b of the lane's ray
    __shared__ uint32_t s_slot[kWave];                 // the hits of this round, compacted
    __shared__ float s_f[4][kWave];                    // channel factors 0..2, the sigma term
    __shared__ uint32_t s_own[kWave];

    const int lane = threadIdx.x & (kWave - 1);
    float cen[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f}, invdir[3] = {1.f, 1.f, 1.f};
    float t = 0.f, tmax = -1.f, delta_scale = 1.f, light = 1.f;
    float out[3] = {0.f, 0.f, 0.f};     // (fit) trace_ray's sums (the ray's first totals march)
    float g[4] = {0.f, 0.f, 0.f, 0.f};  // backward: loaded at refill; fit: known once the first totals march has ended
    double sum[NS] = {};      // phase 0: the segment's sum so far; phase 1: what is still to come behind this sample
    float head[NS] = {};      // the term of the segment's first sample (not in `sum`)
    float scale = 1.f, tail = 0.f;  // s, and g3 T_end (not stopped) or -s^2 T_end C^ (stopped): known after the first march
    float t_ck = 0.f, light_ck = 1.f;  // where the segment begins, and the light that reaches it
    uint32_t rid = 0;
    int phase = 0;            // 0 totals, 1 emitting
    bool any_hit = false, stopped = false, seg_first = true, have_tail = false;
    constexpr float kSegment = 0x1p-20f;
    bool active = false;      // the lane holds a ray (marching or finished)
    Cursor cur;
    uint32_t rounds = 0, progress_round = 0;
    bool exhausted = false;
    uint32_t chunk_next = 0, chunk_end = 0;
    vr_gfloat_t* const g_out = (vr_gfloat_t*)gp.grad_data;
    vr_gcint_t* const g_file = (vr_gcint_t*)gp.file_node;
    bool mark = ARGS::kMark;
    if constexpr (FIT) mark = gp.touched != nullptr;  // (wave-uniform: a kernel argument)
    // this lane's place in a scatter instruction: which of the kPack hits, which element of its run
    const int my_sub = GT::kPack > 1 ? lane / GT::kRun : 0;
    const int my_elem = GT::kPack > 1 ? lane - my_sub * GT::kRun : lane;

    for (;;) {
        {
            bool again;  // a segment whose sum is known starts over, emitting
            if constexpr (FIT) {
                const bool ended = active && !(t < tmax) && phase == 0;
                // ---- the ray's first totals march has ended, with or without a hit: out[], the loss head, g, the totals ----
                const bool first_end = ended && !have_tail;
                if (wave_any(first_end)) {
                    if (first_end) {
                        const uint32_t* rs = ray_slot(p.ray_buf, kGradRayWords, rid);
                        const float t_end = light;
                        float o[4];
                        scale = stopped ? 1.f / (1.f - t_end) : 1.f;  // (finish_ray's, rt_core.cuh:176-194)
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) o[ch] = stopped ? out[ch] * scale : out[ch];
                        o[3] = stopped ? 1.f : 1.f - t_end;
                        loss_head(gp, ray_word(rs, kGradRayPixel), o, g);  // (vr_fit.hip's, found through FitArgs)
                        const double c_sum = ((double)g[0] * (sum[0] + (double)head[0]) +
                                              (double)g[1] * (sum[1] + (double)head[1])) +
                                             (double)g[2] * (sum[2] + (double)head[2]);
                        const float c_hat = (float)c_sum;
                        tail = stopped ? -(scale * scale) * t_end * c_hat : g[3] * t_end;
                        have_tail = true;
                    }
                }
                again = ended && any_hit;
            } else {
                again = active && !(t < tmax) && phase == 0 && any_hit;
            }
            // ---- the restart ----
            if (wave_any(again)) {
                progress_round = (uint32_t)__builtin_amdgcn_readfirstlane((int)rounds);
                if (again) {
                    const uint32_t* rs = ray_slot(p.ray_buf, kGradRayWords, rid);
                    if constexpr (!FIT) {
                        if (!have_tail) {  // the ray's first march: its totals
                            const float t_end = light;
                            const float c_hat = (float)(sum[0] + (double)head[0]);
                            scale = stopped ? 1.f / (1.f - t_end) : 1.f;
                            tail = stopped ? -(scale * scale) * t_end * c_hat : g[3] * t_end;
                            have_tail = true;
                        }
                    }
                    t = t_ck;
                    tmax = u2f(ray_word(rs, kRayTmax));
                    light = light_ck;
                    cur = Cursor();
                    phase = 1;
                    seg_first = true;
                }
            }
        }
        // ---- retire finished rays and hand their lanes new ones, in batches (as weights_kernel) ----
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
                    rid = r;
                    const uint32_t* rs = ray_slot(p.ray_buf, kGradRayWords, r);
                    float vdir[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        cen[i] = u2f(ray_word(rs, kRayCen + i));
                        dir[i] = u2f(ray_word(rs, kRayDir + i));
                        invdir[i] = u2f(ray_word(rs, kRayInvDir + i));
                        vdir[i] = u2f(ray_word(rs, kGradRayVdir + i));
                    }
                    t = u2f(ray_word(rs, kRayT));
                    tmax = u2f(ray_word(rs, kRayTmax));
                    delta_scale = u2f(ray_word(rs, kRayDeltaScale));
                    if constexpr (!FIT) {
                        const vr_f4_t gv = ((const vr_gfloat4_t*)gp.grad_accum)[ray_word(rs, kGradRayPixel)];
                        g[0] = gv.x;
                        g[1] = gv.y;
                        g[2] = gv.z;
                        g[3] = gv.w;
                    }
                    if constexpr (GT::kSh) {
                        float b[VR_MAX_BASIS];
                        precalc_basis<FMA, false, BASIS>(p, vdir, b);
#pragma unroll
                        for (int i = 0; i < BASIS; ++i) s_basis[i * kWave + lane] = b[i];
                    }
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
                phase = 0;
                any_hit = false;
                stopped = false;
                if constexpr (!FIT) sum[0] = 0.0;  // (its head is read only behind a hit, which sets it)
                seg_first = true;
                have_tail = false;
                t_ck = t;
                light_ck = 1.f;
                if constexpr (FIT) {  // (the head too: the loss head runs for a ray without a hit)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        out[ch] = 0.f;
                        sum[ch] = 0.0;
                        head[ch] = 0.f;
                    }
                }
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
                any_hit = false;  // (a ray cut in a totals march emits nothing more; fit: its out[] is what it had summed)
                if (p.status) atomicOr(p.status, 1u);
            }
            progress_round = rounds;
        }
        int m = 0;
        for (; m < p.march_max; ++m) {
            if (__builtin_amdgcn_ballot_w64(t < tmax) == 0ull) break;
            bool emit = false;
            uint32_t e_slot = 0;
            float e_f[4] = {0.f, 0.f, 0.f, 0.f};
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
                const float dda = dda_unit<FMA>(pos, invdir);
                const float t_subcube = N2 ? __builtin_amdgcn_ldexpf(dda, -levels) : dda / cube_sz;
                const float delta_t = t_subcube + p.step_size;
                const float sigma = h2f((uint16_t)(word & 0xFFFFu));
                bool stop = false;
                if (sigma > p.sigma_thresh) {
                    // rt_core.cuh:118-121,174
                    const float att = vr_expf_nonan(-delta_t * delta_scale * sigma);
                    const float weight = light * (1.f - att);
                    // (emitting) a sample that swallows the light begins a segment of its own: sum first
                    if (phase == 1 && !seg_first && light * att < light_ck * kSegment) {
                        t_ck = t;
                        light_ck = light;
                        phase = 0;
                        seg_first = true;
                        if constexpr (FIT) sum[0] = sum[1] = sum[2] = 0.0;
                        else sum[0] = 0.0;
                    }
                    // the colour of the sample, rt_core.cuh:125-170; fit: the ray's first totals march also sums
                    // out[] with the colour kernels' operations in trace_ray's order
                    Record<BASIS> rec;
                    load_record<BASIS>(p, leaf, rec);
                    float c[3], dc[3];  // colour and d colour / d (what the record entry multiplies)
                    if constexpr (BASIS == BASIS_RGBA) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            c[ch] = rec.at(ch);
                            dc[ch] = 1.f;
                        }
                        if constexpr (FIT) {
                            if (!have_tail) {  // rt_core.cuh:161 as render_kernel's owner forms it
#pragma unroll
                                for (int ch = 0; ch < 3; ++ch) out[ch] = P::madd(c[ch], weight, out[ch]);
                            }
                        }
                    } else {
                        float u[3];
                        if constexpr (BASIS == BASIS_1) {
                            const float b0 = (float)0.28209479177387814;
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) u[ch] = b0 * rec.at(ch);
                        } else {
                            float b[VR_MAX_BASIS];
#pragma unroll
                            for (int i = 0; i < BASIS; ++i) b[i] = s_basis[i * kWave + lane];
                            u[0] = channel_dot<FMA, BASIS, 0>(b, rec);
                            u[1] = channel_dot<FMA, BASIS, 1>(b, rec);
                            u[2] = channel_dot<FMA, BASIS, 2>(b, rec);
                        }
                        if constexpr (FIT) {
                            if (!have_tail) {  // rt_core.cuh:161: weight / (1 + expf(-tmp)), added in sample order
#pragma unroll
                                for (int ch = 0; ch < 3; ++ch) out[ch] += weighted_sigmoid(weight, u[ch]);
                            }
                        }
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            c[ch] = sigmoid(u[ch]);
                            dc[ch] = c[ch] * (1.f - c[ch]);
                            if constexpr (BASIS == BASIS_1) dc[ch] *= (float)0.28209479177387814;
                        }
                    }
                    // the sample's terms of the running sums: w G (G = g . c), or per channel w c_ch (fit: g is not
                    // known in the ray's first march)
                    float G = 0.f, term[NS];  // (G: the backward's, here; fit forms G_i in the emitting branch)
                    if constexpr (FIT) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) term[ch] = weight * c[ch];
                    } else {
                        G = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];
                        term[0] = weight * G;
                    }
                    light *= att;  // (now T_{i+1})
                    if (phase == 0) {
                        if constexpr (FIT) {
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) {
                                if (seg_first) head[ch] = term[ch];
                                else sum[ch] += (double)term[ch];
                            }
                        } else {
                            if (seg_first) head[0] = term[0];
                            else sum[0] += (double)term[0];
                        }
                        any_hit = true;
                    } else {
                        if (!seg_first) {
                            if constexpr (FIT) {
#pragma unroll
                                for (int ch = 0; ch < 3; ++ch) sum[ch] -= (double)term[ch];
                            } else {
                                sum[0] -= (double)term[0];  // R_i
                            }
                        }
                        // what the hit adds: G_i and R_i per kind, then the slot, the three channel factors and
                        // the sigma term -- in both arms, each with its own declarations: as one tail behind the
                        // arms, twelve fit flavours were no longer the code they had been (EXPERIMENTS.md)
                        if constexpr (FIT) {
                            const float G_i = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];  // (g is known by now)
                            const float remain =  // R_i
                                (float)(((double)g[0] * sum[0] + (double)g[1] * sum[1]) + (double)g[2] * sum[2]);
                            const float delta = delta_t * delta_scale;
                            emit = true;
                            const uint32_t node = (uint32_t)g_file[N2 ? (leaf >> 3) : leaf / (uint32_t)p.N3];
                            e_slot = N2 ? ((node << 3) | (leaf & 7u)) : node * (uint32_t)p.N3 + leaf % (uint32_t)p.N3;
                            const float sw = scale * weight;
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) e_f[ch] = g[ch] * sw * dc[ch];
                            e_f[3] = delta * (scale * (light * G_i - remain) + tail);
                        } else {
                            const float G_i = G;
                            const float delta = delta_t * delta_scale;
                            emit = true;
                            const uint32_t node = (uint32_t)g_file[N2 ? (leaf >> 3) : leaf / (uint32_t)p.N3];
                            e_slot = N2 ? ((node << 3) | (leaf & 7u)) : node * (uint32_t)p.N3 + leaf % (uint32_t)p.N3;
                            const float sw = scale * weight;
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) e_f[ch] = g[ch] * sw * dc[ch];
                            e_f[3] = delta * (scale * (light * G_i - (float)sum[0]) + tail);  // (sum[0] is R_i)
                        }
                    }
                    seg_first = false;
                    stop = light < p.stop_thresh;
                }
                if (stop) {
                    tmax = -1.f;  // stopped (and no longer alive)
                    stopped = true;
                } else {
                    t += delta_t;
                }
            }
            // ---- the scatter: this round's hits, one (or kPack) per wave instruction ----
            const unsigned long long m_emit = __builtin_amdgcn_ballot_w64(emit);
            if (m_emit != 0ull) {
                const int n_emit = __builtin_popcountll(m_emit);
                if constexpr (ARGS::kMark) {
                    if (mark) {
                        // (result unused: the non-returning hardware OR; bits only ever get set, so no order matters)
                        if (emit)
                            __hip_atomic_fetch_or((vr_guint_t*)gp.touched + (e_slot >> 5), 1u << (e_slot & 31u),
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                if (emit) {
                    const uint32_t k = lane_rank(m_emit);
                    s_slot[k] = e_slot;
                    s_f[0][k] = e_f[0];
                    s_f[1][k] = e_f[1];
                    s_f[2][k] = e_f[2];
                    s_f[3][k] = e_f[3];
                    s_own[k] = (uint32_t)lane;
                }
                // (one wave: its LDS operations execute in order; the compiler must not reorder them)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (int base = 0; base < n_emit; base += GT::kPack) {
                    const int j = base + my_sub;
                    const bool mine = my_sub < GT::kPack && j < n_emit;
#pragma unroll
                    for (int ck = 0; ck < GT::kChunks; ++ck) {
                        const int e = my_elem + ck * kWave;
                        if (mine && e < GT::kRun) {
                            const uint32_t slot = s_slot[j];
                            int ch, off;
                            float bval = 1.f;
                            if constexpr (GT::kSh) {
                                ch = e / BASIS;  // (3 for the sigma element)
                                off = e;
                                if (ch < 3) bval = s_basis[(e - ch * BASIS) * kWave + (int)s_own[j]];
                            } else if constexpr (BASIS == BASIS_1) {
                                ch = e;
                                off = e * p.basis_dim;  // the first coefficient of each channel; sigma at 3 * basis_dim
                            } else {
                                ch = e;
                                off = e;
                            }
                            const float v = s_f[ch][j] * bval;
                            // (result unused: the non-returning hardware add)
                            __hip_atomic_fetch_add(g_out + ((size_t)slot * (uint32_t)p.data_dim + (uint32_t)off), v,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        rounds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(rounds + (uint32_t)m));
    }
}

// The march of a backward launch, behind its ray generation: the flavour of the tree's query kind and basis.
template <int FMA, typename ARGS>
hipError_t launch_backward_march(const KParams& p, const ARGS& args, int n_cus, int waves_override, hipStream_t s) {
    const dim3 grid(persistent_grid(p.n_wave_blocks * p.n_frames, n_cus,
                                    waves_override > 0 ? waves_override : 4 * kBackwardWaves));
    dispatch_query(query_kind(p), [&](auto query) {
        constexpr int Q = decltype(query)::value;
        switch (basis_flavour(p.format, p.basis_dim)) {
#define VR_BACKWARD(B) \
    case B: hipLaunchKernelGGL((backward_kernel<FMA, Q, B, ARGS>), grid, dim3(kWave), 0, s, p, args); break
            VR_BACKWARD(BASIS_RGBA);
            VR_BACKWARD(BASIS_1);
            VR_BACKWARD(BASIS_4);
            VR_BACKWARD(BASIS_9);
            VR_BACKWARD(BASIS_16);
            VR_BACKWARD(BASIS_25);
#undef VR_BACKWARD
        }
    });
    return hipGetLastError();
}

}  // namespace

}  // namespace vr
