// vr_fit.hip -- vr_fit_rays: the L2 loss of a ray batch against target colours and its gradient with respect to
// the tree's values, in one launch.  What vr_render_rays (accum) -> the caller's loss head -> vr_render_backward_rays_touched
// compute in three steps: this march forms trace_ray's out[] itself, then the loss head and g = dL / d out[0..3]
// (include/volrend_hip.h has the head's operations, one rounding each), and carries g back as grad_kernel
// (vr_grad.hip) does.  Ray generation, the records, the queues, the march, the segments and the scatter are the
// backward list's; read vr_grad.hip first -- this file says what differs.
//
// g is not known while the ray's first totals march runs, and G_i = g . c_i enters the sums grad_kernel keeps.
// So the sums are kept PER CHANNEL: S_ch = sum_j w_j c_{j,ch} (three binary64 running sums where grad_kernel has
// one, the first sample of the segment apart in head_ch as there), and with g known
//   R_i = sum_ch g_ch S_ch(what is left behind sample i),   C^ = sum_ch g_ch (S_ch + head_ch)
// -- no third march.  The ray's first totals march also accumulates out[0..2] in binary32 with the colour
// kernels' operations in trace_ray's order (SH: out += weight / (1 + exp(-u)); RGBA: madd(colour, weight, out)),
// which is what makes `accum` the bits of vr_render_rays; at its end the lane forms out[], the head and g, and
// stores sq_err / accum.  Later segments (the kSegment restart) sum their S_ch again; only the first march
// (!have_tail) touches out[].
// A ray that never enters the volume has out[] = 0 and nothing to add: ray generation stores its sq_err / accum
// (fit_raygen_kernel below) and drops it, as the backward list's drops it.
// `touched`, `sq_err` and `accum` are optional at run time: wave-uniform tests on kernel arguments, one set of
// flavours.  Built with -ffp-contract=off, which the head relies on.
#include "vr_dev_march.h"
#include "vr_dev_shade.h"

namespace vr {

namespace {

constexpr int kFitWaves = 4;  // per SIMD, as grad_kernel (profiles/fit_rays_kernel_resources.txt)

typedef __attribute__((address_space(1))) float vr_gfloat_t;
typedef __attribute__((address_space(1))) const float vr_gcfloat_t;
typedef __attribute__((address_space(1))) const int32_t vr_gcint_t;
typedef __attribute__((address_space(1))) uint32_t vr_guint_t;

template <int BASIS>
struct FitTraits {  // (GradTraits of vr_grad.hip: the scatter is the same)
    static constexpr bool kSh = BASIS > 1;
    static constexpr int kRun = kSh ? 3 * BASIS + 1 : 4;
    static constexpr int kPack = kRun >= kWave ? 1 : kWave / kRun;
    static constexpr int kChunks = (kRun + kWave - 1) / kWave;
    static constexpr int kBasisRows = kSh ? BASIS : 1;
};

// The loss head of ray i (include/volrend_hip.h, vr_fit_rays): uncontracted binary32, one rounding per operator.
// Stores sq_err / accum where wanted and leaves dL / d out[0..3] in g.
__device__ __forceinline__ void loss_head(const FitParams& fp, uint32_t i, const float* out, float* g) {
    vr_gcfloat_t* const tg = (vr_gcfloat_t*)fp.target + (size_t)i * 3u;
    const float na = 1.f - out[3];
    float r[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float pred = out[ch] + fp.bg * na;
        r[ch] = pred - tg[ch];
    }
    if (fp.sq_err) ((vr_gfloat_t*)fp.sq_err)[i] = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    if (fp.accum) ((vr_gfloat4_t*)fp.accum)[i] = (vr_f4_t){out[0], out[1], out[2], out[3]};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) g[ch] = fp.grad_scale * r[ch];
    g[3] = -(fp.bg * ((g[0] + g[1]) + g[2]));
}

// march_raygen_rays_kernel<GradRecord> (vr_dev_march.h) that also answers for the rays it drops: a ray of the
// list that does not enter the volume has out[] = 0 (what raygen_rays_kernel composites for it).
template <int FMA, int GW>
__global__ __launch_bounds__(kWave* GW) void fit_raygen_kernel(const KParams p, const RayList rl, const FitParams fp) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    uint32_t id;
    Ray nr;
    float vdir[3] = {0.f, 0.f, 0.f};
    const bool has = list_ray<FMA, GW>(p, rl, lane, wave, id, nr, vdir);
    const bool valid = has && nr.alive;
    if (has && !valid) {
        const float out[4] = {0.f, 0.f, 0.f, 0.f};
        float g[4];
        loss_head(fp, id, out, g);
    }
    store_march_record<GW, GradRecord>(p, valid, lane, wave, nr, vdir, id);
}

// ---------------------------------------------------------------------------
// fit_kernel: grad_kernel's frame, phases, segments and scatter (written out, as there), with the per-channel
// sums, out[] and the loss head described at the top.  A change to the refill rule, the guard or the queue
// protocol in vr_dev_march.h / grad_kernel is made here too.
// ---------------------------------------------------------------------------
template <int FMA, int QUERY, int BASIS>
__global__ __launch_bounds__(kWave, kFitWaves) void fit_kernel(const KParams p, const FitParams fp) {
    using P = Policy<FMA>;
    using GT = FitTraits<BASIS>;
    constexpr bool N2 = QUERY != kQueryGeneric;
    __shared__ float s_basis[GT::kBasisRows * kWave];  // [b][lane]: basis value b of the lane's ray
    __shared__ uint32_t s_slot[kWave];                 // the hits of this round, compacted
    __shared__ float s_f[4][kWave];                    // channel factors 0..2, the sigma term
    __shared__ uint32_t s_own[kWave];

    const int lane = threadIdx.x & (kWave - 1);
    float cen[3] = {0.f, 0.f, 0.f}, dir[3] = {0.f, 0.f, 0.f}, invdir[3] = {1.f, 1.f, 1.f};
    float t = 0.f, tmax = -1.f, delta_scale = 1.f, light = 1.f;
    float out[3] = {0.f, 0.f, 0.f};  // trace_ray's sums (the ray's first totals march)
    float g[4] = {0.f, 0.f, 0.f, 0.f};  // known once that march has ended
    double sum[3] = {0.0, 0.0, 0.0};  // S_ch; phase 0: the segment's sums so far; phase 1: what is still to come
    float head[3] = {0.f, 0.f, 0.f};  // w c_ch of the segment's first sample (not in `sum`)
    float scale = 1.f, tail = 0.f;
    float t_ck = 0.f, light_ck = 1.f;
    uint32_t rid = 0;
    int phase = 0;            // 0 totals, 1 emitting
    bool any_hit = false, stopped = false, seg_first = true, have_tail = false;
    constexpr float kSegment = 0x1p-20f;
    bool active = false;
    Cursor cur;
    uint32_t rounds = 0, progress_round = 0;
    bool exhausted = false;
    uint32_t chunk_next = 0, chunk_end = 0;
    vr_gfloat_t* const g_out = (vr_gfloat_t*)fp.grad_data;
    vr_gcint_t* const g_file = (vr_gcint_t*)fp.file_node;
    const bool mark = fp.touched != nullptr;  // (wave-uniform: a kernel argument)
    const int my_sub = GT::kPack > 1 ? lane / GT::kRun : 0;
    const int my_elem = GT::kPack > 1 ? lane - my_sub * GT::kRun : lane;

    for (;;) {
        {
            const bool ended = active && !(t < tmax) && phase == 0;
            // ---- the ray's first totals march has ended: out[], the loss head, g, the totals ----
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
                    loss_head(fp, ray_word(rs, kGradRayPixel), o, g);
                    const double c_sum = ((double)g[0] * (sum[0] + (double)head[0]) +
                                          (double)g[1] * (sum[1] + (double)head[1])) +
                                         (double)g[2] * (sum[2] + (double)head[2]);
                    const float c_hat = (float)c_sum;
                    tail = stopped ? -(scale * scale) * t_end * c_hat : g[3] * t_end;
                    have_tail = true;
                }
            }
            // ---- a segment whose sums are known starts over, emitting ----
            const bool again = ended && any_hit;
            if (wave_any(again)) {
                progress_round = (uint32_t)__builtin_amdgcn_readfirstlane((int)rounds);
                if (again) {
                    const uint32_t* rs = ray_slot(p.ray_buf, kGradRayWords, rid);
                    t = t_ck;
                    tmax = u2f(ray_word(rs, kRayTmax));
                    light = light_ck;
                    cur = Cursor();
                    phase = 1;
                    seg_first = true;
                }
            }
        }
        // ---- retire finished rays and hand their lanes new ones, in batches (as grad_kernel) ----
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
                seg_first = true;
                have_tail = false;
                t_ck = t;
                light_ck = 1.f;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    out[ch] = 0.f;
                    sum[ch] = 0.0;
                    head[ch] = 0.f;
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
                any_hit = false;  // (a ray cut in a totals march emits nothing more; its out[] is what it had summed)
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
                        sum[0] = sum[1] = sum[2] = 0.0;
                    }
                    // the colour of the sample, rt_core.cuh:125-170
                    Record<BASIS> rec;
                    load_record<BASIS>(p, leaf, rec);
                    float c[3], dc[3];  // colour and d colour / d (what the record entry multiplies)
                    if constexpr (BASIS == BASIS_RGBA) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            c[ch] = rec.at(ch);
                            dc[ch] = 1.f;
                        }
                        if (!have_tail) {  // rt_core.cuh:161 as render_kernel's owner forms it
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) out[ch] = P::madd(c[ch], weight, out[ch]);
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
                        if (!have_tail) {  // rt_core.cuh:161: weight / (1 + expf(-tmp)), added in sample order
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) out[ch] += weighted_sigmoid(weight, u[ch]);
                        }
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            c[ch] = sigmoid(u[ch]);
                            dc[ch] = c[ch] * (1.f - c[ch]);
                            if constexpr (BASIS == BASIS_1) dc[ch] *= (float)0.28209479177387814;
                        }
                    }
                    float wc[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) wc[ch] = weight * c[ch];
                    light *= att;  // (now T_{i+1})
                    if (phase == 0) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            if (seg_first) head[ch] = wc[ch];
                            else sum[ch] += (double)wc[ch];
                        }
                        any_hit = true;
                    } else {
                        if (!seg_first) {
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) sum[ch] -= (double)wc[ch];
                        }
                        const float G = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];
                        const float remain =
                            (float)(((double)g[0] * sum[0] + (double)g[1] * sum[1]) + (double)g[2] * sum[2]);  // R_i
                        const float delta = delta_t * delta_scale;
                        emit = true;
                        const uint32_t node = (uint32_t)g_file[N2 ? (leaf >> 3) : leaf / (uint32_t)p.N3];
                        e_slot = N2 ? ((node << 3) | (leaf & 7u)) : node * (uint32_t)p.N3 + leaf % (uint32_t)p.N3;
                        const float sw = scale * weight;
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) e_f[ch] = g[ch] * sw * dc[ch];
                        e_f[3] = delta * (scale * (light * G - remain) + tail);
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
            // ---- the scatter: this round's hits, one (or kPack) per wave instruction (grad_kernel's) ----
            const unsigned long long m_emit = __builtin_amdgcn_ballot_w64(emit);
            if (m_emit != 0ull) {
                const int n_emit = __builtin_popcountll(m_emit);
                if (mark) {
                    // (result unused: the non-returning hardware OR; bits only ever get set, so no order matters)
                    if (emit)
                        __hip_atomic_fetch_or((vr_guint_t*)fp.touched + (e_slot >> 5), 1u << (e_slot & 31u),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

template <int FMA, int QUERY>
void launch_fit_basis(const KParams& p, const FitParams& fp, dim3 grid, hipStream_t s) {
    switch (basis_flavour(p.format, p.basis_dim)) {
#define VR_FIT(B) \
    case B: hipLaunchKernelGGL((fit_kernel<FMA, QUERY, B>), grid, dim3(kWave), 0, s, p, fp); break
        VR_FIT(BASIS_RGBA);
        VR_FIT(BASIS_1);
        VR_FIT(BASIS_4);
        VR_FIT(BASIS_9);
        VR_FIT(BASIS_16);
        VR_FIT(BASIS_25);
#undef VR_FIT
    }
}

template <int FMA>
hipError_t launch_fp(const KParams& p, const FitParams& fp, int n_cus, int waves_override, int gen_waves, hipStream_t s,
                     const RayList& rays) {
    const int64_t total_blocks = p.n_wave_blocks * p.n_frames;
    {  // ray generation in workgroups of 16 or 4 waves, as launch_march_raygen
        const int gw = gen_waves >= 16 ? 16 : 4;
        const dim3 grid((unsigned)((total_blocks + gw - 1) / gw)), block(kWave * gw);
        if (gw == 16) hipLaunchKernelGGL((fit_raygen_kernel<FMA, 16>), grid, block, 0, s, p, rays, fp);
        else hipLaunchKernelGGL((fit_raygen_kernel<FMA, 4>), grid, block, 0, s, p, rays, fp);
    }
    const dim3 grid(persistent_grid(total_blocks, n_cus, waves_override > 0 ? waves_override : 4 * kFitWaves));
    const int query = query_kind(p);
    if (query == kQueryGeneric) launch_fit_basis<FMA, kQueryGeneric>(p, fp, grid, s);
    else if (query == kQueryN2Blocked) launch_fit_basis<FMA, kQueryN2Blocked>(p, fp, grid, s);
    else launch_fit_basis<FMA, kQueryN2>(p, fp, grid, s);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fit(const KParams& p, const FitParams& fp, int fp_mode, int n_cus, int waves_override, int gen_waves,
                      hipStream_t stream, const RayList* rays) {
    if (p.n_wave_blocks <= 0 || p.n_frames <= 0 || !rays) return hipSuccess;
    return fp_mode == VR_FP_FMA ? launch_fp<1>(p, fp, n_cus, waves_override, gen_waves, stream, *rays)
                                : launch_fp<0>(p, fp, n_cus, waves_override, gen_waves, stream, *rays);
}

}  // namespace vr
