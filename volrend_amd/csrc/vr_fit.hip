// vr_fit.hip -- vr_fit_rays: the L2 loss of a ray batch against target colours and its gradient with respect to
// the tree's values, in one launch.  What vr_render_rays (accum) -> the caller's loss head -> vr_render_backward_rays_touched
// compute in three steps: the march forms trace_ray's out[] itself, then the loss head and g = dL / d out[0..3]
// (include/volrend_hip.h has the head's operations, one rounding each), and carries g back as vr_render_backward
// does.  The march is backward_kernel (vr_dev_backward.h) in its fit kind: ray generation's records, the queues, the
// march, the segments and the scatter are the backward list's; read that header first -- this file says what the
// fit kind does differently, and has what is fit's own: the head, its ray generation, its kernel arguments, its launch.
//
// g is not known while the ray's first totals march runs, and G_i = g . c_i enters the sum the backward keeps.
// So the sums are kept PER CHANNEL: S_ch = sum_j w_j c_{j,ch} (three binary64 running sums where the backward has
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
#include "vr_dev_backward.h"

namespace vr {

namespace {

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

// What backward_kernel takes in its fit kind: FitParams as it is, field for field; the kernel finds loss_head()
// through this type.  `touched` is optional at run time (kMark: the kernel holds the OR, behind a wave-uniform test).
struct FitArgs : FitParams {
    static constexpr bool kFit = true, kMark = true;
    explicit FitArgs(const FitParams& f) : FitParams(f) {}
};

template <int FMA>
hipError_t launch_fp(const KParams& p, const FitParams& fp, int n_cus, int waves_override, int gen_waves, hipStream_t s,
                     const RayList& rays) {
    launch_raygen_waves(p, gen_waves, [&](auto gw, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((fit_raygen_kernel<FMA, decltype(gw)::value>), grid, block, 0, s, p, rays, fp);
    });
    return launch_backward_march<FMA>(p, FitArgs(fp), n_cus, waves_override, s);
}

}  // namespace

hipError_t launch_fit(const KParams& p, const FitParams& fp, int fp_mode, int n_cus, int waves_override, int gen_waves,
                      hipStream_t stream, const RayList* rays) {
    if (p.n_wave_blocks <= 0 || p.n_frames <= 0 || !rays) return hipSuccess;
    return fp_mode == VR_FP_FMA ? launch_fp<1>(p, fp, n_cus, waves_override, gen_waves, stream, *rays)
                                : launch_fp<0>(p, fp, n_cus, waves_override, gen_waves, stream, *rays);
}

}  // namespace vr
