// vr_grad.hip -- vr_render_backward: the derivative of a rendered batch with respect to the tree's values.
// For every pixel, dL/d out[0..3] (grad_accum) is carried back through trace_ray's compositing
// (rt_core.cuh:66-196) to the density and the record entries of every leaf slot a hit sample fell into, and
// the contributions are ADDED into grad_data, which is indexed as the file's data array is.
// The march is backward_kernel (vr_dev_backward.h: the mathematics, the two marches per ray, segments and the
// scatter are described there) in its kind that loads g = dL / d out from grad_accum at refill; this file has that
// kind's kernel arguments and the launch.
#include "vr_dev_backward.h"

namespace vr {

namespace {

// What a backward_kernel flavour takes of GradParams: the unmarked kernels the three pointers they always took (their
// kernel arguments, and with them their code, are what they were before the marked calls existed).
// MARK: the flavour of the marked calls (vr_render_backward_touched).
template <bool MARK>
struct GradArgs {
    static constexpr bool kFit = false, kMark = false;
    const float* grad_accum;
    float* grad_data;
    const int32_t* file_node;
    explicit GradArgs(const GradParams& g) : grad_accum(g.grad_accum), grad_data(g.grad_data), file_node(g.file_node) {}
};
template <>
struct GradArgs<true> : GradArgs<false> {
    static constexpr bool kMark = true;
    uint32_t* touched;
    explicit GradArgs(const GradParams& g) : GradArgs<false>(g), touched(g.touched) {}
};

template <int FMA>
hipError_t launch_fp(const KParams& p, const GradParams& gp, int n_cus, int waves_override, int gen_waves,
                     hipStream_t s, const RayList* rays) {
    launch_march_raygen<FMA, GradRecord>(p, gen_waves, s, rays);
    if (gp.touched) return launch_backward_march<FMA>(p, GradArgs<true>(gp), n_cus, waves_override, s);
    return launch_backward_march<FMA>(p, GradArgs<false>(gp), n_cus, waves_override, s);
}

}  // namespace

hipError_t launch_grad(const KParams& p, const GradParams& gp, int fp_mode, int n_cus, int waves_override,
                       int gen_waves, hipStream_t stream, const RayList* rays) {
    if (p.n_wave_blocks <= 0 || p.n_frames <= 0) return hipSuccess;
    return fp_mode == VR_FP_FMA ? launch_fp<1>(p, gp, n_cus, waves_override, gen_waves, stream, rays)
                                : launch_fp<0>(p, gp, n_cus, waves_override, gen_waves, stream, rays);
}

}  // namespace vr
