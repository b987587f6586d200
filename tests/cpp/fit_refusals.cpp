// fit_refusals.cpp -- the refusals of volrend::fit_rays (include/volrend/rays.hpp), which need no device: every
// check below comes before the tree handle is followed, so the tree carries a handle that is never followed.
// Prints one line per case: "<case> <what()>".
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include "volrend/rays.hpp"
using namespace volrend;
template <typename F> static void expect_throw(const char* name, F&& f) {
    try { f(); std::printf("%s NO_THROW\n", name); }
    catch (const std::runtime_error& e) { std::printf("%s runtime_error: %s\n", name, e.what()); }
}
int main() {
    N3Tree tree;
    tree.device = reinterpret_cast<vr_tree_t>(0x1000);  // never followed: every call below is refused first
    RenderOptions opt;
    const float* o = reinterpret_cast<const float*>(0x3000);
    const float* d = reinterpret_cast<const float*>(0x5000);
    const float* tg = reinterpret_cast<const float*>(0x7000);
    float* gd = reinterpret_cast<float*>(0x9000);
    const Rays rays{o, d, 100};
    Fit fit;
    fit.target = tg;
    fit.grad_scale = 0.5f;
    fit.grad_data = gd;
    expect_throw("null_origins", [&] { fit_rays(tree, Rays{nullptr, d, 100}, opt, fit, nullptr); });
    expect_throw("null_dirs", [&] { fit_rays(tree, Rays{o, nullptr, 100}, opt, fit, nullptr); });
    Fit no_target = fit;
    no_target.target = nullptr;
    expect_throw("null_target", [&] { fit_rays(tree, rays, opt, no_target, nullptr); });
    Fit no_grad = fit;
    no_grad.grad_data = nullptr;
    expect_throw("null_grad_data", [&] { fit_rays(tree, rays, opt, no_grad, nullptr); });
    expect_throw("fp_mode", [&] { fit_rays(tree, rays, opt, fit, nullptr, 2); });
    expect_throw("n_negative", [&] { fit_rays(tree, Rays{o, d, -1}, opt, fit, nullptr); });
    expect_throw("n_large", [&] { fit_rays(tree, Rays{o, d, int64_t(1) << 30}, opt, fit, nullptr); });
    RenderOptions still = opt;
    still.step_size = 0.f;
    expect_throw("step_size", [&] { fit_rays(tree, rays, still, fit, nullptr, VR_FP_FMA); });
    Fit inf_scale = fit, nan_scale = fit;
    inf_scale.grad_scale = INFINITY;
    nan_scale.grad_scale = NAN;
    expect_throw("grad_scale_inf", [&] { fit_rays(tree, rays, opt, inf_scale, nullptr); });
    expect_throw("grad_scale_nan", [&] { fit_rays(tree, rays, opt, nan_scale, nullptr); });
    RenderOptions depth = opt;
    depth.render_depth = true;
    expect_throw("render_depth", [&] { fit_rays(tree, rays, depth, fit, nullptr); });
    RenderOptions probe = opt;
    probe.enable_probe = true;
    expect_throw("enable_probe", [&] { fit_rays(tree, rays, probe, fit, nullptr); });
    RenderOptions rot = opt;
    rot.rot_dirs[1] = 0.25f;
    expect_throw("rot_dirs", [&] { fit_rays(tree, rays, rot, fit, nullptr); });
    tree.device = nullptr;
    expect_throw("null_tree", [&] { fit_rays(tree, rays, opt, fit, nullptr); });
    return 0;
}
