// step_refusals.cpp -- the refusals of volrend::tree_step (include/volrend/step.hpp) and of the marked
// render_backward / render_backward_rays (grad.hpp, rays.hpp), which need no device: every check below comes
// before the tree handle is followed, so the tree carries a handle that is never followed and no pointer is ever
// read or written.  Prints one line per case: "<case> <what()>".
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <vector>
#include "volrend/grad.hpp"
#include "volrend/rays.hpp"
#include "volrend/step.hpp"
using namespace volrend;
template <typename F> static void expect_throw(const char* name, F&& f) {
    try { f(); std::printf("%s NO_THROW\n", name); }
    catch (const std::runtime_error& e) { std::printf("%s runtime_error: %s\n", name, e.what()); }
}
int main() {
    N3Tree tree, none;   // `none` has no device copy: its handle is NULL
    tree.device = reinterpret_cast<vr_tree_t>(0x1000);  // never followed: every call below is refused first
    float* f = reinterpret_cast<float*>(0x5000);
    uint32_t* bits = reinterpret_cast<uint32_t*>(0x6000);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    Step ok;
    ok.master = ok.grad = f;
    ok.touched = bits;
    ok.lr = ok.lr_sigma = 0.1f;
    Step adam = ok;
    adam.kind = StepKind::Adam;
    adam.m = adam.v = f;
    const auto step_with = [&](const char* name, const Step& base, auto&& change) {
        Step s = base;
        change(s);
        expect_throw(name, [&] { tree_step(tree, s, nullptr); });
    };
    expect_throw("step_null_tree", [&] { tree_step(none, ok, nullptr); });
    step_with("step_null_master", ok, [](Step& s) { s.master = nullptr; });
    step_with("step_null_grad", ok, [](Step& s) { s.grad = nullptr; });
    step_with("step_null_touched", ok, [](Step& s) { s.touched = nullptr; });
    step_with("step_kind", ok, [](Step& s) { s.kind = static_cast<StepKind>(2); });
    step_with("step_lr_nan", ok, [&](Step& s) { s.lr = nan; });
    step_with("step_lr_sigma_inf", ok, [&](Step& s) { s.lr_sigma = inf; });
    step_with("step_eps_nan", adam, [&](Step& s) { s.eps = nan; });
    step_with("step_adam_null_m", adam, [](Step& s) { s.m = nullptr; });
    step_with("step_adam_null_v", adam, [](Step& s) { s.v = nullptr; });
    step_with("step_adam_step0", adam, [](Step& s) { s.step = 0; });
    step_with("step_adam_beta1", adam, [](Step& s) { s.beta1 = 1.f; });
    step_with("step_adam_beta2", adam, [](Step& s) { s.beta2 = -0.1f; });

    Camera cam(64, 48, 50.f, 50.f);
    RenderOptions opt;
    std::vector<float> pose(12, 0.f);
    const std::vector<const float*> poses{pose.data()};
    expect_throw("frames_null_touched", [&] { render_backward(tree, cam, poses, opt, f, f, (uint32_t*)nullptr, nullptr); });
    expect_throw("frames_null_tree", [&] { render_backward(none, cam, poses, opt, f, f, bits, nullptr); });
    expect_throw("frames_null_grad", [&] { render_backward(tree, cam, poses, opt, f, nullptr, bits, nullptr); });
    const Rays rays{f, f, 64};
    expect_throw("rays_null_touched", [&] { render_backward_rays(tree, rays, opt, f, f, (uint32_t*)nullptr, nullptr); });
    expect_throw("rays_null_tree", [&] { render_backward_rays(none, rays, opt, f, f, bits, nullptr); });
    expect_throw("rays_null_grad_accum", [&] { render_backward_rays(tree, rays, opt, nullptr, f, bits, nullptr); });
    tree.device = nullptr;
    return 0;
}
