// rays_refusals.cpp -- the refusals of volrend::render_rays / accumulate_weights_rays / render_backward_rays
// (include/volrend/rays.hpp), which need no device: every check below comes before the tree handle is followed,
// so the tree carries a handle that is never followed.  Prints one line per case: "<case> <what()>".
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
    float* acc = reinterpret_cast<float*>(0x7000);
    float* gd = reinterpret_cast<float*>(0x9000);
    const Rays rays{o, d, 100};
    LeafWeights lw{acc, nullptr};
    // colour
    expect_throw("render_null_origins", [&] { render_rays(tree, Rays{nullptr, d, 100}, opt, nullptr, acc, nullptr); });
    expect_throw("render_null_dirs", [&] { render_rays(tree, Rays{o, nullptr, 100}, opt, nullptr, acc, nullptr); });
    expect_throw("render_no_output", [&] { render_rays(tree, rays, opt, nullptr, nullptr, nullptr); });
    expect_throw("render_fp_mode", [&] { render_rays(tree, rays, opt, nullptr, acc, nullptr, 7); });
    expect_throw("render_n_negative", [&] { render_rays(tree, Rays{o, d, -1}, opt, nullptr, acc, nullptr); });
    expect_throw("render_n_large", [&] { render_rays(tree, Rays{o, d, int64_t(1) << 30}, opt, nullptr, acc, nullptr); });
    RenderOptions still = opt;
    still.step_size = 0.f;
    expect_throw("render_step_size", [&] { render_rays(tree, rays, still, nullptr, acc, nullptr, VR_FP_FMA); });
    RenderOptions depth = opt;
    depth.render_depth = true;
    expect_throw("render_render_depth", [&] { render_rays(tree, rays, depth, nullptr, acc, nullptr); });
    RenderOptions probe = opt;
    probe.enable_probe = true;
    expect_throw("render_enable_probe", [&] { render_rays(tree, rays, probe, nullptr, acc, nullptr); });
    // leaf weights
    expect_throw("weights_null_dirs", [&] { accumulate_weights_rays(tree, Rays{o, nullptr, 100}, opt, lw, nullptr); });
    expect_throw("weights_no_output", [&] { accumulate_weights_rays(tree, rays, opt, LeafWeights{nullptr, nullptr}, nullptr); });
    expect_throw("weights_fp_mode", [&] { accumulate_weights_rays(tree, rays, opt, lw, nullptr, -1); });
    expect_throw("weights_n_large", [&] { accumulate_weights_rays(tree, Rays{o, d, int64_t(1) << 31}, opt, lw, nullptr); });
    expect_throw("weights_step_size", [&] { accumulate_weights_rays(tree, rays, still, lw, nullptr); });
    // backward
    expect_throw("backward_null_grad_accum", [&] { render_backward_rays(tree, rays, opt, nullptr, gd, nullptr); });
    expect_throw("backward_null_grad_data", [&] { render_backward_rays(tree, rays, opt, acc, nullptr, nullptr); });
    expect_throw("backward_null_origins", [&] { render_backward_rays(tree, Rays{nullptr, d, 100}, opt, acc, gd, nullptr); });
    expect_throw("backward_fp_mode", [&] { render_backward_rays(tree, rays, opt, acc, gd, nullptr, 2); });
    expect_throw("backward_n_negative", [&] { render_backward_rays(tree, Rays{o, d, -5}, opt, acc, gd, nullptr); });
    expect_throw("backward_step_size", [&] { render_backward_rays(tree, rays, still, acc, gd, nullptr); });
    expect_throw("backward_render_depth", [&] { render_backward_rays(tree, rays, depth, acc, gd, nullptr); });
    expect_throw("backward_enable_probe", [&] { render_backward_rays(tree, rays, probe, acc, gd, nullptr); });
    RenderOptions rot = opt;
    rot.rot_dirs[1] = 0.25f;
    expect_throw("backward_rot_dirs", [&] { render_backward_rays(tree, rays, rot, acc, gd, nullptr); });
    // reserve
    expect_throw("reserve_n_slots", [&] { reserve_rays(tree, 100, 9); });
    expect_throw("reserve_n_large", [&] { reserve_rays(tree, int64_t(1) << 30, 2); });
    tree.device = nullptr;
    expect_throw("reserve_null_tree", [&] { reserve_rays(tree, 100, 2); });
    return 0;
}
