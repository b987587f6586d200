// grad_refusals.cpp -- the refusals of volrend::render_backward (include/volrend/grad.hpp), which need no
// device: every check below comes before the tree handle is followed, so the tree carries a handle that is
// never followed.  Prints one line per case: "<case> <what()>".
#include <cstdio>
#include <stdexcept>
#include "volrend/grad.hpp"
using namespace volrend;
template <typename F> static void expect_throw(const char* name, F&& f) {
    try { f(); std::printf("%s NO_THROW\n", name); }
    catch (const std::runtime_error& e) { std::printf("%s runtime_error: %s\n", name, e.what()); }
}
int main() {
    N3Tree tree;
    tree.device = reinterpret_cast<vr_tree_t>(0x1000);  // never followed: every call below is refused first
    Camera cam(64, 48, 50.f, 50.f);
    RenderOptions opt;
    const float* tr = glm::value_ptr(cam.transform);
    const float* g = reinterpret_cast<const float*>(0x3000);
    float* d = reinterpret_cast<float*>(0x5000);
    expect_throw("null_grad_accum", [&] { render_backward(tree, cam, {tr}, opt, nullptr, d, nullptr); });
    expect_throw("null_grad_data", [&] { render_backward(tree, cam, {tr}, opt, g, nullptr, nullptr); });
    expect_throw("fp_mode", [&] { render_backward(tree, cam, {tr, tr}, opt, g, d, nullptr, 7); });
    RenderOptions still = opt;
    still.step_size = 0.f;
    expect_throw("step_size", [&] { render_backward(tree, cam, {tr}, still, g, d, nullptr, VR_FP_FMA); });
    RenderOptions depth = opt;
    depth.render_depth = true;
    expect_throw("render_depth", [&] { render_backward(tree, cam, {tr}, depth, g, d, nullptr); });
    RenderOptions rot = opt;
    rot.rot_dirs[1] = 0.25f;
    expect_throw("rot_dirs", [&] { render_backward(tree, cam, {tr}, rot, g, d, nullptr); });
    tree.device = nullptr;
    return 0;
}
