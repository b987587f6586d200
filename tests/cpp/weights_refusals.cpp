// weights_refusals.cpp -- the refusals of volrend::accumulate_weights (include/volrend/weights.hpp), which
// need no device: every check of vr_accumulate_weights comes before the tree handle is followed, so the
// tree below carries a handle that is never followed.  Prints one line per case: "<case> <what()>".
#include <cstdio>
#include <stdexcept>
#include "volrend/weights.hpp"
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
    LeafWeights ok{};
    ok.hits = reinterpret_cast<uint32_t*>(0x3000);
    expect_throw("both_null", [&] { accumulate_weights(tree, cam, {tr}, opt, LeafWeights{}, nullptr); });
    expect_throw("fp_mode", [&] { accumulate_weights(tree, cam, {tr, tr}, opt, ok, nullptr, 7); });
    RenderOptions still = opt;
    still.step_size = 0.f;
    expect_throw("step_size", [&] { accumulate_weights(tree, cam, {tr}, still, ok, nullptr, VR_FP_FMA); });
    tree.device = nullptr;
    return 0;
}
