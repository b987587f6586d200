// aov_check.cpp -- the refusals of volrend::launch_renderer_aov[_batch] (include/volrend/aov.hpp), which
// need no device: every check of vr_render_aov comes before the tree handle is dereferenced, so the
// tree below carries a handle that is never followed.  Prints one line per case: "<case> <what()>".
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "volrend/aov.hpp"

using namespace volrend;

template <typename F>
static void expect_throw(const char* name, F&& f) {
    try {
        f();
        std::printf("%s NO_THROW\n", name);
    } catch (const std::invalid_argument& e) {
        std::printf("%s invalid_argument: %s\n", name, e.what());
    } catch (const std::runtime_error& e) {
        std::printf("%s runtime_error: %s\n", name, e.what());
    }
}

int main() {
    static_assert((int)DepthUnits::Tree == VR_DEPTH_TREE && (int)DepthUnits::World == VR_DEPTH_WORLD, "units");
    N3Tree tree;
    tree.device = reinterpret_cast<vr_tree_t>(0x1000);  // never dereferenced: every call below is refused first
    Camera cam(64, 48, 50.f, 50.f);
    RenderOptions opt;
    void* img = reinterpret_cast<void*>(0x2000);
    float* plane = reinterpret_cast<float*>(0x3000);
    AovPlanes ok;
    ok.depth = plane;

    expect_throw("both_null", [&] { launch_renderer_aov(tree, cam, opt, img, nullptr, AovPlanes{}, DepthUnits::Tree, nullptr, true); });
    expect_throw("units", [&] { launch_renderer_aov(tree, cam, opt, img, nullptr, ok, (DepthUnits)7, nullptr, true); });
    AovPlanes narrow = ok;
    narrow.pitch = 64 * 4 - 4;
    expect_throw("pitch_small", [&] { launch_renderer_aov(tree, cam, opt, img, nullptr, narrow, DepthUnits::World, nullptr, true); });
    AovPlanes odd = ok;
    odd.pitch = 64 * 4 + 2;
    expect_throw("pitch_odd", [&] { launch_renderer_aov(tree, cam, opt, img, nullptr, odd, DepthUnits::World, nullptr, true); });
    RenderOptions depth_mode = opt;
    depth_mode.render_depth = true;
    expect_throw("render_depth", [&] { launch_renderer_aov(tree, cam, depth_mode, img, nullptr, ok, DepthUnits::Tree, nullptr, true); });
    RenderOptions probe = opt;
    probe.enable_probe = true;
    expect_throw("probe", [&] { launch_renderer_aov(tree, cam, probe, img, nullptr, ok, DepthUnits::Tree, nullptr, true); });
    expect_throw("null_image", [&] { launch_renderer_aov(tree, cam, opt, nullptr, nullptr, ok, DepthUnits::Tree, nullptr, true); });
    const float* tr = glm::value_ptr(cam.transform);
    expect_throw("batch_sizes", [&] {
        launch_renderer_aov_batch(tree, cam, {tr, tr}, opt, {img, img}, {ok}, DepthUnits::Tree, nullptr);
    });
    expect_throw("batch_second_null", [&] {
        launch_renderer_aov_batch(tree, cam, {tr, tr}, opt, {img, img}, {ok, AovPlanes{}}, DepthUnits::Tree, nullptr);
    });
    tree.device = nullptr;
    return 0;
}
