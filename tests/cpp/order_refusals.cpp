// order_refusals.cpp -- the refusals of volrend::order_rays (include/volrend/rays.hpp), which need no device: every
// check below comes before the tree handle is followed, so the tree carries a handle that is never followed and the
// pointers are never read or written.  Prints one line per case: "<case> <what()>".
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
    const float* pl = reinterpret_cast<const float*>(0x7000);
    float* po = reinterpret_cast<float*>(0x9000);
    void* ws = reinterpret_cast<void*>(0x100000);
    const int64_t n = 100;
    const size_t bytes = order_rays_workspace(n);
    const Rays rays{o, d, n};
    RayOrder out;
    out.order = reinterpret_cast<uint32_t*>(0xB000);
    auto call = [&](const Rays& r, const RayOrder& ro, void* w = reinterpret_cast<void*>(0x100000), size_t wb = 0,
                    int fp = VR_FP_STRICT) { order_rays(tree, r, opt, ro, w, wb ? wb : order_rays_workspace(r.n), nullptr, fp); };
    expect_throw("null_origins", [&] { call(Rays{nullptr, d, n}, out); });
    expect_throw("null_dirs", [&] { call(Rays{o, nullptr, n}, out); });
    RayOrder no_order = out;
    no_order.order = nullptr;
    expect_throw("null_order", [&] { call(rays, no_order); });
    expect_throw("fp_mode", [&] { call(rays, out, ws, 0, 2); });
    expect_throw("n_negative", [&] { call(Rays{o, d, -1}, out); });
    expect_throw("n_large", [&] { call(Rays{o, d, int64_t(1) << 30}, out); });
    RayOrder bits_lo = out, bits_hi = out;
    bits_lo.bits = -1;
    bits_hi.bits = 6;
    expect_throw("bits_negative", [&] { call(rays, bits_lo); });
    expect_throw("bits_large", [&] { call(rays, bits_hi); });
    RayOrder half = out;
    half.payload = pl;
    half.payload_dim = 3;
    expect_throw("payload_without_out", [&] { call(rays, half); });
    RayOrder other = out;
    other.payload_out = po;
    expect_throw("out_without_payload", [&] { call(rays, other); });
    RayOrder wide = out;
    wide.payload = pl;
    wide.payload_out = po;
    wide.payload_dim = 9;
    expect_throw("payload_dim_large", [&] { call(rays, wide); });
    wide.payload_dim = 0;
    expect_throw("payload_dim_zero", [&] { call(rays, wide); });
    RayOrder stray = out;
    stray.payload_dim = 3;
    expect_throw("payload_dim_without_payload", [&] { call(rays, stray); });
    expect_throw("null_workspace", [&] { call(rays, out, nullptr); });
    expect_throw("small_workspace", [&] { call(rays, out, ws, bytes - 1); });
    expect_throw("misaligned_workspace", [&] { call(rays, out, reinterpret_cast<void*>(0x100040)); });
    RayOrder in_place = out;
    in_place.origins_out = const_cast<float*>(o);
    expect_throw("origins_in_place", [&] { call(rays, in_place); });
    in_place = out;
    in_place.dirs_out = const_cast<float*>(d);
    expect_throw("dirs_in_place", [&] { call(rays, in_place); });
    in_place = out;
    in_place.payload = pl;
    in_place.payload_out = const_cast<float*>(pl);
    in_place.payload_dim = 3;
    expect_throw("payload_in_place", [&] { call(rays, in_place); });
    tree.device = nullptr;
    expect_throw("null_tree", [&] { call(rays, out); });
    // what is NOT refused: no ray at all, whatever the workspace
    tree.device = reinterpret_cast<vr_tree_t>(0x1000);
    try {
        order_rays(tree, Rays{o, d, 0}, opt, out, nullptr, 0, nullptr);
        std::printf("n_zero OK\n");
    } catch (const std::runtime_error& e) { std::printf("n_zero runtime_error: %s\n", e.what()); }
    tree.device = nullptr;  // (the handle was never one: nothing to free)
    return 0;
}
