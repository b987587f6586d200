// geometry_refusals.cpp -- the refusals of volrend::tree_geometry / slot_points (include/volrend/geometry.hpp), which
// need no device: every check below comes before any device call, so the pointers are never read or written.  Prints
// one line per case: "<case> <what()>".
#include <cstdio>
#include <stdexcept>
#include "volrend/geometry.hpp"
using namespace volrend;
template <typename F> static void expect_throw(const char* name, F&& f) {
    try { f(); std::printf("%s NO_THROW\n", name); }
    catch (const std::runtime_error& e) { std::printf("%s runtime_error: %s\n", name, e.what()); }
}
int main() {
    Geometry g;
    g.child = reinterpret_cast<const int32_t*>(0x1000);
    g.parent_slot = reinterpret_cast<int32_t*>(0x2000);
    g.node_depth = reinterpret_cast<int32_t*>(0x3000);
    g.node_origin = reinterpret_cast<uint32_t*>(0x4000);
    g.N = 2;
    g.capacity = 10;
    auto geom = [&](const char* name, auto&& change) {
        Geometry bad = g;
        change(bad);
        expect_throw(name, [&] { tree_geometry(bad, nullptr); });
    };
    geom("geometry.null_child", [](Geometry& b) { b.child = nullptr; });
    geom("geometry.no_output", [](Geometry& b) { b.parent_slot = b.node_depth = nullptr; b.node_origin = nullptr; });
    geom("geometry.n_small", [](Geometry& b) { b.N = 1; });
    geom("geometry.n_large", [](Geometry& b) { b.N = 17; });
    geom("geometry.capacity_zero", [](Geometry& b) { b.capacity = 0; });
    geom("geometry.capacity_large", [](Geometry& b) { b.capacity = int64_t(1) << 31; });
    geom("geometry.too_many_slots", [](Geometry& b) { b.capacity = (int64_t(1) << 31) - 1; });

    SlotPoints p;
    p.slots = reinterpret_cast<const int32_t*>(0x5000);
    p.n = 100;
    p.k = 3;
    p.mode = PointsMode::Jitter;
    p.points = reinterpret_cast<float*>(0x6000);
    p.depth = reinterpret_cast<int32_t*>(0x7000);
    p.side = reinterpret_cast<float*>(0x8000);
    auto pts = [&](const char* name, auto&& change) {
        Geometry bg = g;
        SlotPoints bad = p;
        change(bg, bad);
        expect_throw(name, [&] { slot_points(bg, bad, nullptr); });
    };
    pts("points.null_slots", [](Geometry&, SlotPoints& b) { b.slots = nullptr; });
    pts("points.null_node_depth", [](Geometry& bg, SlotPoints&) { bg.node_depth = nullptr; });
    pts("points.null_node_origin", [](Geometry& bg, SlotPoints&) { bg.node_origin = nullptr; });
    pts("points.no_output", [](Geometry&, SlotPoints& b) { b.points = b.side = nullptr; b.depth = nullptr; });
    pts("points.n_negative", [](Geometry&, SlotPoints& b) { b.n = -1; });
    pts("points.n_large", [](Geometry&, SlotPoints& b) { b.n = int64_t(1) << 31; });
    pts("points.k_zero", [](Geometry&, SlotPoints& b) { b.k = 0; });
    pts("points.k_large", [](Geometry&, SlotPoints& b) { b.k = 65; });
    pts("points.mode", [](Geometry&, SlotPoints& b) { b.mode = static_cast<PointsMode>(2); });
    pts("points.N", [](Geometry& bg, SlotPoints&) { bg.N = 0; });
    pts("points.capacity", [](Geometry& bg, SlotPoints&) { bg.capacity = -3; });
    // what is NOT refused: an empty list, whatever its pointer -- nothing is read and nothing is launched
    try {
        SlotPoints none = p;
        none.n = 0;
        none.slots = nullptr;
        slot_points(g, none, nullptr);
        std::printf("points.n_zero OK\n");
    } catch (const std::runtime_error& e) { std::printf("points.n_zero runtime_error: %s\n", e.what()); }
    return 0;
}
