// geometry.cpp -- volrend::tree_geometry / slot_points over vr_tree_geometry / vr_slot_points.
#include "volrend/geometry.hpp"

#include "volrend/internal/check.hpp"

namespace volrend {

void tree_geometry(const Geometry& g, void* stream) {
    VrGeometry c{};
    c.child = g.child;
    c.parent_slot = g.parent_slot;
    c.node_depth = g.node_depth;
    c.node_origin = g.node_origin;
    c.capacity = g.capacity;
    c.N = g.N;
    internal::vr_check(vr_tree_geometry(&c, stream), "vr_tree_geometry");
}

void slot_points(const Geometry& g, const SlotPoints& p, void* stream) {
    VrSlotPoints c{};
    c.node_depth = g.node_depth;
    c.node_origin = g.node_origin;
    c.slots = p.slots;
    c.points = p.points;
    c.depth = p.depth;
    c.side = p.side;
    c.capacity = g.capacity;
    c.n = p.n;
    c.N = g.N;
    c.k = p.k;
    c.mode = (int32_t)p.mode;
    c.seed = p.seed;
    internal::vr_check(vr_slot_points(&c, stream), "vr_slot_points");
}

}  // namespace volrend
