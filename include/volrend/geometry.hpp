// volrend::tree_geometry / slot_points -- where a slot is, on the device, over the HIP C ABI (vr_tree_geometry /
// vr_slot_points; include/volrend_hip.h has the semantics in plain integers).  The calls work on arrays in the FILE's
// layout in device memory, on the current device, take no tree and only enqueue on `stream`.  Geometry: per node the
// slot that links to it, its depth and the integer coordinate of its lower corner in the grid of its level.  Points:
// k points in the cell of each listed slot, in TREE coordinates (vr_query_points(VR_SPACE_TREE) takes them as they
// are), with the slot's depth and cell edge.  Each call throws std::runtime_error ("vr_tree_geometry: ..." etc.)
// where the C call refuses its arguments.
#pragma once
#include <cstdint>

#include "volrend_hip.h"

namespace volrend {

struct Geometry {
    const int32_t* child = nullptr;   // device [capacity * N^3]: the file's relative offsets, 0 = leaf
    int N = 0;
    int64_t capacity = 0;
    int32_t* parent_slot = nullptr;   // device [capacity], or nullptr: not wanted
    int32_t* node_depth = nullptr;    // device [capacity], or nullptr
    uint32_t* node_origin = nullptr;  // device [capacity][3], or nullptr
};

enum class PointsMode { Center = VR_POINTS_CENTER, Jitter = VR_POINTS_JITTER };

struct SlotPoints {
    const int32_t* slots = nullptr;   // device [n]: slot indices, in any order, repeats allowed
    int64_t n = 0;
    int k = 1;                        // points per slot, 1..VR_POINTS_MAX_K
    PointsMode mode = PointsMode::Center;
    uint32_t seed = 0;                // Jitter
    float* points = nullptr;          // device [n][k][3], or nullptr: not wanted
    int32_t* depth = nullptr;         // device [n], or nullptr
    float* side = nullptr;            // device [n], or nullptr
};

// Enqueue only.  At least one output of g.
void tree_geometry(const Geometry& g, void* stream);
// Enqueue only.  g: the tree and the node_depth / node_origin a tree_geometry of it wrote (ordered before this call
// by `stream` or by the caller).  At least one output of p.
void slot_points(const Geometry& g, const SlotPoints& p, void* stream);

}  // namespace volrend
