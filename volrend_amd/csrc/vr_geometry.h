// vr_geometry.h -- shared between the host side of vr_tree_geometry / vr_slot_points (vr_geometry.cpp) and their
// kernels (vr_geometry.hip).  Not part of the public ABI.
#pragma once
#include "vr_internal.h"

namespace vr {

constexpr int kGeomMaxDepth = VR_GEOM_MAX_DEPTH;

// One vr_tree_geometry, passed BY VALUE to the kernels.  `parent` is the caller's parent_slot or the call's
// temporary; the walk kernel runs when node_depth or node_origin is wanted.
struct GeometryArgs {
    const int32_t* child;
    int32_t* parent;
    int32_t* node_depth;    // or NULL
    uint32_t* node_origin;  // or NULL
    int64_t capacity, n_slots;
    int32_t N, N3;
};

// One vr_slot_points, passed BY VALUE to the kernel.
struct SlotPointsArgs {
    const int32_t* node_depth;
    const uint32_t* node_origin;
    const int32_t* slots;
    float* points;   // or NULL
    int32_t* depth;  // or NULL
    float* side;     // or NULL
    int64_t n_slots, n, total, n_chunks;  // total = n * k outputs, in chunks of 64
    int32_t N, N3, k, jitter;
    uint32_t seed;
};

// vr_geometry.hip.  Geometry: the fill of `parent` with -1, the scatter over the slots and, when an output of it is
// wanted, the walk.  Points: the one kernel; a.n_chunks > 0.
hipError_t launch_tree_geometry(const GeometryArgs& a, hipStream_t stream);
hipError_t launch_slot_points(const SlotPointsArgs& a, hipStream_t stream);

}  // namespace vr
