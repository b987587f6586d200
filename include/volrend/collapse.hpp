// volrend::collapse_plan / collapse_apply -- a tree restated with selected frontier nodes merged into their parent
// slots and the node array compacted, on the device, over the HIP C ABI (vr_collapse_plan / vr_collapse_apply;
// include/volrend_hip.h has the semantics in plain integers).  The calls work on arrays in the FILE's layout in
// device memory, on the current device, and take no tree: read the values of an uploaded tree with read_data
// (update.hpp), collapse, and upload the result with N3Tree's device-array constructor.  The selection is per NODE;
// the kept nodes keep their relative order, and one call collapses one level.  Each call throws std::runtime_error
// ("vr_collapse_plan: ..." etc.) where the C call refuses its arguments.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "volrend_hip.h"

namespace volrend {

enum class CollapseRule { Keep = VR_COLLAPSE_KEEP, Zero = VR_COLLAPSE_ZERO, Mean = VR_COLLAPSE_MEAN };

// One companion array, indexed as the file's data array (slot * dim + e): the tree's binary16 values, a float32
// master, optimiser moments, leaf weights.
struct CollapseArray {
    const void* src = nullptr;  // device, capacity * N^3 * dim elements
    void* dst = nullptr;        // device, n_keep * N^3 * dim elements, != src
    int elem_bytes = 2;         // 2 or 4: elements move as bits; Mean reads binary16 / binary32
    int dim = 1;                // elements per slot
    CollapseRule rule = CollapseRule::Keep;  // what the parent slot of a collapsed node gets
};

struct Collapse {
    const int32_t* child = nullptr;   // device [capacity * N^3]: the file's relative offsets, 0 = leaf
    const uint32_t* sel = nullptr;    // device bitmap over NODES: bit m & 31 of word m >> 5
    int N = 0;
    int64_t capacity = 0;
    void* workspace = nullptr;        // device, collapse_workspace(N, capacity) bytes, 256-byte aligned: the caller's,
    size_t workspace_bytes = 0;       // unchanged between plan and apply
};

// The optional outputs of collapse_apply, each device memory or nullptr.
struct CollapseMaps {
    int32_t* node_map = nullptr;   // [capacity]: the new index of an old node, -1 if collapsed
    int32_t* src_node = nullptr;   // [n_keep]: the old index of a new node
    int32_t* into_slot = nullptr;  // [capacity]: the new slot a collapsed node went into, else -1
};

size_t collapse_workspace(int N, int64_t capacity);
// The number of kept nodes (capacity minus the selected frontier nodes).  Waits for `stream`: the one host-blocking
// step.
int64_t collapse_plan(const Collapse& c, void* stream);
// Enqueue only.  child_out: device [n_keep * N^3]; n_keep: what collapse_plan returned for the same c.
void collapse_apply(const Collapse& c, int64_t n_keep, int32_t* child_out, const CollapseMaps& maps,
                    const std::vector<CollapseArray>& arrays, void* stream);

}  // namespace volrend
