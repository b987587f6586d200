// volrend::refine_plan / refine_apply -- a tree restated with selected leaves subdivided, on the device, over the HIP
// C ABI (vr_refine_plan / vr_refine_apply; include/volrend_hip.h has the semantics in plain integers).  The calls
// work on arrays in the FILE's layout in device memory, on the current device, and take no tree: read the values of
// an uploaded tree with read_data (update.hpp), refine, and upload the result with N3Tree's device-array
// constructor.  The refinement is append-only: old nodes and slots keep their indices, the r-th refined slot in
// ascending order becomes node capacity + r.  Each call throws std::runtime_error ("vr_refine_plan: ..." etc.) where
// the C call refuses its arguments.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "volrend_hip.h"

namespace volrend {

// One companion array, indexed as the file's data array (slot * dim + e): the tree's binary16 values, a float32
// master, optimiser moments, leaf weights.
struct RefineArray {
    const void* src = nullptr;  // device, capacity * N^3 * dim elements
    void* dst = nullptr;        // device, (capacity + n_new) * N^3 * dim elements, != src
    int elem_bytes = 2;         // 2 or 4: elements move as bits
    int dim = 1;                // elements per slot
    bool zero = false;          // the slots of new nodes: false = the refined slot's elements, true = zero bits
};

struct Refine {
    const int32_t* child = nullptr;   // device [capacity * N^3]: the file's relative offsets, 0 = leaf
    const uint32_t* sel = nullptr;    // device: the `touched` bitmap format, bit s & 31 of word s >> 5
    int N = 0;
    int64_t capacity = 0;
    void* workspace = nullptr;        // device, refine_workspace(N, capacity) bytes, 256-byte aligned: the caller's,
    size_t workspace_bytes = 0;       // unchanged between plan and apply
};

size_t refine_workspace(int N, int64_t capacity);
// The number of refined slots (selected AND leaf).  Waits for `stream`: the one host-blocking step.
int64_t refine_plan(const Refine& r, void* stream);
// Enqueue only.  child_out: device [(capacity + n_new) * N^3]; src_slot: device [n_new] or nullptr; n_new: what
// refine_plan returned for the same r.
void refine_apply(const Refine& r, int64_t n_new, int32_t* child_out, int32_t* src_slot,
                  const std::vector<RefineArray>& arrays, void* stream);

}  // namespace volrend
