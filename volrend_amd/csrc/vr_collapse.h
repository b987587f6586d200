// vr_collapse.h -- shared between the host side of vr_collapse_plan / vr_collapse_apply (vr_collapse.cpp) and their
// kernels (vr_collapse.hip).  Not part of the public ABI.
#pragma once
#include "vr_internal.h"

namespace vr {

// The caller's workspace, every part rounded up to whole 256-byte lines.  With W = ceil(capacity / 32) words of the
// selection bitmap over NODES:
//   col  [W]        uint32  the collapse word: sel AND frontier, bit 0 of word 0 and the bits at or beyond capacity cleared
//   count[W + 1]    uint64  popcount of the KEEP word (NOT col, the bits at or beyond capacity cleared); count[W] = 0,
//                           so that the scan's last output is the total
//   first[W + 1]    uint64  exclusive scan of count: the new index of the first kept node of word w; first[W] = n_keep
//   into [capacity] int32   apply's own into_slot, used where the caller passes none and an array has a rule other
//                           than KEEP
//   the scan's temporary storage, bounded as vr_refine.h bounds it; launch_collapse_plan refuses to scan otherwise.
constexpr size_t kCollapseLine = 256;
constexpr size_t kCollapseScanBase = 64 * 1024;
constexpr size_t kCollapseScanPerWord = 1;
inline size_t collapse_lines(size_t bytes) { return (bytes + kCollapseLine - 1) / kCollapseLine * kCollapseLine; }
inline int64_t collapse_words(int64_t capacity) { return (capacity + 31) / 32; }
inline size_t collapse_scan_bytes(int64_t words) {
    return collapse_lines(kCollapseScanBase + kCollapseScanPerWord * (size_t)(words + 1));
}
inline size_t collapse_workspace_bytes(int64_t capacity) {
    const int64_t w = collapse_words(capacity);
    return collapse_lines((size_t)w * 4) + 2 * collapse_lines((size_t)(w + 1) * 8) + collapse_lines((size_t)capacity * 4) +
           collapse_scan_bytes(w);
}

// One call, passed BY VALUE to the kernels.
struct CollapseArgs {
    const int32_t* child;
    const uint32_t* sel;
    int32_t* child_out;
    int32_t* node_map;                // or NULL
    int32_t* src_node;                // or NULL
    int32_t* into_slot;               // the caller's, or `into` of the workspace, or NULL when nobody reads it
    uint32_t* col;                    // workspace
    unsigned long long* count;
    unsigned long long* first;
    int32_t* into;
    void* scan_tmp;
    size_t scan_tmp_bytes;
    int64_t capacity, n_keep, n_slots, words;
    int32_t N3;
};

// One companion array of an apply.
struct CollapseArray {
    const void* src;
    void* dst;
    int32_t elem_bytes, dim, rule;
};

// vr_collapse.hip.  Plan: the collapse-word kernel and the scan; *scan_need = the bytes the scan asked for -- when
// that exceeds a.scan_tmp_bytes nothing is enqueued and hipErrorInvalidValue is returned.  Apply: the fill of
// into_slot, the child kernel, and per array the gather and (ZERO / MEAN) the kernel of the merged slots.
hipError_t launch_collapse_plan(const CollapseArgs& a, size_t* scan_need, hipStream_t stream);
hipError_t launch_collapse_apply(const CollapseArgs& a, const CollapseArray* arrays, int n_arrays, hipStream_t stream);

}  // namespace vr
