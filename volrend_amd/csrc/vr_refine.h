// vr_refine.h -- shared between the host side of vr_refine_plan / vr_refine_apply (vr_refine.cpp) and their kernels
// (vr_refine.hip).  Not part of the public ABI.
#pragma once
#include "vr_internal.h"

namespace vr {

// The caller's workspace, every part rounded up to whole 256-byte lines.  With W = ceil(capacity * N^3 / 32) words
// of the selection bitmap:
//   mask [W]      uint32  sel AND leaf, the bits at or beyond capacity * N^3 cleared
//   count[W + 1]  uint64  popcount of mask[w]; count[W] = 0, so that the scan's last output is the total
//   first[W + 1]  uint64  exclusive scan of count: the rank of the first refined slot of word w; first[W] = n_new
//   the scan's temporary storage: a few look-back words per block of >= 256 counts, bounded from above by
//   kRefineScanBase + kRefineScanPerWord * (W + 1); launch_refine_plan refuses to scan when the bound does not hold.
constexpr size_t kRefineLine = 256;
constexpr size_t kRefineScanBase = 64 * 1024;
constexpr size_t kRefineScanPerWord = 1;
inline size_t refine_lines(size_t bytes) { return (bytes + kRefineLine - 1) / kRefineLine * kRefineLine; }
inline int64_t refine_words(int N, int64_t capacity) { return (capacity * (int64_t)(N * N * N) + 31) / 32; }
inline size_t refine_scan_bytes(int64_t words) { return refine_lines(kRefineScanBase + kRefineScanPerWord * (size_t)(words + 1)); }
inline size_t refine_workspace_bytes(int N, int64_t capacity) {
    const int64_t w = refine_words(N, capacity);
    return refine_lines((size_t)w * 4) + 2 * refine_lines((size_t)(w + 1) * 8) + refine_scan_bytes(w);
}

// One call, passed BY VALUE to the kernels.
struct RefineArgs {
    const int32_t* child;
    const uint32_t* sel;
    int32_t* child_out;
    int32_t* src_slot;                // or NULL
    uint32_t* mask;                   // workspace
    unsigned long long* count;
    unsigned long long* first;
    void* scan_tmp;
    size_t scan_tmp_bytes;
    int64_t capacity, n_new, n_slots, words;
    int32_t N3;
};

// One companion array of an apply.
struct RefineArray {
    const void* src;
    void* dst;
    int32_t elem_bytes, dim, zero;
};

// vr_refine.hip.  Plan: mask kernel and scan; *scan_need = the bytes the scan asked for -- when that exceeds
// a.scan_tmp_bytes nothing is enqueued and hipErrorInvalidValue is returned.  Apply: the child kernel, and per array
// the copy of the old part and the expand kernel.
hipError_t launch_refine_plan(const RefineArgs& a, size_t* scan_need, hipStream_t stream);
hipError_t launch_refine_apply(const RefineArgs& a, const RefineArray* arrays, int n_arrays, hipStream_t stream);

}  // namespace vr
