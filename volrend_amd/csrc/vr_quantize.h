// vr_quantize.h -- shared between the host side of vr_quantize (vr_quantize.cpp) and its kernels
// (vr_quantize.hip).  Not part of the public ABI.
#pragma once
#include "vr_internal.h"

namespace vr {

constexpr int kQuantMaxBits = 16;
constexpr int kQuantRows = 65536;            // rows of one codebook, whatever `bits`
constexpr int kQuantMaxSortBoxes = 1 << 15;  // boxes that exist when a sort runs (levels 0 .. 15)
constexpr int kQuantBoxWords = 8;            // per box: min[3], 0xFFFF - max[3] of the orderable images, 2 spare

// The caller's workspace, every part a whole number of 256-byte lines:
//   pts   [n_slots] x 4 halves : the orderable images of (R, G, B) of the basis function at work, and the kept flag
//   key   2 x [n_slots] words  : the sort's keys, ping and pong
//   idx   2 x [n_slots] words  : the slot indices travelling with them
//   boxes kQuantMaxSortBoxes x kQuantBoxWords words, axis kQuantMaxSortBoxes words
//   sums  kQuantRows x 3 int64 : the codebook sums of the basis function at work
//   n_kept one word in a line of its own
//   sort  the radix sort's temporary storage, bounded as in vr_order.h (launch_quantize checks the bound)
constexpr size_t kQuantLine = 256;
constexpr size_t kQuantSortBase = 64 * 1024;
constexpr size_t kQuantSortPerSlot = 4;
inline size_t quant_lines(size_t bytes) { return (bytes + kQuantLine - 1) / kQuantLine * kQuantLine; }
inline size_t quant_sort_bytes(int64_t n) { return kQuantSortBase + quant_lines((size_t)n * 4) / 4 * kQuantSortPerSlot; }
constexpr size_t kQuantBoxBytes = (size_t)kQuantMaxSortBoxes * kQuantBoxWords * 4;
constexpr size_t kQuantAxisBytes = (size_t)kQuantMaxSortBoxes * 4;
constexpr size_t kQuantSumBytes = (size_t)kQuantRows * 3 * 8;
inline size_t quant_workspace_bytes(int64_t n) {
    return quant_lines((size_t)n * 8) + 4 * quant_lines((size_t)n * 4) + kQuantBoxBytes + kQuantAxisBytes +
           kQuantSumBytes + kQuantLine + quant_sort_bytes(n);
}

// One vr_quantize, passed BY VALUE to the kernels.
struct QuantizeArgs {
    const uint16_t* data;
    uint16_t* quant_colors;
    uint16_t* quant_map;
    uint16_t* sigma;
    uint16_t* data_retained;  // or NULL
    uint2* pts;
    uint32_t* key[2];
    uint32_t* idx[2];
    uint32_t* boxes;
    uint32_t* axis;
    long long* sums;
    uint32_t* n_kept;
    void* sort_tmp;
    size_t sort_tmp_bytes;
    int64_t n_slots;
    int32_t data_dim, n_basis, n_retained, n_quant, bits;
    float sigma_thresh;
};

// vr_quantize.hip: everything of one call, enqueued on `stream`.  *sort_need = the most the sort asked for; when
// that exceeds a.sort_tmp_bytes nothing is enqueued and hipErrorInvalidValue is returned.
hipError_t launch_quantize(const QuantizeArgs& a, size_t* sort_need, hipStream_t stream);

}  // namespace vr
