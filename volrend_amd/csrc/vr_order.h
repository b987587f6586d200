// vr_order.h -- shared between the host side of vr_order_rays (vr_order.cpp) and its kernels (vr_order.hip).
// Not part of the public ABI.
#pragma once
#include "vr_internal.h"

namespace vr {

constexpr int kOrderDefaultBits = 2;   // VrRayOrder.bits == 0 (include/volrend_hip.h states the value)
constexpr int kOrderMaxBits = 5;       // 6 * 5 = 30 key bits; bit 31 is only set in the miss key
constexpr int kOrderMaxPayload = 8;    // floats per payload row
constexpr uint32_t kOrderMissKey = 0xFFFFFFFFu;
constexpr int kOrderKeyWaves = 4;      // GW of order_key_kernel: waves per workgroup

// The caller's workspace: four arrays of n words (keys and ray indices, each twice: the sort ping-pongs
// between them), each rounded up to whole 256-byte lines, and behind them the sort's own temporary storage.
// Its size is a property of rocPRIM's tuning for the device, which cannot be asked without a device call:
// kOrderSortBase + kOrderSortPerRay * n bounds it from above (one 4-byte look-back word per radix digit and
// block of >= 1024 items, a few KB of histograms), and launch_order refuses to sort when the bound does not hold.
constexpr size_t kOrderLine = 256;
constexpr size_t kOrderSortBase = 64 * 1024;
constexpr size_t kOrderSortPerRay = 4;
inline size_t order_array_bytes(int64_t n) { return ((size_t)n * 4 + kOrderLine - 1) / kOrderLine * kOrderLine; }
inline size_t order_sort_bytes(int64_t n) { return kOrderSortBase + order_array_bytes(n) / 4 * kOrderSortPerRay; }
inline size_t order_workspace_bytes(int64_t n) {
    return n <= 0 ? 0 : 4 * order_array_bytes(n) + order_sort_bytes(n);
}

// One call, passed BY VALUE next to KParams (of which only what setup_ray_from reads is filled in) and the list.
struct OrderArgs {
    int32_t bits;            // 1..kOrderMaxBits, resolved
    int32_t payload_dim;     // 0 without a payload
    uint32_t* key[2];        // workspace: [n] each
    uint32_t* idx[2];
    void* sort_tmp;          // workspace: the sort's temporary storage
    size_t sort_tmp_bytes;
    const float* origins;    // the list (the gather pass reads its rows)
    const float* dirs;
    uint32_t* order;         // VrRayOrder
    uint32_t* keys;
    float* origins_out;
    float* dirs_out;
    const float* payload;
    float* payload_out;
};

// vr_order.hip: key kernel, stable sort of (key, index) pairs, gather kernel.  *sort_need = the bytes the sort
// asked for; when that exceeds a.sort_tmp_bytes nothing is enqueued and hipErrorInvalidValue is returned.
hipError_t launch_order(const KParams& p, const RayList& rl, const OrderArgs& a, int fp_mode, size_t* sort_need,
                        hipStream_t stream);

}  // namespace vr
