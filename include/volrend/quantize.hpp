// volrend::quantize -- the median-cut encoder of the compressed tree.npz format, on the device, over the HIP C ABI
// (vr_quantize; include/volrend_hip.h has the definition, which the result meets bit for bit).  The call works on a
// data array in the FILE's layout in device memory, on the current device, takes no tree and only enqueues on
// `stream`: read the values of an uploaded tree with read_data (update.hpp), quantise, and hand the four outputs to
// N3Tree's quantised upload or to a file writer.  The outputs are exactly the arrays of VrQuantDesc with n_quant =
// n_basis - n_retained.  The buffers are the caller's (DeviceBuffer of internal/hip_owners.hpp holds them well);
// the workspace is free again once the work on `stream` is done.  Throws std::runtime_error ("vr_quantize: ...")
// where the C call refuses its arguments.
#pragma once
#include <cstdint>

#include "volrend_hip.h"

namespace volrend {

struct Quantize {
    const uint16_t* data = nullptr;     // device [n_slots][data_dim] binary16
    int64_t n_slots = 0;                // capacity * N^3
    int data_dim = 0;                   // 3 * n_basis + 1
    int n_retained = 1;                 // basis functions stored uncompressed, 0 .. n_basis - 1
    int bits = 16;                      // 1..16: 2^bits codebook rows in use
    float sigma_thresh = 2.0f;          // slots with (float)sigma > sigma_thresh are kept
    uint16_t* quant_colors = nullptr;   // device [n_quant][65536][3] binary16
    uint16_t* quant_map = nullptr;      // device [n_quant][n_slots]
    uint16_t* sigma = nullptr;          // device [n_slots] binary16
    uint16_t* data_retained = nullptr;  // device [n_retained][n_slots][3]; nullptr iff n_retained == 0
    void* workspace = nullptr;          // device, quantize_workspace(n_slots, data_dim) bytes, 256-byte aligned
    int64_t workspace_bytes = 0;
};

// Bytes of workspace; throws for arguments vr_quantize refuses.  No device call.
int64_t quantize_workspace(int64_t n_slots, int data_dim);
// Enqueue only.
void quantize(const Quantize& q, void* stream);

}  // namespace volrend
