// vr_quantize.cpp -- the C ABI of vr_quantize (include/volrend_hip.h), host side: argument checks, the carving of
// the caller's workspace, and the enqueue.  No tree handle: the call works on the calling thread's current device
// and waits for nothing.  The kernels and the sort are in vr_quantize.hip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "vr_host.h"
#include "vr_quantize.h"

namespace {

bool size_args_ok(int64_t n_slots, int data_dim) {
    return n_slots >= 1 && n_slots <= (int64_t)INT32_MAX && data_dim >= 4 && (data_dim - 1) % 3 == 0;
}

}  // namespace

extern "C" {

int64_t vr_quantize_workspace(int64_t n_slots, int data_dim) {
    return size_args_ok(n_slots, data_dim) ? (int64_t)vr::quant_workspace_bytes(n_slots) : -1;
}

int vr_quantize(const VrQuantize* q, void* stream) {
    const char* const what = "vr_quantize";
    if (!q) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (!q->data || !q->quant_colors || !q->quant_map || !q->sigma || !q->workspace)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL data, quant_colors, quant_map, sigma or workspace", what);
    if (!size_args_ok(q->n_slots, q->data_dim))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n_slots = %lld outside [1, 2^31) or data_dim = %d not 3 * n_basis + 1",
                    what, (long long)q->n_slots, q->data_dim);
    const int n_basis = (q->data_dim - 1) / 3;
    if (q->n_retained < 0 || q->n_retained > n_basis - 1)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n_retained = %d outside 0..%d", what, q->n_retained, n_basis - 1);
    if ((q->data_retained != nullptr) != (q->n_retained > 0))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: data_retained goes with n_retained > 0, and only with it", what);
    if (q->bits < 1 || q->bits > vr::kQuantMaxBits)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: bits = %d outside 1..%d", what, q->bits, vr::kQuantMaxBits);
    if (q->sigma_thresh != q->sigma_thresh) return fail(VR_ERR_INVALID_ARGUMENT, "%s: sigma_thresh is NaN", what);
    const void* const in = q->data;
    if (q->quant_colors == in || q->quant_map == in || q->sigma == in || q->data_retained == in)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: an output is the input array", what);
    const size_t need = vr::quant_workspace_bytes(q->n_slots);
    if (q->workspace_bytes < 0 || (uint64_t)q->workspace_bytes < need ||
        reinterpret_cast<uintptr_t>(q->workspace) % vr::kQuantLine != 0)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: workspace %p of %lld bytes: %zu bytes, 256-byte aligned, are needed", what,
                    q->workspace, (long long)q->workspace_bytes, need);

    vr::QuantizeArgs a;
    memset(&a, 0, sizeof(a));
    a.data = q->data;
    a.quant_colors = q->quant_colors;
    a.quant_map = q->quant_map;
    a.sigma = q->sigma;
    a.data_retained = q->data_retained;
    a.n_slots = q->n_slots;
    a.data_dim = q->data_dim;
    a.n_basis = n_basis;
    a.n_retained = q->n_retained;
    a.n_quant = n_basis - q->n_retained;
    a.bits = q->bits;
    a.sigma_thresh = q->sigma_thresh;
    char* w = static_cast<char*>(q->workspace);
    const size_t words = vr::quant_lines((size_t)a.n_slots * 4);
    a.pts = reinterpret_cast<uint2*>(w);
    w += vr::quant_lines((size_t)a.n_slots * 8);
    for (int i = 0; i < 2; ++i) {
        a.key[i] = reinterpret_cast<uint32_t*>(w);
        a.idx[i] = reinterpret_cast<uint32_t*>(w + 2 * words);
        w += words;
    }
    w += 2 * words;
    a.boxes = reinterpret_cast<uint32_t*>(w);
    w += vr::kQuantBoxBytes;
    a.axis = reinterpret_cast<uint32_t*>(w);
    w += vr::kQuantAxisBytes;
    a.sums = reinterpret_cast<long long*>(w);
    w += vr::kQuantSumBytes;
    a.n_kept = reinterpret_cast<uint32_t*>(w);
    w += vr::kQuantLine;
    a.sort_tmp = w;
    a.sort_tmp_bytes = vr::quant_sort_bytes(a.n_slots);

    size_t sort_need = 0;
    const hipError_t e = vr::launch_quantize(a, &sort_need, static_cast<hipStream_t>(stream));
    if (sort_need > a.sort_tmp_bytes)
        return fail(VR_ERR_HIP, "%s: the sort asks for %zu bytes of temporary storage for %lld slots, the workspace rule "
                    "allows %zu", what, sort_need, (long long)a.n_slots, a.sort_tmp_bytes);
    HIP_TRY(e);
    return VR_OK;
}

}  // extern "C"
