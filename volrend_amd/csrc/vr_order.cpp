// vr_order.cpp -- the C ABI of vr_order_rays (include/volrend_hip.h), host side: argument checks, the split of the
// caller's workspace, the tree's device, one enqueue.  The kernels and the sort are in vr_order.hip.
#include <hip/hip_runtime.h>

#include <cstring>

#include "vr_host.h"
#include "vr_order.h"

extern "C" {

int64_t vr_order_rays_workspace(int64_t n) { return (int64_t)vr::order_workspace_bytes(n); }

// Enqueue-only, on the tree's device; read-only on the tree: no launch slot, no mutex, as the point queries.
int vr_order_rays(vr_tree_t t, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,
                  const VrRayOrder* out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* const what = "vr_order_rays";
    if (!t || !rays || !rays->origins || !rays->dirs || !opt || !out || !out->order)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (fp_mode != VR_FP_STRICT && fp_mode != VR_FP_FMA)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: unknown fp_mode %d", what, fp_mode);
    if (n < 0 || n >= (1ll << 30))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n=%lld outside [0, 2^30)", what, (long long)n);
    if (out->bits < 0 || out->bits > vr::kOrderMaxBits)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: bits = %d outside [0, %d]", what, out->bits, vr::kOrderMaxBits);
    if ((out->payload != nullptr) != (out->payload_out != nullptr))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: payload and payload_out go together", what);
    if (out->payload ? (out->payload_dim < 1 || out->payload_dim > vr::kOrderMaxPayload) : out->payload_dim != 0)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: payload_dim = %d (1..%d with a payload, 0 without)", what,
                    out->payload_dim, vr::kOrderMaxPayload);
    if (out->origins_out == rays->origins || out->dirs_out == rays->dirs ||
        (out->payload && out->payload_out == out->payload))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: an output is its own input (the gather is not in place)", what);
    if (n == 0) return VR_OK;
    const size_t need = vr::order_workspace_bytes(n);
    if (!workspace || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % vr::kOrderLine != 0)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: workspace %p of %zu bytes: %zu bytes, 256-byte aligned, are needed",
                    what, workspace, workspace_bytes, need);

    vr::OrderArgs a;
    memset(&a, 0, sizeof(a));
    a.bits = out->bits ? out->bits : vr::kOrderDefaultBits;
    a.payload_dim = out->payload_dim;
    char* w = static_cast<char*>(workspace);
    const size_t arr = vr::order_array_bytes(n);
    for (int i = 0; i < 2; ++i) {
        a.key[i] = reinterpret_cast<uint32_t*>(w + (size_t)i * arr);
        a.idx[i] = reinterpret_cast<uint32_t*>(w + (size_t)(2 + i) * arr);
    }
    a.sort_tmp = w + 4 * arr;
    a.sort_tmp_bytes = vr::order_sort_bytes(n);
    a.origins = rays->origins;
    a.dirs = rays->dirs;
    a.order = out->order;
    a.keys = out->keys;
    a.origins_out = out->origins_out;
    a.dirs_out = out->dirs_out;
    a.payload = out->payload;
    a.payload_out = out->payload_out;

    DeviceGuard guard(t->device);
    // what setup_ray_from reads of KParams: the tree's transform and NDC numbers, the box; no rotation, no depth mode
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    fill_tree_params(k, t);
    for (uint32_t*& bm : k.touch) bm = nullptr;
    memcpy(k.bbox, opt->render_bbox, sizeof(k.bbox));
    size_t sort_need = 0;
    const hipError_t e = vr::launch_order(k, vr::RayList{rays->origins, rays->dirs, n}, a, fp_mode, &sort_need,
                                          static_cast<hipStream_t>(stream));
    if (sort_need > a.sort_tmp_bytes)
        return fail(VR_ERR_UNSUPPORTED, "%s: the sort asks for %zu bytes of temporary storage for n = %lld, the workspace "
                    "rule allows %zu", what, sort_need, (long long)n, a.sort_tmp_bytes);
    HIP_TRY(e);
    return VR_OK;
}

}  // extern "C"
