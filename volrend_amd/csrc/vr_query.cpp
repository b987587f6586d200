// vr_query.cpp -- the C ABI of the bulk point queries (include/volrend_hip.h), host side: argument
// checks, the tree's device, one launch.  The kernels are in vr_query.hip.
#include <hip/hip_runtime.h>

#include <cstring>

#include "vr_host.h"
#include "vr_query.h"

namespace {

// What both calls check before they look at the points; fills the outputs of `q`.
int check_outputs(const VrTreeOpaque* t, const VrQueryOut* out, bool have_dirs, int space, vr::QueryArgs& q) {
    if (!out) return fail(VR_ERR_INVALID_ARGUMENT, "out is NULL");
    if (!out->sigma && !out->depth && !out->local && !out->coeffs && !out->rgb)
        return fail(VR_ERR_INVALID_ARGUMENT, "no output is wanted: every pointer of VrQueryOut is NULL");
    if (space != VR_SPACE_WORLD && space != VR_SPACE_TREE)
        return fail(VR_ERR_INVALID_ARGUMENT, "unknown space %d", space);
    if (out->rgb && !have_dirs) return fail(VR_ERR_INVALID_ARGUMENT, "rgb needs directions");
    if (out->rgb && (t->desc.format == VR_FORMAT_SG || t->desc.format == VR_FORMAT_ASG))
        return fail(VR_ERR_UNSUPPORTED, "rgb of SG / ASG trees is not supported by the point queries");
    q.space = space;
    q.sigma = out->sigma;
    q.depth = out->depth;
    q.local = out->local;
    q.coeffs = out->coeffs;
    q.coeffs_vec4 = (t->desc.data_dim - 1) % 4 == 0 && reinterpret_cast<uintptr_t>(out->coeffs) % 16 == 0;
    q.rgb = out->rgb;
    return VR_OK;
}

// Enqueue-only, on the tree's device; read-only on the tree: no launch slot, no mutex (the touch
// bitmaps, the one part of KParams that changes after upload, are not read by these kernels).
int enqueue_query(const VrTreeOpaque* t, const vr::QueryArgs& q, int source, void* stream) {
    DeviceGuard guard(t->device);
    vr::KParams k;
    memset(&k, 0, sizeof(k));
    fill_tree_params(k, t);
    for (uint32_t*& bm : k.touch) bm = nullptr;
    HIP_TRY(vr::launch_query(k, q, source, t->n_cus, static_cast<hipStream_t>(stream)));
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_query_points(vr_tree_t t, int64_t n, const float* xyz_dev, const float* dirs_dev, int space,
                    const VrQueryOut* out, void* stream) {
    if (!t) return fail(VR_ERR_INVALID_ARGUMENT, "tree is NULL");
    if (n < 0) return fail(VR_ERR_INVALID_ARGUMENT, "n = %lld is negative", (long long)n);
    if (!xyz_dev) return fail(VR_ERR_INVALID_ARGUMENT, "xyz is NULL");
    vr::QueryArgs q;
    memset(&q, 0, sizeof(q));
    if (int rc = check_outputs(t, out, dirs_dev != nullptr, space, q)) return rc;
    if (n == 0) return VR_OK;
    q.xyz = xyz_dev;
    q.dirs = dirs_dev;
    q.n = n;
    q.n_chunks = (n + 63) >> 6;
    return enqueue_query(t, q, vr::kPointsArray, stream);
}

int vr_query_grid(vr_tree_t t, const float lo[3], const float hi[3], const int32_t res[3],
                  const float dir[3], int space, const VrQueryOut* out, void* stream) {
    if (!t) return fail(VR_ERR_INVALID_ARGUMENT, "tree is NULL");
    if (!lo || !hi || !res) return fail(VR_ERR_INVALID_ARGUMENT, "lo / hi / res is NULL");
    int64_t cells = 1;
    for (int i = 0; i < 3; ++i) {
        if (res[i] < 1) return fail(VR_ERR_INVALID_ARGUMENT, "res[%d] = %d must be positive", i, res[i]);
        // (each factor < 2^31: the running product is checked before it can overflow)
        if (cells > vr::kMaxGridCells / res[i])
            return fail(VR_ERR_INVALID_ARGUMENT, "res %d x %d x %d exceeds 2^40 cells", res[0], res[1], res[2]);
        cells *= res[i];
    }
    vr::QueryArgs q;
    memset(&q, 0, sizeof(q));
    if (int rc = check_outputs(t, out, dir != nullptr, space, q)) return rc;
    for (int i = 0; i < 3; ++i) {
        q.lo[i] = lo[i];
        const float extent = hi[i] - lo[i];  // one rounding per operator (-ffp-contract=off)
        q.cell[i] = extent / (float)res[i];
        q.res[i] = res[i];
        if (dir) q.dir[i] = dir[i];
    }
    q.k_blocks = (int32_t)(((int64_t)res[2] + 63) / 64);
    q.n = cells;
    q.n_chunks = (int64_t)res[0] * res[1] * q.k_blocks;
    return enqueue_query(t, q, vr::kPointsGrid, stream);
}

}  // extern "C"
