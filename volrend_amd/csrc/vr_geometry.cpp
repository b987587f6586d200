// vr_geometry.cpp -- the C ABI of vr_tree_geometry / vr_slot_points (include/volrend_hip.h), host side: argument
// checks and the enqueues.  No tree handle: the calls work on the calling thread's current device, and neither
// waits for anything.  The kernels are in vr_geometry.hip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "vr_geometry.h"
#include "vr_host.h"

namespace {

// What both calls refuse of N and capacity; n_slots on success.
int tree_args(const char* what, int N, int64_t capacity, int64_t& n_slots) {
    if (N < 2 || N > 16) return fail(VR_ERR_INVALID_ARGUMENT, "%s: N=%d out of range", what, N);
    if (capacity < 1 || capacity > INT32_MAX)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: capacity = %lld outside [1, 2^31)", what, (long long)capacity);
    n_slots = capacity * (int64_t)(N * N * N);
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_tree_geometry(const VrGeometry* g, void* stream) {
    const char* const what = "vr_tree_geometry";
    if (!g || !g->child) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (!g->parent_slot && !g->node_depth && !g->node_origin)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: no output is wanted", what);
    vr::GeometryArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = tree_args(what, g->N, g->capacity, a.n_slots)) return rc;
    if (a.n_slots > (int64_t)INT32_MAX + 1)
        return fail(VR_ERR_UNSUPPORTED, "%s: parent links are int32 slot indices, the tree has %lld slots", what,
                    (long long)a.n_slots);
    a.child = g->child;
    a.node_depth = g->node_depth;
    a.node_origin = g->node_origin;
    a.capacity = g->capacity;
    a.N = g->N;
    a.N3 = g->N * g->N * g->N;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    a.parent = g->parent_slot;
    void* tmp = nullptr;  // the parent links of a call that does not want them: stream-ordered, no wait
    if (!a.parent) {
        HIP_TRY(hipMallocAsync(&tmp, (size_t)a.capacity * sizeof(int32_t), hs));
        a.parent = static_cast<int32_t*>(tmp);
    }
    const hipError_t e = vr::launch_tree_geometry(a, hs);
    const hipError_t f = tmp ? hipFreeAsync(tmp, hs) : hipSuccess;  // behind whatever did get enqueued
    HIP_TRY(e);
    HIP_TRY(f);
    return VR_OK;
}

int vr_slot_points(const VrSlotPoints* p, void* stream) {
    const char* const what = "vr_slot_points";
    if (!p) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (!p->points && !p->depth && !p->side) return fail(VR_ERR_INVALID_ARGUMENT, "%s: no output is wanted", what);
    vr::SlotPointsArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = tree_args(what, p->N, p->capacity, a.n_slots)) return rc;
    if (p->n < 0 || p->n > INT32_MAX)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n=%lld outside [0, 2^31)", what, (long long)p->n);
    if (p->k < 1 || p->k > VR_POINTS_MAX_K)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: k=%d outside 1..%d", what, p->k, VR_POINTS_MAX_K);
    if (p->mode != VR_POINTS_CENTER && p->mode != VR_POINTS_JITTER)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: mode = %d is unknown", what, p->mode);
    if (p->n > 0 && (!p->node_depth || !p->node_origin || !p->slots))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL node_depth, node_origin or slots", what);
    if (a.n_slots > (int64_t)INT32_MAX + 1)
        return fail(VR_ERR_UNSUPPORTED, "%s: slots holds int32 slot indices, the tree has %lld slots", what,
                    (long long)a.n_slots);
    if (p->n == 0) return VR_OK;
    a.node_depth = p->node_depth;
    a.node_origin = p->node_origin;
    a.slots = p->slots;
    a.points = p->points;
    a.depth = p->depth;
    a.side = p->side;
    a.n = p->n;
    a.k = p->k;
    a.total = p->n * (int64_t)p->k;
    a.n_chunks = (a.total + 63) / 64;
    a.N = p->N;
    a.N3 = p->N * p->N * p->N;
    a.jitter = p->mode == VR_POINTS_JITTER;
    a.seed = p->seed;
    HIP_TRY(vr::launch_slot_points(a, static_cast<hipStream_t>(stream)));
    return VR_OK;
}

}  // extern "C"
