// vr_collapse.cpp -- the C ABI of vr_collapse_plan / vr_collapse_apply (include/volrend_hip.h), host side: argument
// checks, the split of the caller's workspace, the enqueues, and plan's one wait.  No tree handle: the calls work on
// the calling thread's current device.  The kernels and the scan are in vr_collapse.hip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "vr_collapse.h"
#include "vr_host.h"

namespace {

// What plan and apply both refuse, and the split of the workspace.
int collapse_args(const char* what, const VrCollapse* c, vr::CollapseArgs& a) {
    if (!c || !c->child || !c->sel || !c->workspace) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (c->N < 2 || c->N > 16) return fail(VR_ERR_INVALID_ARGUMENT, "%s: N=%d out of range", what, c->N);
    if (c->capacity < 1 || c->capacity > INT32_MAX)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: capacity = %lld outside [1, 2^31)", what, (long long)c->capacity);
    const size_t need = vr::collapse_workspace_bytes(c->capacity);
    if (c->workspace_bytes < 0 || (size_t)c->workspace_bytes < need ||
        reinterpret_cast<uintptr_t>(c->workspace) % vr::kCollapseLine != 0)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: workspace %p of %lld bytes: %zu bytes, 256-byte aligned, are needed",
                    what, c->workspace, (long long)c->workspace_bytes, need);
    memset(&a, 0, sizeof(a));
    a.child = c->child;
    a.sel = c->sel;
    a.capacity = c->capacity;
    a.N3 = c->N * c->N * c->N;
    a.n_slots = c->capacity * a.N3;
    a.words = vr::collapse_words(c->capacity);
    char* w = static_cast<char*>(c->workspace);
    a.col = reinterpret_cast<uint32_t*>(w);
    w += vr::collapse_lines((size_t)a.words * 4);
    a.count = reinterpret_cast<unsigned long long*>(w);
    w += vr::collapse_lines((size_t)(a.words + 1) * 8);
    a.first = reinterpret_cast<unsigned long long*>(w);
    w += vr::collapse_lines((size_t)(a.words + 1) * 8);
    a.into = reinterpret_cast<int32_t*>(w);
    w += vr::collapse_lines((size_t)a.capacity * 4);
    a.scan_tmp = w;
    a.scan_tmp_bytes = vr::collapse_scan_bytes(a.words);
    return VR_OK;
}

}  // namespace

extern "C" {

int64_t vr_collapse_workspace(int N, int64_t capacity) {
    if (N < 2 || N > 16 || capacity < 1 || capacity > INT32_MAX) return -1;
    return (int64_t)vr::collapse_workspace_bytes(capacity);
}

int vr_collapse_plan(const VrCollapse* c, int64_t* n_keep, void* stream) {
    const char* const what = "vr_collapse_plan";
    if (!n_keep) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    vr::CollapseArgs a;
    if (int rc = collapse_args(what, c, a)) return rc;
    *n_keep = 0;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    size_t scan_need = 0;
    const hipError_t e = vr::launch_collapse_plan(a, &scan_need, hs);
    if (scan_need > a.scan_tmp_bytes)
        return fail(VR_ERR_UNSUPPORTED, "%s: the scan asks for %zu bytes of temporary storage for %lld words, the "
                    "workspace rule allows %zu", what, scan_need, (long long)a.words, a.scan_tmp_bytes);
    HIP_TRY(e);
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, a.first + a.words, sizeof(total), hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    *n_keep = (int64_t)total;
    return VR_OK;
}

int vr_collapse_apply(const VrCollapse* c, void* stream) {
    const char* const what = "vr_collapse_apply";
    vr::CollapseArgs a;
    if (int rc = collapse_args(what, c, a)) return rc;
    if (!c->child_out) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL child_out", what);
    if (c->child_out == c->child) return fail(VR_ERR_INVALID_ARGUMENT, "%s: child_out is child (not in place)", what);
    if (c->n_keep < 1 || c->n_keep > c->capacity)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n_keep = %lld outside [1, capacity = %lld]", what, (long long)c->n_keep,
                    (long long)c->capacity);
    if (c->n_arrays < 0 || c->n_arrays > VR_COLLAPSE_MAX_ARRAYS || (c->n_arrays > 0 && !c->arrays))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n_arrays = %d (0..%d, with arrays)", what, c->n_arrays,
                    VR_COLLAPSE_MAX_ARRAYS);
    vr::CollapseArray arrays[VR_COLLAPSE_MAX_ARRAYS];
    bool merges = false;
    for (int i = 0; i < c->n_arrays; ++i) {
        const VrCollapseArray& s = c->arrays[i];
        if (s.elem_bytes != 2 && s.elem_bytes != 4)
            return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d].elem_bytes = %d (2 or 4)", what, i, s.elem_bytes);
        if (s.dim < 1) return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d].dim = %d", what, i, s.dim);
        if (s.rule != VR_COLLAPSE_KEEP && s.rule != VR_COLLAPSE_ZERO && s.rule != VR_COLLAPSE_MEAN)
            return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d].rule = %d is unknown", what, i, s.rule);
        if (!s.src || !s.dst || s.dst == s.src)
            return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d]: src and dst are two device arrays", what, i);
        arrays[i] = vr::CollapseArray{s.src, s.dst, s.elem_bytes, s.dim, s.rule};
        merges = merges || s.rule != VR_COLLAPSE_KEEP;
    }
    if ((c->into_slot || merges) && a.n_slots > (int64_t)INT32_MAX + 1)
        return fail(VR_ERR_UNSUPPORTED, "%s: into_slot (the caller's, or the one ZERO / MEAN arrays go by) holds int32 "
                    "slot indices, the tree has %lld slots", what, (long long)a.n_slots);
    a.child_out = c->child_out;
    a.node_map = c->node_map;
    a.src_node = c->src_node;
    a.into_slot = c->into_slot ? c->into_slot : merges ? a.into : nullptr;
    a.n_keep = c->n_keep;
    HIP_TRY(vr::launch_collapse_apply(a, arrays, c->n_arrays, static_cast<hipStream_t>(stream)));
    return VR_OK;
}

}  // extern "C"
