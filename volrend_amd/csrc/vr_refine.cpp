// vr_refine.cpp -- the C ABI of vr_refine_plan / vr_refine_apply (include/volrend_hip.h), host side: argument
// checks, the split of the caller's workspace, the enqueues, and plan's one wait.  No tree handle: the calls work on
// the calling thread's current device.  The kernels and the scan are in vr_refine.hip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "vr_host.h"
#include "vr_refine.h"

namespace {

// What plan and apply both refuse, and the split of the workspace.
int refine_args(const char* what, const VrRefine* r, vr::RefineArgs& a) {
    if (!r || !r->child || !r->sel || !r->workspace) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    if (r->N < 2 || r->N > 16) return fail(VR_ERR_INVALID_ARGUMENT, "%s: N=%d out of range", what, r->N);
    if (r->capacity < 1 || r->capacity > INT32_MAX)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: capacity = %lld outside [1, 2^31)", what, (long long)r->capacity);
    const size_t need = vr::refine_workspace_bytes(r->N, r->capacity);
    if (r->workspace_bytes < 0 || (size_t)r->workspace_bytes < need ||
        reinterpret_cast<uintptr_t>(r->workspace) % vr::kRefineLine != 0)
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: workspace %p of %lld bytes: %zu bytes, 256-byte aligned, are needed",
                    what, r->workspace, (long long)r->workspace_bytes, need);
    memset(&a, 0, sizeof(a));
    a.child = r->child;
    a.sel = r->sel;
    a.capacity = r->capacity;
    a.N3 = r->N * r->N * r->N;
    a.n_slots = r->capacity * a.N3;
    a.words = vr::refine_words(r->N, r->capacity);
    char* w = static_cast<char*>(r->workspace);
    a.mask = reinterpret_cast<uint32_t*>(w);
    w += vr::refine_lines((size_t)a.words * 4);
    a.count = reinterpret_cast<unsigned long long*>(w);
    w += vr::refine_lines((size_t)(a.words + 1) * 8);
    a.first = reinterpret_cast<unsigned long long*>(w);
    w += vr::refine_lines((size_t)(a.words + 1) * 8);
    a.scan_tmp = w;
    a.scan_tmp_bytes = vr::refine_scan_bytes(a.words);
    return VR_OK;
}

}  // namespace

extern "C" {

int64_t vr_refine_workspace(int N, int64_t capacity) {
    if (N < 2 || N > 16 || capacity < 1 || capacity > INT32_MAX) return -1;
    return (int64_t)vr::refine_workspace_bytes(N, capacity);
}

int vr_refine_plan(const VrRefine* r, int64_t* n_new, void* stream) {
    const char* const what = "vr_refine_plan";
    if (!n_new) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL argument", what);
    vr::RefineArgs a;
    if (int rc = refine_args(what, r, a)) return rc;
    *n_new = 0;
    const hipStream_t hs = static_cast<hipStream_t>(stream);
    size_t scan_need = 0;
    const hipError_t e = vr::launch_refine_plan(a, &scan_need, hs);
    if (scan_need > a.scan_tmp_bytes)
        return fail(VR_ERR_UNSUPPORTED, "%s: the scan asks for %zu bytes of temporary storage for %lld words, the "
                    "workspace rule allows %zu", what, scan_need, (long long)a.words, a.scan_tmp_bytes);
    HIP_TRY(e);
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, a.first + a.words, sizeof(total), hipMemcpyDeviceToHost, hs));
    HIP_TRY(hipStreamSynchronize(hs));
    if (total > (unsigned long long)(INT32_MAX - r->capacity))
        return fail(VR_ERR_UNSUPPORTED, "%s: capacity %lld + %llu new nodes exceeds what int32 child words address", what,
                    (long long)r->capacity, total);
    *n_new = (int64_t)total;
    return VR_OK;
}

int vr_refine_apply(const VrRefine* r, void* stream) {
    const char* const what = "vr_refine_apply";
    vr::RefineArgs a;
    if (int rc = refine_args(what, r, a)) return rc;
    if (!r->child_out) return fail(VR_ERR_INVALID_ARGUMENT, "%s: NULL child_out", what);
    if (r->child_out == r->child) return fail(VR_ERR_INVALID_ARGUMENT, "%s: child_out is child (not in place)", what);
    if (r->n_new < 0) return fail(VR_ERR_INVALID_ARGUMENT, "%s: n_new = %lld is negative", what, (long long)r->n_new);
    if (r->n_arrays < 0 || r->n_arrays > VR_REFINE_MAX_ARRAYS || (r->n_arrays > 0 && !r->arrays))
        return fail(VR_ERR_INVALID_ARGUMENT, "%s: n_arrays = %d (0..%d, with arrays)", what, r->n_arrays,
                    VR_REFINE_MAX_ARRAYS);
    vr::RefineArray arrays[VR_REFINE_MAX_ARRAYS];
    for (int i = 0; i < r->n_arrays; ++i) {
        const VrRefineArray& s = r->arrays[i];
        if (s.elem_bytes != 2 && s.elem_bytes != 4)
            return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d].elem_bytes = %d (2 or 4)", what, i, s.elem_bytes);
        if (s.dim < 1) return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d].dim = %d", what, i, s.dim);
        if (s.fill != VR_REFINE_COPY && s.fill != VR_REFINE_ZERO)
            return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d].fill = %d is unknown", what, i, s.fill);
        if (!s.src || !s.dst || s.dst == s.src)
            return fail(VR_ERR_INVALID_ARGUMENT, "%s: arrays[%d]: src and dst are two device arrays", what, i);
        arrays[i] = vr::RefineArray{s.src, s.dst, s.elem_bytes, s.dim, s.fill == VR_REFINE_ZERO};
    }
    if (r->n_new > INT32_MAX - r->capacity)
        return fail(VR_ERR_UNSUPPORTED, "%s: capacity %lld + %lld new nodes exceeds what int32 child words address", what,
                    (long long)r->capacity, (long long)r->n_new);
    if (r->src_slot && a.n_slots > (int64_t)INT32_MAX + 1)
        return fail(VR_ERR_UNSUPPORTED, "%s: src_slot holds int32 slot indices, the tree has %lld slots", what,
                    (long long)a.n_slots);
    a.child_out = r->child_out;
    a.src_slot = r->src_slot;
    a.n_new = r->n_new;
    HIP_TRY(vr::launch_refine_apply(a, arrays, r->n_arrays, static_cast<hipStream_t>(stream)));
    return VR_OK;
}

}  // extern "C"
