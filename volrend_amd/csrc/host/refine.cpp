// refine.cpp -- volrend::refine_plan / refine_apply over vr_refine_plan / vr_refine_apply.
#include "volrend/refine.hpp"

#include "volrend/internal/check.hpp"

namespace volrend {

namespace {

VrRefine to_c(const Refine& r) {
    VrRefine c{};
    c.child = r.child;
    c.sel = r.sel;
    c.workspace = r.workspace;
    c.workspace_bytes = (int64_t)r.workspace_bytes;
    c.capacity = r.capacity;
    c.N = r.N;
    return c;
}

}  // namespace

size_t refine_workspace(int N, int64_t capacity) {
    const int64_t bytes = vr_refine_workspace(N, capacity);
    if (bytes < 0) throw std::runtime_error("vr_refine_workspace: N or capacity out of range");
    return (size_t)bytes;
}

int64_t refine_plan(const Refine& r, void* stream) {
    const VrRefine c = to_c(r);
    int64_t n_new = 0;
    internal::vr_check(vr_refine_plan(&c, &n_new, stream), "vr_refine_plan");
    return n_new;
}

void refine_apply(const Refine& r, int64_t n_new, int32_t* child_out, int32_t* src_slot,
                  const std::vector<RefineArray>& arrays, void* stream) {
    VrRefine c = to_c(r);
    std::vector<VrRefineArray> ca;
    for (const RefineArray& a : arrays)
        ca.push_back(VrRefineArray{a.src, a.dst, a.elem_bytes, a.dim, a.zero ? VR_REFINE_ZERO : VR_REFINE_COPY, 0});
    c.child_out = child_out;
    c.src_slot = src_slot;
    c.n_new = n_new;
    c.arrays = ca.data();
    c.n_arrays = (int32_t)ca.size();
    internal::vr_check(vr_refine_apply(&c, stream), "vr_refine_apply");
}

}  // namespace volrend
