// collapse.cpp -- volrend::collapse_plan / collapse_apply over vr_collapse_plan / vr_collapse_apply.
#include "volrend/collapse.hpp"

#include "volrend/internal/check.hpp"

namespace volrend {

namespace {

VrCollapse to_c(const Collapse& r) {
    VrCollapse c{};
    c.child = r.child;
    c.sel = r.sel;
    c.workspace = r.workspace;
    c.workspace_bytes = (int64_t)r.workspace_bytes;
    c.capacity = r.capacity;
    c.N = r.N;
    return c;
}

}  // namespace

size_t collapse_workspace(int N, int64_t capacity) {
    const int64_t bytes = vr_collapse_workspace(N, capacity);
    if (bytes < 0) throw std::runtime_error("vr_collapse_workspace: N or capacity out of range");
    return (size_t)bytes;
}

int64_t collapse_plan(const Collapse& r, void* stream) {
    const VrCollapse c = to_c(r);
    int64_t n_keep = 0;
    internal::vr_check(vr_collapse_plan(&c, &n_keep, stream), "vr_collapse_plan");
    return n_keep;
}

void collapse_apply(const Collapse& r, int64_t n_keep, int32_t* child_out, const CollapseMaps& maps,
                    const std::vector<CollapseArray>& arrays, void* stream) {
    VrCollapse c = to_c(r);
    std::vector<VrCollapseArray> ca;
    for (const CollapseArray& a : arrays)
        ca.push_back(VrCollapseArray{a.src, a.dst, a.elem_bytes, a.dim, (int32_t)a.rule, 0});
    c.child_out = child_out;
    c.node_map = maps.node_map;
    c.src_node = maps.src_node;
    c.into_slot = maps.into_slot;
    c.n_keep = n_keep;
    c.arrays = ca.data();
    c.n_arrays = (int32_t)ca.size();
    internal::vr_check(vr_collapse_apply(&c, stream), "vr_collapse_apply");
}

}  // namespace volrend
