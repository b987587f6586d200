// vr_values.cpp -- the value passes vr_tree_update_data / vr_tree_read_data and the sparse step vr_tree_step (no
// launch slot, no KParams), and the device copies of a tree's host tables, which they share with the march launches (vr_launch.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "vr_host.h"

int ensure_device_table(VrTreeOpaque* t, DeviceBuffer& dev, const std::vector<int32_t>& host, size_t entries,
                        const char* name) {
    if (dev) return VR_OK;
    const size_t bytes = host.size() * sizeof(int32_t);
    if (bytes != entries * sizeof(int32_t)) return fail(VR_ERR_HIP, "the tree carries no %s table", name);
    hipError_t e = dev.alloc(bytes);
    if (e == hipSuccess) e = hipMemcpy(dev.get(), host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)dev.reset();
        return fail(hip_code(e), "%s table of %zu bytes: %s", name, bytes, hipGetErrorString(e));
    }
    t->device_bytes += bytes;
    return VR_OK;
}

int ensure_file_nodes(VrTreeOpaque* t) {
    return ensure_device_table(t, t->file_node_dev, t->file_node, (size_t)t->desc.capacity, "file-order");
}

namespace {

// The tables of a value pass, under the launch mutex (the call's one host-blocking step): the file-order table
// and, for trees with bricks, the brick-root table (brick -> its node), which the refresh of the bricks reads.
int ensure_value_tables(VrTreeOpaque* t) {
    if (int rc = ensure_file_nodes(t)) return rc;
    if (t->top_levels > 0 && t->n_bricks > 0)
        if (int rc = ensure_device_table(t, t->brick_root_dev, t->brick_root, (size_t)t->n_bricks, "brick-root")) return rc;
    return VR_OK;
}

// Both value passes: the refusals that need no tree, the two tables (the call's one host-blocking step), the
// values pass and -- after an update of a tree with a lookup structure -- the refresh of its sigma fields
// behind it on the same stream.  No launch slot: the passes hold no per-call scratch.
int tree_data_pass(vr_tree_t t, void* data_dev, int dtype, void* stream, bool update) {
    if (!t || !data_dev) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (dtype != VR_DATA_F16 && dtype != VR_DATA_F32) return fail(VR_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
    DeviceGuard device_guard(t->device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> guard(t->launch_mutex);  // (also orders an update among the launches of other host threads)
    if (int rc = ensure_value_tables(t)) return rc;
    vr::UpdateArgs a;
    a.nodes = t->arrays[kNodes].get<uint32_t>();
    a.leaves = t->arrays[kLeaves].get<uint16_t>();
    a.file_node = t->file_node_dev.get<int32_t>();
    a.data = data_dev;
    a.capacity = t->desc.capacity;
    a.N3 = t->desc.N * t->desc.N * t->desc.N;
    a.data_dim = t->desc.data_dim;
    a.stride_h = t->leaf_stride_h;
    a.f32 = dtype == VR_DATA_F32;
    if (!update) {
        HIP_TRY(vr::launch_read_values(a, t->n_cus, hs));
        return VR_OK;
    }
    HIP_TRY(vr::launch_update_values(a, t->n_cus, hs));
    if (t->top_levels > 0)
        HIP_TRY(vr::launch_refresh_lookup(a.nodes, t->brick_root_dev.get<int32_t>(), t->n_bricks,
                                          t->arrays[kTop].get<uint2>(), t->arrays[kBricks].get<uint32_t>(),
                                          t->top_levels, t->brick_levels, hs));
    HIP_TRY(refresh_occupancy(t, hs));
    return VR_OK;
}

// What vr_tree_step refuses without following the tree handle.
int validate_step(vr_tree_t t, const VrStep* s) {
    if (!t || !s || !s->master || !s->grad || !s->touched) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->kind != VR_STEP_SGD && s->kind != VR_STEP_ADAM) return fail(VR_ERR_INVALID_ARGUMENT, "unknown kind %d", s->kind);
    if (!std::isfinite(s->lr) || !std::isfinite(s->lr_sigma))
        return fail(VR_ERR_INVALID_ARGUMENT, "lr / lr_sigma must be finite (got %g, %g)", (double)s->lr, (double)s->lr_sigma);
    if (!std::isfinite(s->eps)) return fail(VR_ERR_INVALID_ARGUMENT, "eps must be finite (got %g)", (double)s->eps);
    if (s->kind == VR_STEP_ADAM) {
        if (!s->m || !s->v) return fail(VR_ERR_INVALID_ARGUMENT, "VR_STEP_ADAM: NULL moments (m / v)");
        if (s->step < 1) return fail(VR_ERR_INVALID_ARGUMENT, "VR_STEP_ADAM: step=%d must be at least 1", s->step);
        if (!(s->beta1 >= 0.f && s->beta1 < 1.f) || !(s->beta2 >= 0.f && s->beta2 < 1.f))
            return fail(VR_ERR_INVALID_ARGUMENT, "VR_STEP_ADAM: beta1=%g, beta2=%g outside [0, 1)", (double)s->beta1,
                        (double)s->beta2);
    }
    return VR_OK;
}

}  // namespace

extern "C" {

// The sparse step: the three tables, the values kernel over the bitmap and -- for a tree with a lookup structure --
// the whole refresh of its sigma fields behind it, as tree_data_pass enqueues it behind an update.
int vr_tree_step(vr_tree_t t, const VrStep* s, void* stream) {
    if (int rc = validate_step(t, s)) return rc;
    DeviceGuard device_guard(t->device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> guard(t->launch_mutex);
    if (int rc = ensure_value_tables(t)) return rc;
    if (!t->node_of_file_dev) {  // file node -> device node: the inverse of file_node, built here on the host
        const size_t cap = (size_t)t->desc.capacity;
        if (t->file_node.size() != cap) return fail(VR_ERR_HIP, "the tree carries no file-order table");
        std::vector<int32_t> inverse(cap);
        for (size_t m = 0; m < cap; ++m) inverse[(size_t)t->file_node[m]] = (int32_t)m;
        if (int rc = ensure_device_table(t, t->node_of_file_dev, inverse, cap, "device-order")) return rc;
    }
    vr::StepArgs a;
    a.nodes = t->arrays[kNodes].get<uint32_t>();
    a.leaves = t->arrays[kLeaves].get<uint16_t>();
    a.node_of_file = t->node_of_file_dev.get<int32_t>();
    a.master = s->master;
    a.grad = s->grad;
    a.m = s->m;
    a.v = s->v;
    a.touched = s->touched;
    a.N3 = t->desc.N * t->desc.N * t->desc.N;
    a.n_slots = t->desc.capacity * a.N3;
    a.n_words = (a.n_slots + 31) / 32;
    a.data_dim = t->desc.data_dim;
    a.stride_h = t->leaf_stride_h;
    a.adam = s->kind == VR_STEP_ADAM;
    a.lr = s->lr;
    a.lr_sigma = s->lr_sigma;
    a.beta1 = a.beta2 = a.omb1 = a.omb2 = a.eps = 0.f;
    a.sbc2 = 1.f;
    if (a.adam) {  // four scalars in binary64, each rounded once
        const double b1 = (double)s->beta1, b2 = (double)s->beta2;
        const double bc1 = 1.0 - std::pow(b1, (double)s->step);
        a.beta1 = s->beta1;
        a.beta2 = s->beta2;
        a.omb1 = (float)(1.0 - b1);
        a.omb2 = (float)(1.0 - b2);
        a.sbc2 = (float)std::sqrt(1.0 - std::pow(b2, (double)s->step));
        a.lr = (float)((double)s->lr / bc1);
        a.lr_sigma = (float)((double)s->lr_sigma / bc1);
        a.eps = s->eps;
    }
    if (a.n_words > 0 && a.data_dim > 0) HIP_TRY(vr::launch_step_values(a, t->n_cus, hs));
    if (t->top_levels > 0)
        HIP_TRY(vr::launch_refresh_lookup(a.nodes, t->brick_root_dev.get<int32_t>(), t->n_bricks,
                                          t->arrays[kTop].get<uint2>(), t->arrays[kBricks].get<uint32_t>(),
                                          t->top_levels, t->brick_levels, hs));
    HIP_TRY(refresh_occupancy(t, hs));
    return VR_OK;
}

int vr_tree_update_data(vr_tree_t t, const void* data_dev, int dtype, void* stream) {
    return tree_data_pass(t, const_cast<void*>(data_dev), dtype, stream, true);
}

int vr_tree_read_data(vr_tree_t t, void* data_dev, int dtype, void* stream) {
    return tree_data_pass(t, data_dev, dtype, stream, false);
}

}  // extern "C"
