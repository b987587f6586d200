// vr_values.cpp -- the value passes vr_tree_update_data / vr_tree_read_data (no launch slot, no KParams), and the
// device copies of a tree's host tables, which they share with the march launches (vr_launch.cpp).
#include <hip/hip_runtime.h>

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

// Both value passes: the refusals that need no tree, the two tables (the call's one host-blocking step), the
// values pass and -- after an update of a tree with a lookup structure -- the refresh of its sigma fields
// behind it on the same stream.  No launch slot: the passes hold no per-call scratch.
int tree_data_pass(vr_tree_t t, void* data_dev, int dtype, void* stream, bool update) {
    if (!t || !data_dev) return fail(VR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (dtype != VR_DATA_F16 && dtype != VR_DATA_F32) return fail(VR_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
    DeviceGuard device_guard(t->device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> guard(t->launch_mutex);  // (also orders an update among the launches of other host threads)
    if (int rc = ensure_file_nodes(t)) return rc;
    // the brick-root table (brick -> its node), which the refresh of the bricks reads; trees without bricks have none
    if (t->top_levels > 0 && t->n_bricks > 0)
        if (int rc = ensure_device_table(t, t->brick_root_dev, t->brick_root, (size_t)t->n_bricks, "brick-root")) return rc;
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
    return VR_OK;
}

}  // namespace

extern "C" {

int vr_tree_update_data(vr_tree_t t, const void* data_dev, int dtype, void* stream) {
    return tree_data_pass(t, const_cast<void*>(data_dev), dtype, stream, true);
}

int vr_tree_read_data(vr_tree_t t, void* data_dev, int dtype, void* stream) {
    return tree_data_pass(t, data_dev, dtype, stream, false);
}

}  // extern "C"
