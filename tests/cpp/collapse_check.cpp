// collapse_check -- volrend::collapse_plan / collapse_apply (include/volrend/collapse.hpp) and N3Tree's device-array
// constructor on a real GPU.  Driven by tests/test_gpu_cpp_collapse.py, which compares the results with the numpy
// restatement of tests/collapse_util.py.
//
//   collapse_check <tree.npz> <sel.raw> <master.raw> <out prefix>
// sel.raw: ceil(capacity / 32) uint32 words over NODES; master.raw: capacity * N^3 * data_dim float32.  The tree's
// binary16 values come from read_data.  Writes <prefix>child.raw, <prefix>node_map.raw, <prefix>src_node.raw,
// <prefix>into_slot.raw (int32), <prefix>data.raw (binary16 bits: MEAN), <prefix>master.raw (float32: MEAN),
// <prefix>moment.raw (float32: the master again, ZERO), <prefix>kept.raw (float32: the master again, KEEP) and
// <prefix>reread.raw: read_data of the tree uploaded from the collapsed device arrays.
// Prints `key value` lines; also checks that refused calls throw.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/collapse.hpp"
#include "volrend/n3tree.hpp"
#include "volrend/update.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

template <typename T>
static bool read_raw(const char* path, std::vector<T>& v) {
    std::ifstream f(path, std::ios::binary);
    return (bool)f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

template <typename T>
static int write_device(const std::string& path, const T* dev, size_t count) {
    std::vector<T> h(count);
    HIP_OK(hipMemcpy(h.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)(count * sizeof(T)));
    return 0;
}

int main(int argc, char* argv[]) {
    using namespace volrend;
    if (argc < 5) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const std::string prefix = argv[4];
        const size_t N3 = (size_t)tree.N * tree.N * tree.N, dd = (size_t)tree.data_dim;
        const size_t cap = (size_t)tree.capacity, slots = cap * N3, words = (cap + 31) / 32;
        std::vector<uint32_t> sel(words);
        std::vector<float> master(slots * dd);
        if (!read_raw(argv[2], sel) || !read_raw(argv[3], master)) return 5;
        const internal::NpyArray& cchild = tree.child_;

        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        int32_t* child;
        uint32_t* sel_dev;
        uint16_t* data;
        float* master_dev;
        void* ws;
        const size_t ws_bytes = collapse_workspace(tree.N, tree.capacity);
        HIP_OK(hipMalloc((void**)&child, slots * 4));
        HIP_OK(hipMalloc((void**)&sel_dev, words * 4));
        HIP_OK(hipMalloc((void**)&data, slots * dd * 2));
        HIP_OK(hipMalloc((void**)&master_dev, slots * dd * 4));
        HIP_OK(hipMalloc(&ws, ws_bytes));
        HIP_OK(hipMemcpy(child, cchild.data<int32_t>(), slots * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(sel_dev, sel.data(), words * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(master_dev, master.data(), slots * dd * 4, hipMemcpyHostToDevice));
        read_data(tree, data, DataType::F16, stream);

        Collapse c;
        c.child = child;
        c.sel = sel_dev;
        c.N = tree.N;
        c.capacity = tree.capacity;
        c.workspace = ws;
        c.workspace_bytes = ws_bytes;
        const int64_t n_keep = collapse_plan(c, stream);
        const size_t out_slots = (size_t)n_keep * N3;
        int32_t* child_out;
        CollapseMaps maps;
        uint16_t* data_out;
        float *master_out, *moment_out, *kept_out;
        HIP_OK(hipMalloc((void**)&child_out, out_slots * 4));
        HIP_OK(hipMalloc((void**)&maps.node_map, cap * 4));
        HIP_OK(hipMalloc((void**)&maps.src_node, (size_t)n_keep * 4));
        HIP_OK(hipMalloc((void**)&maps.into_slot, cap * 4));
        HIP_OK(hipMalloc((void**)&data_out, out_slots * dd * 2));
        HIP_OK(hipMalloc((void**)&master_out, out_slots * dd * 4));
        HIP_OK(hipMalloc((void**)&moment_out, out_slots * dd * 4));
        HIP_OK(hipMalloc((void**)&kept_out, out_slots * dd * 4));
        std::vector<CollapseArray> arrays(4);
        arrays[0] = CollapseArray{data, data_out, 2, (int)dd, CollapseRule::Mean};
        arrays[1] = CollapseArray{master_dev, master_out, 4, (int)dd, CollapseRule::Mean};
        arrays[2] = CollapseArray{master_dev, moment_out, 4, (int)dd, CollapseRule::Zero};
        arrays[3] = CollapseArray{master_dev, kept_out, 4, (int)dd, CollapseRule::Keep};
        collapse_apply(c, n_keep, child_out, maps, arrays, stream);
        HIP_OK(hipStreamSynchronize(stream));
        printf("n_keep %lld\n", (long long)n_keep);
        printf("workspace %zu\n", ws_bytes);
        if (write_device(prefix + "child.raw", child_out, out_slots) ||
            write_device(prefix + "node_map.raw", maps.node_map, cap) ||
            write_device(prefix + "src_node.raw", maps.src_node, (size_t)n_keep) ||
            write_device(prefix + "into_slot.raw", maps.into_slot, cap) ||
            write_device(prefix + "data.raw", data_out, out_slots * dd) ||
            write_device(prefix + "master.raw", master_out, out_slots * dd) ||
            write_device(prefix + "moment.raw", moment_out, out_slots * dd) ||
            write_device(prefix + "kept.raw", kept_out, out_slots * dd))
            return 4;

        {   // the collapsed arrays as a tree, without leaving the device
            N3Tree collapsed(tree, child_out, data_out, (int)n_keep);
            VrTreeInfo info;
            if (!collapsed.is_cuda_loaded() || vr_tree_info(collapsed.device, &info) != VR_OK) return 3;
            printf("capacity %lld\n", (long long)info.capacity);
            printf("max_depth %d\n", info.max_depth);
            HIP_OK(hipMemsetAsync(data_out, 0xEE, out_slots * dd * 2, stream));  // (the tree keeps a copy of its own)
            read_data(collapsed, data_out, DataType::F16, stream);
            HIP_OK(hipStreamSynchronize(stream));
            if (write_device(prefix + "reread.raw", data_out, out_slots * dd)) return 4;
        }

        int threw = 0;
        try {
            Collapse bad = c;
            bad.workspace_bytes -= 1;
            collapse_plan(bad, stream);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_collapse_plan") != std::string::npos &&
                     std::string(e.what()).find("workspace") != std::string::npos;
        }
        try {
            collapse_apply(c, n_keep, child, maps, arrays, stream);  // child_out == child
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_collapse_apply") != std::string::npos;
        }
        try {
            std::vector<CollapseArray> bad = arrays;
            bad[1].elem_bytes = 8;
            collapse_apply(c, n_keep, child_out, maps, bad, stream);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("arrays[1]") != std::string::npos;
        }
        try {
            collapse_apply(c, (int64_t)cap + 1, child_out, maps, arrays, stream);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("n_keep") != std::string::npos;
        }
        try {
            collapse_workspace(1, 10);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_collapse_workspace") != std::string::npos;
        }
        printf("throws %d\n", threw);
        for (void* p : {(void*)child, (void*)sel_dev, (void*)data, (void*)master_dev, ws, (void*)child_out,
                        (void*)maps.node_map, (void*)maps.src_node, (void*)maps.into_slot, (void*)data_out,
                        (void*)master_out, (void*)moment_out, (void*)kept_out})
            HIP_OK(hipFree(p));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
