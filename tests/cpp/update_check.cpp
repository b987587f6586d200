// update_check -- volrend::update_data / read_data (include/volrend/update.hpp) on a real GPU.
// Driven by tests/test_gpu_cpp_update.py, which compares the results with the arrays it wrote.
//
//   update_check <tree.npz> <data.raw> <before_f16.raw> <after_f32.raw> <after_f16.raw>
// data.raw: capacity * N^3 * data_dim binary16 values, the file's indexing.  Reads the uploaded tree back
// (before_f16.raw), writes data.raw into it as binary16 and reads it back as binary32 (after_f32.raw), writes THAT
// into the tree as binary32 and reads it back as binary16 (after_f16.raw); all on one stream, synchronised once.
// Also checks that a refused call throws.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/n3tree.hpp"
#include "volrend/renderer_kernel.hpp"
#include "volrend/update.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

static bool dump(const char* path, const void* dev, size_t bytes) {
    std::vector<char> h(bytes);
    if (hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
    std::ofstream out(path, std::ios::binary);
    out.write(h.data(), (std::streamsize)bytes);
    return (bool)out;
}

int main(int argc, char* argv[]) {
    using namespace volrend;
    if (argc < 6) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const size_t elems = (size_t)tree.capacity * tree.N * tree.N * tree.N * tree.data_dim;
        std::vector<uint16_t> data(elems);
        std::ifstream f(argv[2], std::ios::binary);
        if (!f.read(reinterpret_cast<char*>(data.data()), (std::streamsize)(elems * 2))) return 5;
        uint16_t *in16 = nullptr, *before16 = nullptr, *after16 = nullptr;
        float* after32 = nullptr;
        HIP_OK(hipMalloc((void**)&in16, elems * 2));
        HIP_OK(hipMalloc((void**)&before16, elems * 2));
        HIP_OK(hipMalloc((void**)&after16, elems * 2));
        HIP_OK(hipMalloc((void**)&after32, elems * 4));
        HIP_OK(hipMemcpy(in16, data.data(), elems * 2, hipMemcpyHostToDevice));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        read_data(tree, before16, DataType::F16, stream);
        update_data(tree, in16, DataType::F16, stream);
        read_data(tree, after32, DataType::F32, stream);
        update_data(tree, after32, DataType::F32, stream);
        read_data(tree, after16, DataType::F16, stream);
        HIP_OK(hipStreamSynchronize(stream));
        check_render_status(tree);
        if (!dump(argv[3], before16, elems * 2) || !dump(argv[4], after32, elems * 4) || !dump(argv[5], after16, elems * 2))
            return 6;
        printf("elements %zu\n", elems);

        bool threw = false;
        try {
            update_data(tree, nullptr, DataType::F16, stream);
        } catch (const std::runtime_error& e) {
            threw = std::string(e.what()).find("vr_tree_update_data") != std::string::npos;
        }
        printf("throws %d\n", threw ? 1 : 0);
        HIP_OK(hipFree(in16));
        HIP_OK(hipFree(before16));
        HIP_OK(hipFree(after16));
        HIP_OK(hipFree(after32));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
