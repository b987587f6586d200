// step_check -- the marked volrend::render_backward_rays (include/volrend/rays.hpp) and volrend::tree_step
// (include/volrend/step.hpp) on a real GPU.  Driven by tests/test_gpu_cpp_step.py, which compares the results with
// the arrays it expects.
//
//   step_check <tree.npz> <origins.raw> <dirs.raw> <grad_accum.raw> <n> <lr> <lr_sigma> <out prefix>
// The three inputs are float32 [n][3], [n][3], [n][4].  Reads the uploaded tree back as binary32 (the master
// copy), runs the marked backward over the rays into a zeroed gradient and a zeroed bitmap, writes both out
// (<prefix>grad.raw, <prefix>touched.raw), takes one SGD step and writes out master, gradient, bitmap and the
// tree's binary16 values (<prefix>master.raw, grad_after.raw, touched_after.raw, tree.raw); all on one stream.
// Also checks that a refused call throws.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/n3tree.hpp"
#include "volrend/rays.hpp"
#include "volrend/renderer_kernel.hpp"
#include "volrend/step.hpp"
#include "volrend/update.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

static bool dump(const std::string& path, const void* dev, size_t bytes) {
    std::vector<char> h(bytes);
    if (hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
    std::ofstream out(path, std::ios::binary);
    out.write(h.data(), (std::streamsize)bytes);
    return (bool)out;
}

static float* load(const char* path, size_t floats) {
    std::vector<float> h(floats);
    std::ifstream f(path, std::ios::binary);
    if (!f.read(reinterpret_cast<char*>(h.data()), (std::streamsize)(floats * 4))) return nullptr;
    float* d = nullptr;
    if (hipMalloc((void**)&d, floats * 4) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), floats * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

int main(int argc, char* argv[]) {
    using namespace volrend;
    if (argc < 9) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const size_t n = (size_t)atoll(argv[5]);
        const std::string prefix = argv[8];
        const size_t elems = (size_t)tree.capacity * tree.N * tree.N * tree.N * tree.data_dim;
        const size_t words = touched_words(tree);
        float *origins = load(argv[2], n * 3), *dirs = load(argv[3], n * 3), *grad_accum = load(argv[4], n * 4);
        if (!origins || !dirs || !grad_accum) return 5;
        float *master = nullptr, *grad = nullptr;
        uint32_t* touched = nullptr;
        uint16_t* values = nullptr;
        HIP_OK(hipMalloc((void**)&master, elems * 4));
        HIP_OK(hipMalloc((void**)&grad, elems * 4));
        HIP_OK(hipMalloc((void**)&touched, words * 4));
        HIP_OK(hipMalloc((void**)&values, elems * 2));
        HIP_OK(hipMemset(grad, 0, elems * 4));
        HIP_OK(hipMemset(touched, 0, words * 4));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        read_data(tree, master, DataType::F32, stream);
        const Rays rays{origins, dirs, (int64_t)n};
        render_backward_rays(tree, rays, RenderOptions(), grad_accum, grad, touched, stream);
        HIP_OK(hipStreamSynchronize(stream));
        if (!dump(prefix + "grad.raw", grad, elems * 4) || !dump(prefix + "touched.raw", touched, words * 4)) return 6;
        Step s;
        s.master = master;
        s.grad = grad;
        s.touched = touched;
        s.kind = StepKind::SGD;
        s.lr = (float)atof(argv[6]);
        s.lr_sigma = (float)atof(argv[7]);
        tree_step(tree, s, stream);
        read_data(tree, values, DataType::F16, stream);
        HIP_OK(hipStreamSynchronize(stream));
        check_render_status(tree);
        if (!dump(prefix + "master.raw", master, elems * 4) || !dump(prefix + "grad_after.raw", grad, elems * 4) ||
            !dump(prefix + "touched_after.raw", touched, words * 4) || !dump(prefix + "tree.raw", values, elems * 2))
            return 6;
        printf("elements %zu\n", elems);
        printf("words %zu\n", words);

        int threw = 0;
        try {
            s.touched = nullptr;
            tree_step(tree, s, stream);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_tree_step") != std::string::npos;
        }
        try {
            render_backward_rays(tree, rays, RenderOptions(), grad_accum, grad, (uint32_t*)nullptr, stream);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_render_backward_rays_touched") != std::string::npos;
        }
        printf("throws %d\n", threw);
        for (void* p : {(void*)origins, (void*)dirs, (void*)grad_accum, (void*)master, (void*)grad, (void*)touched,
                        (void*)values})
            HIP_OK(hipFree(p));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
