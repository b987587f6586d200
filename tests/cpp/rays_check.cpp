// rays_check -- volrend::render_rays / accumulate_weights_rays / render_backward_rays (include/volrend/rays.hpp)
// on a real GPU.  Driven by tests/test_gpu_cpp_rays.py, which compares the results with the CPU yardsticks.
//
//   rays_check <tree.npz> <origins.raw> <dirs.raw> <n> <fp_mode> <grad_accum.raw> <out prefix>
// origins.raw / dirs.raw: n x 3 float32; grad_accum.raw: n x 4 float32.  Writes <prefix>rgba.raw (n x 4 bytes),
// <prefix>accum.raw (n x 4 float32), <prefix>max_weight.raw / <prefix>hits.raw (capacity * N^3 each) and
// <prefix>grad.raw (capacity * N^3 * data_dim float32); the list goes in two calls (the first n / 3 rays, then
// the others) for the weights and the backward.  Also checks that a refused call throws.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/n3tree.hpp"
#include "volrend/rays.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

static bool read_floats(const char* path, std::vector<float>& v) {
    std::ifstream f(path, std::ios::binary);
    return (bool)f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
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
    if (argc < 8) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const size_t n = (size_t)atoll(argv[4]);
        const int fp_mode = atoi(argv[5]);
        const std::string prefix = argv[7];
        std::vector<float> o(n * 3), d(n * 3), g(n * 4);
        if (!read_floats(argv[2], o) || !read_floats(argv[3], d) || !read_floats(argv[6], g)) return 5;
        const size_t slots = (size_t)tree.capacity * tree.N * tree.N * tree.N, elems = slots * tree.data_dim;
        float *o_dev, *d_dev, *g_dev, *accum, *mw, *grad;
        uint32_t *rgba, *hits;
        HIP_OK(hipMalloc((void**)&o_dev, n * 12));
        HIP_OK(hipMalloc((void**)&d_dev, n * 12));
        HIP_OK(hipMalloc((void**)&g_dev, n * 16));
        HIP_OK(hipMalloc((void**)&accum, n * 16));
        HIP_OK(hipMalloc((void**)&rgba, n * 4));
        HIP_OK(hipMalloc((void**)&mw, slots * 4));
        HIP_OK(hipMalloc((void**)&hits, slots * 4));
        HIP_OK(hipMalloc((void**)&grad, elems * 4));
        HIP_OK(hipMemcpy(o_dev, o.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_dev, d.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(g_dev, g.data(), n * 16, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(mw, 0, slots * 4));
        HIP_OK(hipMemset(hits, 0, slots * 4));
        HIP_OK(hipMemset(grad, 0, elems * 4));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        RenderOptions opt;
        const Rays all{o_dev, d_dev, (int64_t)n};
        const size_t k = n / 3;
        const Rays head{o_dev, d_dev, (int64_t)k}, tail{o_dev + 3 * k, d_dev + 3 * k, (int64_t)(n - k)};
        reserve_rays(tree, (int64_t)n, 1);
        render_rays(tree, all, opt, rgba, accum, stream, fp_mode);
        const LeafWeights lw{mw, hits};
        accumulate_weights_rays(tree, Rays{o_dev, d_dev, 0}, opt, lw, stream, fp_mode);  // the warm-up call
        accumulate_weights_rays(tree, head, opt, lw, stream, fp_mode);
        accumulate_weights_rays(tree, tail, opt, lw, stream, fp_mode);
        render_backward_rays(tree, head, opt, g_dev, grad, stream, fp_mode);
        render_backward_rays(tree, tail, opt, g_dev + 4 * k, grad, stream, fp_mode);
        HIP_OK(hipStreamSynchronize(stream));
        check_render_status(tree);
        if (write_device(prefix + "rgba.raw", rgba, n) || write_device(prefix + "accum.raw", accum, n * 4) ||
            write_device(prefix + "max_weight.raw", mw, slots) || write_device(prefix + "hits.raw", hits, slots) ||
            write_device(prefix + "grad.raw", grad, elems))
            return 4;
        printf("rays %zu\n", n);

        int threw = 0;
        try {
            render_rays(tree, all, opt, nullptr, nullptr, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_render_rays") != std::string::npos;
        }
        try {
            render_backward_rays(tree, all, opt, nullptr, grad, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_render_backward_rays") != std::string::npos;
        }
        printf("throws %d\n", threw);
        for (void* p : {(void*)o_dev, (void*)d_dev, (void*)g_dev, (void*)accum, (void*)rgba, (void*)mw, (void*)hits,
                        (void*)grad})
            HIP_OK(hipFree(p));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
