// fit_check -- volrend::fit_rays (include/volrend/rays.hpp) on a real GPU.  Driven by tests/test_gpu_cpp_fit.py,
// which compares the results with the CPU yardsticks.
//
//   fit_check <tree.npz> <origins.raw> <dirs.raw> <n> <fp_mode> <target.raw> <background> <grad_scale> <out prefix>
// origins.raw / dirs.raw / target.raw: n x 3 float32.  Writes <prefix>sq_err.raw (n float32), <prefix>accum.raw
// (n x 4 float32), <prefix>touched.raw (ceil(capacity * N^3 / 32) words) and <prefix>grad.raw (capacity * N^3 *
// data_dim float32).  Also checks that a refused call throws.
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
    if (argc < 10) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const size_t n = (size_t)atoll(argv[4]);
        const int fp_mode = atoi(argv[5]);
        const std::string prefix = argv[9];
        std::vector<float> o(n * 3), d(n * 3), tg(n * 3);
        if (!read_floats(argv[2], o) || !read_floats(argv[3], d) || !read_floats(argv[6], tg)) return 5;
        const size_t slots = (size_t)tree.capacity * tree.N * tree.N * tree.N, elems = slots * tree.data_dim;
        const size_t words = (slots + 31) / 32;
        float *o_dev, *d_dev, *t_dev, *accum, *sq_err, *grad;
        uint32_t* touched;
        HIP_OK(hipMalloc((void**)&o_dev, n * 12));
        HIP_OK(hipMalloc((void**)&d_dev, n * 12));
        HIP_OK(hipMalloc((void**)&t_dev, n * 12));
        HIP_OK(hipMalloc((void**)&accum, n * 16));
        HIP_OK(hipMalloc((void**)&sq_err, n * 4));
        HIP_OK(hipMalloc((void**)&grad, elems * 4));
        HIP_OK(hipMalloc((void**)&touched, words * 4));
        HIP_OK(hipMemcpy(o_dev, o.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_dev, d.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(t_dev, tg.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(grad, 0, elems * 4));
        HIP_OK(hipMemset(touched, 0, words * 4));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        RenderOptions opt;
        opt.background_brightness = (float)atof(argv[7]);
        const Rays all{o_dev, d_dev, (int64_t)n};
        Fit fit;
        fit.target = t_dev;
        fit.grad_scale = (float)atof(argv[8]);
        fit.grad_data = grad;
        fit.touched = touched;
        fit.sq_err = sq_err;
        fit.accum = accum;
        reserve_rays(tree, (int64_t)n, 1);
        fit_rays(tree, Rays{o_dev, d_dev, 0}, opt, fit, stream, fp_mode);  // the warm-up call: launches nothing
        fit_rays(tree, all, opt, fit, stream, fp_mode);
        HIP_OK(hipStreamSynchronize(stream));
        check_render_status(tree);
        if (write_device(prefix + "sq_err.raw", sq_err, n) || write_device(prefix + "accum.raw", accum, n * 4) ||
            write_device(prefix + "touched.raw", touched, words) || write_device(prefix + "grad.raw", grad, elems))
            return 4;
        printf("rays %zu\n", n);

        int threw = 0;
        try {
            Fit bad = fit;
            bad.target = nullptr;
            fit_rays(tree, all, opt, bad, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_fit_rays") != std::string::npos;
        }
        try {
            RenderOptions narrow = opt;
            narrow.basis_minmax[1] = 3;
            fit_rays(tree, all, narrow, fit, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_fit_rays") != std::string::npos &&
                     std::string(e.what()).find("basis_minmax") != std::string::npos;
        }
        printf("throws %d\n", threw);
        for (void* p : {(void*)o_dev, (void*)d_dev, (void*)t_dev, (void*)accum, (void*)sq_err, (void*)grad, (void*)touched})
            HIP_OK(hipFree(p));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
