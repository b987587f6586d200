// grad_check -- volrend::render_backward (include/volrend/grad.hpp) on a real GPU.
// Driven by tests/test_gpu_cpp_grad.py, which compares the result with the CPU restatement.
//
//   grad_check <tree.npz> <poses.raw> <n> <width> <height> <focal> <fp_mode> <grad_accum.raw> <grad_data.raw>
// poses.raw: n x 12 float32 (column-major 4x3 c2w); grad_accum.raw: n x height x width x 4 float32.
// Adds the first n / 2 poses and then the others into the same zeroed buffer (two calls) and writes it to
// grad_data.raw.  Also checks that a refused call throws.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/grad.hpp"
#include "volrend/n3tree.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

int main(int argc, char* argv[]) {
    using namespace volrend;
    if (argc < 10) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const size_t n = (size_t)atoll(argv[3]);
        std::vector<float> poses(n * 12);
        std::ifstream f(argv[2], std::ios::binary);
        if (!f.read(reinterpret_cast<char*>(poses.data()), (std::streamsize)(poses.size() * sizeof(float)))) return 5;
        Camera cam(atoi(argv[4]), atoi(argv[5]), (float)atof(argv[6]), (float)atof(argv[6]));
        const int fp_mode = atoi(argv[7]);
        const size_t frame = (size_t)cam.width * cam.height * 4;
        std::vector<float> g(n * frame);
        std::ifstream fg(argv[8], std::ios::binary);
        if (!fg.read(reinterpret_cast<char*>(g.data()), (std::streamsize)(g.size() * sizeof(float)))) return 5;
        const size_t elems = (size_t)tree.capacity * tree.N * tree.N * tree.N * tree.data_dim;
        float *g_dev = nullptr, *d_dev = nullptr;
        HIP_OK(hipMalloc((void**)&g_dev, g.size() * 4));
        HIP_OK(hipMalloc((void**)&d_dev, elems * 4));
        HIP_OK(hipMemcpy(g_dev, g.data(), g.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_dev, 0, elems * 4));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        RenderOptions opt;
        std::vector<const float*> first, second;
        for (size_t i = 0; i < n; ++i) (i < n / 2 ? first : second).push_back(poses.data() + 12 * i);
        render_backward(tree, cam, {}, opt, g_dev, d_dev, stream);  // the warm-up call: no pose, no launch
        render_backward(tree, cam, first, opt, g_dev, d_dev, stream, fp_mode);
        render_backward(tree, cam, second, opt, g_dev + first.size() * frame, d_dev, stream, fp_mode);
        HIP_OK(hipStreamSynchronize(stream));
        check_render_status(tree);
        std::vector<float> h(elems);
        HIP_OK(hipMemcpy(h.data(), d_dev, elems * 4, hipMemcpyDeviceToHost));
        std::ofstream out(argv[9], std::ios::binary);
        out.write(reinterpret_cast<const char*>(h.data()), (std::streamsize)(elems * 4));
        printf("elements %zu\n", elems);

        bool threw = false;
        try {
            render_backward(tree, cam, first, opt, nullptr, d_dev, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw = std::string(e.what()).find("vr_render_backward") != std::string::npos;
        }
        printf("throws %d\n", threw ? 1 : 0);
        HIP_OK(hipFree(g_dev));
        HIP_OK(hipFree(d_dev));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
