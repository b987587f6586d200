// weights_check -- volrend::accumulate_weights (include/volrend/weights.hpp) on a real GPU.
// Driven by tests/test_gpu_cpp_weights.py, which computes the same digests from the CPU restatement.
//
//   weights_check <tree.npz> <poses.raw> <n> <width> <height> <focal> <fp_mode>
// poses.raw: n x 12 float32 (column-major 4x3 c2w).  Accumulates the first n / 2 poses and then the others
// into the same zeroed buffers (two calls) and prints "max_weight <digest>" / "hits <digest>":
// digest = sum over the 32-bit words w_i of (w_i + 1) * ((2 i + 1) * K) mod 2^64, K = 0x9E3779B97F4A7C15.
// Also checks that a refused call throws.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/n3tree.hpp"
#include "volrend/weights.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

static uint64_t digest(const std::vector<uint32_t>& w) {
    uint64_t d = 0;
    for (size_t i = 0; i < w.size(); ++i) d += ((uint64_t)w[i] + 1u) * ((2u * (uint64_t)i + 1u) * 0x9E3779B97F4A7C15ull);
    return d;
}

int main(int argc, char* argv[]) {
    using namespace volrend;
    if (argc < 8) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const size_t n = (size_t)atoll(argv[3]);
        std::vector<float> poses(n * 12);
        std::ifstream f(argv[2], std::ios::binary);
        if (!f.read(reinterpret_cast<char*>(poses.data()), (std::streamsize)(poses.size() * sizeof(float)))) return 5;
        Camera cam(atoi(argv[4]), atoi(argv[5]), (float)atof(argv[6]), (float)atof(argv[6]));
        const int fp_mode = atoi(argv[7]);
        const size_t slots = (size_t)tree.capacity * tree.N * tree.N * tree.N;
        LeafWeights out{};
        HIP_OK(hipMalloc((void**)&out.max_weight, slots * 4));
        HIP_OK(hipMalloc((void**)&out.hits, slots * 4));
        HIP_OK(hipMemset(out.max_weight, 0, slots * 4));
        HIP_OK(hipMemset(out.hits, 0, slots * 4));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        RenderOptions opt;
        std::vector<const float*> first, second;
        for (size_t i = 0; i < n; ++i) (i < n / 2 ? first : second).push_back(poses.data() + 12 * i);
        accumulate_weights(tree, cam, {}, opt, out, stream);  // the warm-up call: no pose, no launch
        accumulate_weights(tree, cam, first, opt, out, stream, fp_mode);
        accumulate_weights(tree, cam, second, opt, out, stream, fp_mode);
        HIP_OK(hipStreamSynchronize(stream));
        check_render_status(tree);
        std::vector<uint32_t> h(slots);
        HIP_OK(hipMemcpy(h.data(), out.max_weight, slots * 4, hipMemcpyDeviceToHost));
        printf("max_weight %016llx\n", (unsigned long long)digest(h));
        HIP_OK(hipMemcpy(h.data(), out.hits, slots * 4, hipMemcpyDeviceToHost));
        printf("hits %016llx\n", (unsigned long long)digest(h));

        bool threw = false;
        try {
            accumulate_weights(tree, cam, first, opt, LeafWeights{}, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw = std::string(e.what()).find("vr_accumulate_weights") != std::string::npos;
        }
        printf("throws %d\n", threw ? 1 : 0);
        HIP_OK(hipFree(out.max_weight));
        HIP_OK(hipFree(out.hits));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
