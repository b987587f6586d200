// query_check -- volrend::query_points / query_grid (include/volrend/query.hpp) on a real GPU.
// Driven by tests/test_gpu_cpp_query.py, which computes the same digests from the CPU oracle.
//
//   query_check <tree.npz> <points.raw> <dirs.raw> <n> <r0> <r1> <r2>
// points / dirs: n x 3 float32 (world coordinates / directions).  Runs query_points on them and
// query_grid over the box -1.2 .. 1.1 with direction dirs[0], every output wanted, and prints one
// "name digest" line per output: digest = sum over the 32-bit words w_i of (w_i + 1) * ((2 i + 1) * K)
// mod 2^64, K = 0x9E3779B97F4A7C15.  Also checks that a refused call throws.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/n3tree.hpp"
#include "volrend/query.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

namespace {

uint64_t digest(const std::vector<uint32_t>& w) {
    uint64_t d = 0;
    for (size_t i = 0; i < w.size(); ++i) d += ((uint64_t)w[i] + 1u) * ((2u * (uint64_t)i + 1u) * 0x9E3779B97F4A7C15ull);
    return d;
}

bool read_floats(const char* path, size_t count, std::vector<float>& out) {
    out.resize(count);
    std::ifstream f(path, std::ios::binary);
    return (bool)f.read(reinterpret_cast<char*>(out.data()), (std::streamsize)(count * sizeof(float)));
}

struct Outputs {
    uint32_t* dev[5] = {};
    size_t words[5] = {};
    int alloc(size_t n, int k) {
        const size_t per[5] = {1, 1, 3, (size_t)k, 3};
        for (int i = 0; i < 5; ++i) {
            words[i] = n * per[i];
            HIP_OK(hipMalloc((void**)&dev[i], words[i] * 4));
            HIP_OK(hipMemset(dev[i], 0xFF, words[i] * 4));
        }
        return 0;
    }
    volrend::QueryOut out() const {
        volrend::QueryOut o;
        o.sigma = (float*)dev[0];
        o.depth = (int32_t*)dev[1];
        o.local = (float*)dev[2];
        o.coeffs = (float*)dev[3];
        o.rgb = (float*)dev[4];
        return o;
    }
    int print(const char* prefix) const {
        static const char* names[5] = {"sigma", "depth", "local", "coeffs", "rgb"};
        for (int i = 0; i < 5; ++i) {
            std::vector<uint32_t> h(words[i]);
            HIP_OK(hipMemcpy(h.data(), dev[i], words[i] * 4, hipMemcpyDeviceToHost));
            printf("%s.%s %016llx\n", prefix, names[i], (unsigned long long)digest(h));
            HIP_OK(hipFree(dev[i]));
        }
        return 0;
    }
};

}  // namespace

int main(int argc, char* argv[]) {
    using namespace volrend;
    if (argc < 8) return 2;
    try {
        N3Tree tree(argv[1]);  // open() + upload
        if (!tree.is_cuda_loaded()) return 3;
        const size_t n = (size_t)atoll(argv[4]);
        const std::array<int32_t, 3> res = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
        std::vector<float> pts, dirs;
        if (!read_floats(argv[2], n * 3, pts) || !read_floats(argv[3], n * 3, dirs)) return 5;
        float *pts_dev = nullptr, *dirs_dev = nullptr;
        HIP_OK(hipMalloc((void**)&pts_dev, n * 12));
        HIP_OK(hipMalloc((void**)&dirs_dev, n * 12));
        HIP_OK(hipMemcpy(pts_dev, pts.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dirs_dev, dirs.data(), n * 12, hipMemcpyHostToDevice));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        const int k = tree.data_dim - 1;

        Outputs a, g;
        if (a.alloc(n, k) || g.alloc((size_t)res[0] * res[1] * res[2], k)) return 4;
        query_points(tree, (int64_t)n, pts_dev, dirs_dev, a.out(), stream);  // world space by default
        query_grid(tree, {-1.2f, -1.2f, -1.2f}, {1.1f, 1.1f, 1.1f}, res, dirs.data(), g.out(), stream,
                   QuerySpace::World);
        HIP_OK(hipStreamSynchronize(stream));
        if (a.print("points") || g.print("grid")) return 4;

        // a refused call throws the way launch_renderer does, with the library's message
        bool threw = false;
        try {
            QueryOut none{};
            query_points(tree, (int64_t)n, pts_dev, nullptr, none, stream, QuerySpace::Tree);
        } catch (const std::runtime_error& e) {
            threw = std::string(e.what()).find("vr_query_points") != std::string::npos;
        }
        printf("throws %d\n", threw ? 1 : 0);
        HIP_OK(hipFree(pts_dev));
        HIP_OK(hipFree(dirs_dev));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
