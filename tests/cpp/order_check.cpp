// order_check -- volrend::order_rays (include/volrend/rays.hpp) on a real GPU.  Driven by tests/test_gpu_cpp_order.py,
// which compares the results with the restatement of the key (tests/cpp/order_restatement.c) and the result rule.
//
//   order_check <tree.npz> <origins.raw> <dirs.raw> <n> <fp_mode> <bits> <payload.raw> <payload_dim> <out prefix>
// origins.raw / dirs.raw: n x 3 float32; payload.raw: n x payload_dim float32.  Writes <prefix>order.raw and
// <prefix>keys.raw (n uint32), <prefix>origins.raw / <prefix>dirs.raw (n x 3 float32) and <prefix>payload.raw.
// Prints `key value` lines; also checks that a refused call throws and that n == 0 enqueues nothing.
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
        const int fp_mode = atoi(argv[5]), bits = atoi(argv[6]), dim = atoi(argv[8]);
        const std::string prefix = argv[9];
        std::vector<float> o(n * 3), d(n * 3), pl(n * dim);
        if (!read_floats(argv[2], o) || !read_floats(argv[3], d) || !read_floats(argv[7], pl)) return 5;
        const size_t ws_bytes = order_rays_workspace((int64_t)n);
        float *o_dev, *d_dev, *p_dev, *o_out, *d_out, *p_out;
        uint32_t *order, *keys;
        void* ws;
        HIP_OK(hipMalloc((void**)&o_dev, n * 12));
        HIP_OK(hipMalloc((void**)&d_dev, n * 12));
        HIP_OK(hipMalloc((void**)&p_dev, n * dim * 4));
        HIP_OK(hipMalloc((void**)&o_out, n * 12));
        HIP_OK(hipMalloc((void**)&d_out, n * 12));
        HIP_OK(hipMalloc((void**)&p_out, n * dim * 4));
        HIP_OK(hipMalloc((void**)&order, n * 4));
        HIP_OK(hipMalloc((void**)&keys, n * 4));
        HIP_OK(hipMalloc(&ws, ws_bytes));
        HIP_OK(hipMemcpy(o_dev, o.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_dev, d.data(), n * 12, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(p_dev, pl.data(), n * dim * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(order, 0xEE, n * 4));
        hipStream_t stream;
        HIP_OK(hipStreamCreate(&stream));
        RenderOptions opt;
        const Rays all{o_dev, d_dev, (int64_t)n};
        RayOrder out;
        out.bits = bits;
        out.order = order;
        out.keys = keys;
        out.origins_out = o_out;
        out.dirs_out = d_out;
        out.payload = p_dev;
        out.payload_out = p_out;
        out.payload_dim = dim;
        order_rays(tree, Rays{o_dev, d_dev, 0}, opt, out, nullptr, 0, stream, fp_mode);  // no ray: nothing is enqueued
        HIP_OK(hipStreamSynchronize(stream));
        uint32_t first = 0;
        HIP_OK(hipMemcpy(&first, order, 4, hipMemcpyDeviceToHost));
        printf("untouched %d\n", first == 0xEEEEEEEEu);
        order_rays(tree, all, opt, out, ws, ws_bytes, stream, fp_mode);
        HIP_OK(hipStreamSynchronize(stream));
        if (write_device(prefix + "order.raw", order, n) || write_device(prefix + "keys.raw", keys, n) ||
            write_device(prefix + "origins.raw", o_out, n * 3) || write_device(prefix + "dirs.raw", d_out, n * 3) ||
            write_device(prefix + "payload.raw", p_out, n * dim))
            return 4;
        printf("rays %zu\n", n);
        printf("workspace %zu\n", ws_bytes);

        int threw = 0;
        try {
            order_rays(tree, all, opt, out, ws, ws_bytes - 1, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_order_rays") != std::string::npos &&
                     std::string(e.what()).find("workspace") != std::string::npos;
        }
        try {
            RayOrder bad = out;
            bad.bits = 6;
            order_rays(tree, all, opt, bad, ws, ws_bytes, stream, fp_mode);
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("bits") != std::string::npos;
        }
        printf("throws %d\n", threw);
        for (void* p : {(void*)o_dev, (void*)d_dev, (void*)p_dev, (void*)o_out, (void*)d_out, (void*)p_out, (void*)order,
                        (void*)keys, ws})
            HIP_OK(hipFree(p));
        HIP_OK(hipStreamDestroy(stream));
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
