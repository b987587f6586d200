// quantize_check -- volrend::quantize (include/volrend/quantize.hpp) on a real GPU.  Driven by
// tests/test_gpu_cpp_quantize.py, which computes the same digests from the numpy restatement of
// tests/quantize_util.py.
//
//   quantize_check <data.raw> <n_slots> <data_dim> <n_retained> <bits> <sigma_thresh>
// data.raw: n_slots * data_dim binary16 (n_slots even: every output is whole 32-bit words).  Runs quantize on a
// stream of its own with buffers held by DeviceBuffer and prints one "name digest" line per output: digest = sum over
// the 32-bit words w_i of (w_i + 1) * ((2 i + 1) * K) mod 2^64, K = 0x9E3779B97F4A7C15.  Also checks that a refused
// call throws.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "volrend/internal/hip_owners.hpp"
#include "volrend/quantize.hpp"

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

static int print_digest(const char* name, const void* dev, size_t words) {
    std::vector<uint32_t> w(words);
    HIP_OK(hipMemcpy(w.data(), dev, words * 4, hipMemcpyDeviceToHost));
    uint64_t d = 0;
    for (size_t i = 0; i < words; ++i) d += ((uint64_t)w[i] + 1u) * ((2u * (uint64_t)i + 1u) * 0x9E3779B97F4A7C15ull);
    printf("%s %016llx\n", name, (unsigned long long)d);
    return 0;
}

int main(int argc, char* argv[]) {
    using namespace volrend;
    using volrend::internal::DeviceBuffer;
    using volrend::internal::DeviceStream;
    if (argc < 7) return 2;
    const int64_t n_slots = atoll(argv[2]);
    const int dim = atoi(argv[3]), retain = atoi(argv[4]), bits = atoi(argv[5]);
    const float thresh = (float)atof(argv[6]);
    const int n_quant = (dim - 1) / 3 - retain;
    std::vector<uint16_t> data((size_t)n_slots * dim);
    {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f.read(reinterpret_cast<char*>(data.data()), (std::streamsize)(data.size() * 2))) return 5;
    }
    try {
        DeviceStream stream;
        HIP_OK(stream.create(hipStreamNonBlocking));
        DeviceBuffer in, colors, map, sigma, retained, work;
        const size_t color_bytes = (size_t)n_quant * 65536 * 3 * 2, map_bytes = (size_t)n_quant * n_slots * 2;
        const size_t retained_bytes = (size_t)retain * n_slots * 3 * 2;
        const int64_t work_bytes = quantize_workspace(n_slots, dim);
        HIP_OK(in.alloc(data.size() * 2));
        HIP_OK(colors.alloc(color_bytes));
        HIP_OK(map.alloc(map_bytes));
        HIP_OK(sigma.alloc((size_t)n_slots * 2));
        if (retain) HIP_OK(retained.alloc(retained_bytes));
        HIP_OK(work.alloc((size_t)work_bytes));
        HIP_OK(hipMemcpy(in.get(), data.data(), data.size() * 2, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(work.get(), 0x5A, (size_t)work_bytes));
        HIP_OK(hipDeviceSynchronize());

        Quantize q;
        q.data = in.get<uint16_t>();
        q.n_slots = n_slots;
        q.data_dim = dim;
        q.n_retained = retain;
        q.bits = bits;
        q.sigma_thresh = thresh;
        q.quant_colors = colors.get<uint16_t>();
        q.quant_map = map.get<uint16_t>();
        q.sigma = sigma.get<uint16_t>();
        q.data_retained = retain ? retained.get<uint16_t>() : nullptr;
        q.workspace = work.get();
        q.workspace_bytes = work_bytes;
        quantize(q, stream.get());
        HIP_OK(hipStreamSynchronize(stream.get()));
        if (print_digest("quant_colors", colors.get(), color_bytes / 4) || print_digest("quant_map", map.get(), map_bytes / 4) ||
            print_digest("sigma", sigma.get(), (size_t)n_slots / 2) ||
            (retain && print_digest("data_retained", retained.get(), retained_bytes / 4)))
            return 4;

        int threw = 0;
        try {
            Quantize bad = q;
            bad.bits = 17;
            quantize(bad, stream.get());
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("vr_quantize") != std::string::npos &&
                     std::string(e.what()).find("bits") != std::string::npos;
        }
        try {
            Quantize bad = q;
            bad.workspace_bytes -= 1;
            quantize(bad, stream.get());
        } catch (const std::runtime_error& e) {
            threw += std::string(e.what()).find("workspace") != std::string::npos;
        }
        printf("throws %d\n", threw);
    } catch (const std::exception& e) {
        printf("EXCEPTION %s\n", e.what());
        return 3;
    }
    return 0;
}
