// sort_floor -- what the bare radix sorts inside one vr_quantize cost: rocprim::radix_sort_pairs of n (uint32 key,
// uint32 value) pairs over the key bits 0 .. 17 + l for l = 0 .. bits - 1, as vr_quantize.hip runs them, with nothing
// around them.  tools/quantize_bench.py builds and runs it.
//
//   sort_floor <n> <bits> <reps>
// Prints one line "level <l> <ms>" per level: the mean over <reps> event-timed sorts after one warm-up.  Keys are a
// fixed hash of the index masked to the level's bits; the sort reads the same unsorted input every time.
// Measurement tooling, not the product.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <rocprim/device/device_radix_sort.hpp>

#define HIP_OK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 4;                                                             \
        }                                                                         \
    } while (0)

__global__ void fill_kernel(uint32_t* keys, uint32_t* vals, unsigned n, uint32_t mask) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint32_t x = i * 0x9e3779b9u + 1u;
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
        keys[i] = x & mask;
        vals[i] = i;
    }
}

int main(int argc, char* argv[]) {
    if (argc < 4) return 2;
    const unsigned n = (unsigned)strtoul(argv[1], nullptr, 10);
    const int bits = atoi(argv[2]), reps = atoi(argv[3]);
    if (n < 1 || bits < 1 || bits > 16 || reps < 1) return 2;
    uint32_t *k_in, *k_out, *v_in, *v_out;
    HIP_OK(hipMalloc((void**)&k_in, (size_t)n * 4));
    HIP_OK(hipMalloc((void**)&k_out, (size_t)n * 4));
    HIP_OK(hipMalloc((void**)&v_in, (size_t)n * 4));
    HIP_OK(hipMalloc((void**)&v_out, (size_t)n * 4));
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    for (int l = 0; l < bits; ++l) {
        const unsigned end = 17u + (unsigned)l;
        hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, nullptr, k_in, v_in, n,
                           end >= 32 ? 0xFFFFFFFFu : (1u << end) - 1u);
        HIP_OK(hipGetLastError());
        size_t bytes = 0;
        HIP_OK(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, n, 0u, end, nullptr));
        void* tmp = nullptr;
        HIP_OK(hipMalloc(&tmp, bytes ? bytes : 4));
        HIP_OK(rocprim::radix_sort_pairs(tmp, bytes, k_in, k_out, v_in, v_out, n, 0u, end, nullptr));
        HIP_OK(hipEventRecord(e0, nullptr));
        for (int r = 0; r < reps; ++r)
            HIP_OK(rocprim::radix_sort_pairs(tmp, bytes, k_in, k_out, v_in, v_out, n, 0u, end, nullptr));
        HIP_OK(hipEventRecord(e1, nullptr));
        HIP_OK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        printf("level %d %.5f\n", l, ms / reps);
        HIP_OK(hipFree(tmp));
    }
    for (void* p : {(void*)k_in, (void*)k_out, (void*)v_in, (void*)v_out}) HIP_OK(hipFree(p));
    return 0;
}
