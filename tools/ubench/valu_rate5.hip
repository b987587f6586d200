// valu_rate5 -- does a wave issue INDEPENDENT vector instructions faster than DEPENDENT ones on gfx950?
// The shade round's dot products are v_fma_mix_f32 + v_add_f32 pairs on one accumulator per colour channel
// (vr_device_math.h mul_add_half).  Three orders of the same 3 x 32 pairs per loop body:
//   chain1       channel 0's 32 pairs, then channel 1's, then channel 2's: every instruction reads the result of
//                the one before it
//   chain3       per coefficient three products, then three sums (a three-channel unit): a result is read
//                three instructions after it was issued
//   chain3_pairs product, sum, product, sum, ... rotating over the channels: a sum right behind its product, the
//                accumulator three pairs old
// at 1 wave per SIMD (the wave is alone: what a wave's own dependent path costs) and at 5 (the SH16 flavour's
// occupancy: the other waves fill the gaps).  Wall clock over the grid; prints SIMD clocks per instruction per
// WAVE at a nominal 2.2 GHz -- the ratios between the cases are what is read.
#include <hip/hip_runtime.h>

#include <cstdio>

#define REP8(x) x x x x x x x x
#define REP32(x) REP8(x) REP8(x) REP8(x) REP8(x)
// %0..%2 accumulators, %3..%5 products, %6 b, %7..%9 packed words, %10 = -0.0 (scalar)
#define MIX(t, w) "v_fma_mix_f32 %" #t ", %6, %" #w ", %10 op_sel_hi:[0,1,0]\n"
#define ADD(c, t) "v_add_f32 %" #c ", %" #t ", %" #c "\n"
#define OPERANDS                                                                                      \
    : "+v"(c0), "+v"(c1), "+v"(c2), "=&v"(t0), "=&v"(t1), "=&v"(t2)                                  \
    : "v"(b), "v"(w0), "v"(w1), "v"(w2), "s"(0x80000000u)
#define PAIR(c, t, w) MIX(t, w) ADD(c, t)
#define BODY_CHAIN1                                            \
    asm volatile(REP32(PAIR(0, 3, 7)) OPERANDS);               \
    asm volatile(REP32(PAIR(1, 4, 8)) OPERANDS);               \
    asm volatile(REP32(PAIR(2, 5, 9)) OPERANDS);
#define UNIT3 MIX(3, 7) MIX(4, 8) MIX(5, 9) ADD(0, 3) ADD(1, 4) ADD(2, 5)
#define BODY_CHAIN3 asm volatile(REP32(UNIT3) OPERANDS);
#define BODY_CHAIN3_PAIRS asm volatile(REP32(PAIR(0, 3, 7) PAIR(1, 4, 8) PAIR(2, 5, 9)) OPERANDS);

#define DEFK(NAME, BODY)                                                                  \
    __global__ void NAME(float* out, int iters) {                                         \
        float c0 = threadIdx.x, c1 = c0 + 1.f, c2 = c0 + 2.f, t0, t1, t2, b = 0.5f;       \
        unsigned w0 = 0x3c003800u + threadIdx.x, w1 = w0 + 1u, w2 = w0 + 2u;              \
        for (int i = 0; i < iters; ++i) { BODY }                                          \
        out[blockIdx.x * blockDim.x + threadIdx.x] = c0 + c1 + c2;                        \
    }
DEFK(k_chain1, BODY_CHAIN1) DEFK(k_chain3, BODY_CHAIN3) DEFK(k_chain3_pairs, BODY_CHAIN3_PAIRS)

template <typename K>
void run(const char* name, K kern, int waves) {
    hipDeviceProp_t prop;
    (void)hipGetDeviceProperties(&prop, 0);
    const int iters = 2048, blocks = prop.multiProcessorCount * waves;  // a 256-thread block: one wave per SIMD of a CU
    float* out;
    (void)hipMalloc(&out, (size_t)blocks * 256 * 4);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, out, iters);
    (void)hipDeviceSynchronize();
    float best = 1e9f;
    for (int rep = 0; rep < 5; ++rep) {
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, out, iters);
        (void)hipEventRecord(e1);
        (void)hipDeviceSynchronize();
        float ms;
        (void)hipEventElapsedTime(&ms, e0, e1);
        best = ms < best ? ms : best;
    }
    const double n_inst = (double)iters * 32 * 6;  // per wave
    printf("{\"case\": \"%s\", \"waves_per_simd\": %d, \"ns_per_inst_per_wave\": %.3f, "
           "\"clocks_per_inst_per_wave_at_2p2GHz\": %.2f, \"clocks_per_inst_per_simd_at_2p2GHz\": %.2f}\n",
           name, waves, best * 1e6 / n_inst, best * 1e6 / n_inst * 2.2, best * 1e6 / n_inst * 2.2 / waves);
    (void)hipFree(out);
}

int main() {
    for (int waves : {1, 5}) {
        run("chain1", k_chain1, waves);
        run("chain3", k_chain3, waves);
        run("chain3_pairs", k_chain3_pairs, waves);
    }
    return 0;
}
