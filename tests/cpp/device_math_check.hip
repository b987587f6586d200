// device_math_check -- volrend_amd/csrc/vr_device_math.h, included as the kernels include it,
// run on the GPU over whole input domains and compared with the CPU oracle's C functions
// (oracle/vr_detmath.h, called through liboracle.so).  Driven by tests/test_gpu_device_math.py,
// which compiles this file with the product's own flags (volrend_amd/build.py FLAGS).
//
//   vr_expf                  every one of the 2^32 float bit patterns
//   vr_expf2                 the same 2^32 patterns in .x, a bijective scramble of them in .y
//   h2f                      every binary16 pattern
//   mul_half / fma_half /    every binary16 pattern, in the low and in the high half of the word
//   mul_add_half             (the other half holds a varying pattern, NaNs included), times a
//                            fixed table of (b, c) operands
//
// Equality is bit for bit, except that any NaN matches any NaN.  One line per check:
//   check <name> total=<n> mismatches=<m>
// followed by up to 8 "  mismatch ..." lines; the exit status is 1 if any check has mismatches.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "vr_device_math.h"

extern "C" float or_expf(float x);            // oracle/vr_oracle.c: vr_det_expf
extern "C" float or_half2float(uint16_t h);   // oracle/vr_oracle.c: vr_half_bits_to_float

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(4);                                                                        \
        }                                                                                   \
    } while (0)

static const int kHostThreads = 16;

// .y input of vr_expf2 for .x = bits: odd multiplier + xor-shift, a bijection of uint32
__host__ __device__ static inline uint32_t partner(uint32_t u) {
    u *= 0x9E3779B1u;
    return u ^ (u >> 15);
}

// the half pattern that shares the word with h
__host__ __device__ static inline uint32_t other_half(uint32_t h, uint32_t j) {
    return (h * 40503u + j * 0x7C01u + 0x7E00u) & 0xFFFFu;
}

__global__ void k_expf(uint32_t base, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = vr::vr_expf(vr::u2f(base + i));
}

__global__ void k_expf2(uint32_t base, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint32_t u = base + i;
        const vr::float2v r = vr::vr_expf2((vr::float2v){vr::u2f(u), vr::u2f(partner(u))});
        out[2 * (size_t)i] = r.x;
        out[2 * (size_t)i + 1] = r.y;
    }
}

__global__ void k_h2f(float* out) {
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h < 65536u) out[h] = vr::h2f((uint16_t)h);
}

// out[((j - j0) * 65536 + h) * 6 + {0..5}] = mul_half<0>, mul_half<1>, fma_half<0>, fma_half<1>,
// mul_add_half<0>, mul_add_half<1> of b[j], c[j] and the half pattern h
__global__ void k_half_ops(const float* b, const float* c, uint32_t j0, uint32_t nj, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nj * 65536u) return;
    const uint32_t h = i & 0xFFFFu, j = j0 + (i >> 16);
    const uint32_t lo = h | (other_half(h, j) << 16), hi = (h << 16) | other_half(h, j);
    const float bj = b[j], cj = c[j];
    float* o = out + (size_t)i * 6;
    o[0] = vr::mul_half<0>(bj, lo);
    o[1] = vr::mul_half<1>(bj, hi);
    o[2] = vr::fma_half<0>(bj, lo, cj);
    o[3] = vr::fma_half<1>(bj, hi, cj);
    o[4] = vr::mul_add_half<0>(bj, lo, cj);
    o[5] = vr::mul_add_half<1>(bj, hi, cj);
}

static inline uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static inline float fl(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline bool same(float a, float b) {
    return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b);
}

struct Check {
    std::string name;
    std::atomic<uint64_t> total{0}, bad{0};
    std::mutex mu;
    std::vector<std::string> first;

    void fail(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        if (bad++ >= 8) return;
        std::lock_guard<std::mutex> g(mu);
        char buf[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        first.push_back(buf);
    }
    bool report() {
        printf("check %s total=%llu mismatches=%llu\n", name.c_str(), (unsigned long long)total.load(),
               (unsigned long long)bad.load());
        for (auto& s : first) printf("  mismatch %s\n", s.c_str());
        fflush(stdout);
        return bad.load() == 0;
    }
};

// runs f(i) for i in [0, n) on kHostThreads threads
template <class F>
static void parallel_for(uint64_t n, F f) {
    std::vector<std::thread> ts;
    for (int t = 0; t < kHostThreads; ++t)
        ts.emplace_back([&, t] {
            const uint64_t a = n * t / kHostThreads, e = n * (t + 1) / kHostThreads;
            for (uint64_t i = a; i < e; ++i) f(i);
        });
    for (auto& th : ts) th.join();
}

static const uint32_t kChunk = 1u << 26;

static bool check_expf() {
    Check ce, ce2;
    ce.name = "vr_expf";
    ce2.name = "vr_expf2";
    float *d1, *d2;
    HIP_OK(hipMalloc(&d1, sizeof(float) * kChunk));
    HIP_OK(hipMalloc(&d2, sizeof(float) * 2 * (size_t)kChunk));
    std::vector<float> h1(kChunk), h2(2 * (size_t)kChunk);
    for (uint64_t base = 0; base < (1ull << 32); base += kChunk) {
        const uint32_t b = (uint32_t)base;
        k_expf<<<kChunk / 256, 256>>>(b, kChunk, d1);
        HIP_OK(hipGetLastError());
        k_expf2<<<kChunk / 256, 256>>>(b, kChunk, d2);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(h1.data(), d1, sizeof(float) * kChunk, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(h2.data(), d2, sizeof(float) * 2 * (size_t)kChunk, hipMemcpyDeviceToHost));
        parallel_for(kChunk, [&](uint64_t i) {
            const uint32_t u = b + (uint32_t)i, v = partner(u);
            const float want_u = or_expf(fl(u)), want_v = or_expf(fl(v));
            if (!same(h1[i], want_u))
                ce.fail("x=0x%08x got=0x%08x want=0x%08x", u, bits(h1[i]), bits(want_u));
            if (!same(h2[2 * i], want_u))
                ce2.fail(".x x=0x%08x (.y 0x%08x) got=0x%08x want=0x%08x", u, v, bits(h2[2 * i]), bits(want_u));
            if (!same(h2[2 * i + 1], want_v))
                ce2.fail(".y x=0x%08x (.x 0x%08x) got=0x%08x want=0x%08x", v, u, bits(h2[2 * i + 1]),
                         bits(want_v));
        });
        ce.total += kChunk;
        ce2.total += 2ull * kChunk;
    }
    HIP_OK(hipFree(d1));
    HIP_OK(hipFree(d2));
    const bool a = ce.report();
    const bool c = ce2.report();
    return a && c;
}

// (b, c) operands: every pair of special values (signed zeros, infinities, NaN, float subnormals,
// magnitudes whose product with the largest / smallest half overflows or underflows) and 300
// random pairs (any bit pattern; moderate magnitudes; a moderate b with a special c)
static void operand_table(std::vector<float>& b, std::vector<float>& c) {
    const float inf = INFINITY, nan = NAN;
    const float special[] = {0.f, -0.f, inf, -inf, nan, fl(0x00000001u), fl(0x80000001u), fl(0x007FFFFFu),
                             fl(0x00400000u), 1.f, -1.f, 3.0e38f, -3.0e38f, 1e34f, 6e33f, 1e-40f,
                             1e-30f, 1e-38f, 1.17549435e-38f, 65504.f, 1.f / 65504.f, 0.5f};
    const int ns = sizeof special / sizeof special[0];
    for (int i = 0; i < ns; ++i)  // every pair of special values
        for (int k = 0; k < ns; ++k) b.push_back(special[i]), c.push_back(special[k]);
    std::mt19937 rng(12345);
    auto any_bits = [&] { return fl(rng()); };  // any exponent, NaNs included
    auto moderate = [&] {
        return std::ldexp(std::uniform_real_distribution<float>(-2.f, 2.f)(rng), (int)(rng() % 60) - 30);
    };
    for (int i = 0; i < 100; ++i) {
        b.push_back(any_bits()), c.push_back(any_bits());
        b.push_back(moderate()), c.push_back(moderate());
        b.push_back(moderate()), c.push_back(special[i % ns]);
    }
}

static bool check_half() {
    Check ch, cm, cf, ca;
    ch.name = "h2f";
    cm.name = "mul_half";
    cf.name = "fma_half";
    ca.name = "mul_add_half";
    bool ok = true;
    {
        float* d;
        HIP_OK(hipMalloc(&d, sizeof(float) * 65536));
        k_h2f<<<256, 256>>>(d);
        HIP_OK(hipGetLastError());
        std::vector<float> h(65536);
        HIP_OK(hipMemcpy(h.data(), d, sizeof(float) * 65536, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d));
        for (uint32_t i = 0; i < 65536; ++i) {
            const float want = or_half2float((uint16_t)i);
            if (!same(h[i], want)) ch.fail("h=0x%04x got=0x%08x want=0x%08x", i, bits(h[i]), bits(want));
        }
        ch.total += 65536;
    }
    std::vector<float> b, c;
    operand_table(b, c);
    const uint32_t n = (uint32_t)b.size(), step = 32;
    std::vector<float> hf(65536);
    for (uint32_t i = 0; i < 65536; ++i) hf[i] = or_half2float((uint16_t)i);
    float *db, *dc, *dout;
    HIP_OK(hipMalloc(&db, sizeof(float) * n));
    HIP_OK(hipMalloc(&dc, sizeof(float) * n));
    HIP_OK(hipMalloc(&dout, sizeof(float) * 6 * 65536 * (size_t)step));
    HIP_OK(hipMemcpy(db, b.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dc, c.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    std::vector<float> out(6 * 65536 * (size_t)step);
    for (uint32_t j0 = 0; j0 < n; j0 += step) {
        const uint32_t nj = n - j0 < step ? n - j0 : step;
        k_half_ops<<<(nj * 65536u + 255) / 256, 256>>>(db, dc, j0, nj, dout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out.data(), dout, sizeof(float) * 6 * 65536 * (size_t)nj, hipMemcpyDeviceToHost));
        parallel_for((uint64_t)nj * 65536, [&](uint64_t i) {
            const uint32_t h = (uint32_t)(i & 0xFFFF), j = j0 + (uint32_t)(i >> 16);
            const float x = hf[h], bj = b[j], cj = c[j];
            const float want_m = bj * x, want_f = std::fma(bj, x, cj);
            const float want_a = bj * x + cj;  // two roundings (-ffp-contract=off)
            const float* o = &out[i * 6];
            for (int hi = 0; hi < 2; ++hi) {
                if (!same(o[hi], want_m))
                    cm.fail("HI=%d h=0x%04x b=0x%08x got=0x%08x want=0x%08x", hi, h, bits(bj), bits(o[hi]),
                            bits(want_m));
                if (!same(o[2 + hi], want_f))
                    cf.fail("HI=%d h=0x%04x b=0x%08x c=0x%08x got=0x%08x want=0x%08x", hi, h, bits(bj), bits(cj),
                            bits(o[2 + hi]), bits(want_f));
                if (!same(o[4 + hi], want_a))
                    ca.fail("HI=%d h=0x%04x b=0x%08x c=0x%08x got=0x%08x want=0x%08x", hi, h, bits(bj), bits(cj),
                            bits(o[4 + hi]), bits(want_a));
            }
        });
        cm.total += 2ull * nj * 65536;
        cf.total += 2ull * nj * 65536;
        ca.total += 2ull * nj * 65536;
    }
    HIP_OK(hipFree(db));
    HIP_OK(hipFree(dc));
    HIP_OK(hipFree(dout));
    printf("operands %u (b, c) pairs\n", n);
    ok &= ch.report();
    ok &= cm.report();
    ok &= cf.report();
    ok &= ca.report();
    return ok;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    bool ok = true;
    if (what == "all" || what == "half") ok &= check_half();
    if (what == "all" || what == "expf") ok &= check_expf();
    return ok ? 0 : 1;
}
