// device_forms_check -- the arithmetic forms the kernels rest on, run on the GPU over whole operand domains and
// compared with the CPU oracle (liboracle.so) and with the same C expression under the oracle's flags
// (tests/cpp/forms_reference.c).  The product headers are included unchanged and this file is compiled with the
// product's own flags (volrend_amd/build.py FLAGS), so what -ffp-contract=off and
// -fno-gpu-flush-denormals-to-zero make of a division, a square root or an FP64 product is what is under test.
// Driven by tests/test_gpu_device_forms.py.
//
//   sweep [others_every]
//           every one of the 2^32 float bit patterns x, all forms in one pass (words of device_forms.h); with an odd
//           others_every > 1 only expf_nonan, quant8, recip, sqrt and n2_axis take every pattern and the other
//           forms take the multiples of others_every (the host reference is what the pass costs):
//             expf_nonan     vr_expf_nonan against or_expf, every non-NaN pattern
//             sigmoid        sigmoid(x) of vr_dev_shade.h
//             sigmoid2       weighted_sigmoid2(1, x, partner(x)), both components
//             quant8         quant8(x)
//             recip, sqrt, floor, invdir      1.f / x, sqrtf, floorf, (float)(1.0 / ((double)x + 1e-9))
//             n2_axis        what query_n2 does to one coordinate (clamp by median, digits from one conversion,
//                            local coordinate by fract) against the literal float recurrence, every non-NaN x
//             ldexp_div      ldexp(x, -k) against x / 2^k: every x with a k drawn from its pattern, and every
//                            k = 0..31 for every x with a biased exponent <= 32 (all subnormal quotients)
//             div            a / x for four dividends, and a / b over every pair of table values
//   table   byte_over_255, box_t (the FP64 slab products of the ray / box test), both FP models of dda_unit,
//           norm3, normalize3, mv3, dot3, cross3 over 2^22 seeded operand sets, and precalc_basis in every
//           form the kernels instantiate over a lattice of directions plus degenerate ones
//
// Equality is bit for bit, except that any NaN matches any NaN.  One line per check:
//   check <name> total=<n> mismatches=<m>
// followed by up to 8 "  mismatch ..." lines; the exit status is 1 if any check has mismatches.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "vr_internal.h"
#include "vr_device_math.h"
#include "vr_dev_shade.h"
#include "vr_dev_query.h"

#include "device_forms.h"

// oracle/vr_oracle.h (C; OrTree is declared there)
extern "C" {
#include "vr_oracle.h"
}
// tests/cpp/forms_reference.c
extern "C" {
int ref_keeps_subnormals(void);
uint32_t ref_n2_axis(float x, uint32_t* u, float* local);
float ref_ldexp_div(float x, int k);
uint32_t ref_ldexp_fold(float x);
float ref_div(float a, float b);
float ref_byte_over_255(int b);
float ref_box_t(float b, float c, float inv, int sign);
void ref_sweep(uint32_t base, uint32_t n, uint32_t stride, uint32_t others_every, uint32_t* out);
}

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(4);                                                                        \
        }                                                                                   \
    } while (0)

static const int kHostThreads = 16;

// ---------------------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------------------

__global__ void k_subnormals(uint32_t* out) {
    volatile float tiny = 1e-40f, one = 1.f;
    out[0] = tiny * one != 0.f;
}

// query_n2 on one coordinate (vr_dev_query.h:67-77 and 137-140), with its builtins: the clamped coordinate's
// integer digits, and the local coordinate of a leaf at depth d
__device__ __forceinline__ float n2_clamp(float x) {
    const float hi = 1.f - 1e-6f;
    return __builtin_amdgcn_fmed3f(x, 0.f, hi);
}
__device__ __forceinline__ float n2_local(float c, int d) {
    const float cs = vr::u2f((uint32_t)(127 + d) << 23);  // 2^d
    return __builtin_amdgcn_fractf(c * cs);
}

// out[w * n + i] = word w (device_forms.h) of pattern base + i
__global__ void k_sweep(uint32_t base, uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t u = base + i;
    const float x = vr::u2f(u), y = vr::u2f(forms_partner(u));
    uint32_t* o = out + i;
    o[(size_t)W_EXPF_NONAN * n] = vr::f2u(vr::vr_expf_nonan(-x));
    o[(size_t)W_SIGMOID * n] = vr::f2u(vr::sigmoid(x));
    const vr::float2v s = vr::weighted_sigmoid2(1.f, x, y);
    o[(size_t)W_SIGMOID2_X * n] = vr::f2u(s.x);
    o[(size_t)W_SIGMOID2_Y * n] = vr::f2u(s.y);
    o[(size_t)W_QUANT8 * n] = vr::quant8(x);
    o[(size_t)W_RECIP * n] = vr::f2u(1.f / x);
    o[(size_t)W_SQRT * n] = vr::f2u(__builtin_sqrtf(x));
    o[(size_t)W_FLOOR * n] = vr::f2u(__builtin_floorf(x));
    o[(size_t)W_INVDIR * n] = vr::f2u((float)(1.0 / ((double)x + 1e-9)));
    const float c = n2_clamp(x);
    o[(size_t)W_N2_U * n] = (uint32_t)(c * 16777216.f);
    uint32_t fold = 0;
#pragma unroll
    for (int d = 1; d <= 24; ++d) fold += forms_rotl(vr::f2u(n2_local(c, d)), d);
    o[(size_t)W_N2_FOLD * n] = fold;
    o[(size_t)W_LDEXP * n] = vr::f2u(__builtin_amdgcn_ldexpf(x, -forms_k(u)));
#pragma unroll
    for (int j = 0; j < 4; ++j) o[(size_t)(W_DIV0 + j) * n] = vr::f2u(vr::u2f(forms_div_a_bits(j)) / x);
}

// x = pattern base + i with the sign bit `sign`: sum over k = 0..31 of rotl(bits(ldexp(x, -k)), k)
__global__ void k_ldexp_fold(uint32_t base, uint32_t n, uint32_t sign, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = vr::u2f((base + i) | sign);
    uint32_t fold = 0;
    for (int k = 0; k < 32; ++k) fold += forms_rotl(vr::f2u(__builtin_amdgcn_ldexpf(x, -k)), k);
    out[i] = fold;
}

// the terms of the two folds for one x, for the report of a mismatch: 24 local coordinates, 32 quotients
__global__ void k_fold_terms(float x, float* out) {
    const float c = n2_clamp(x);
    for (int d = 1; d <= 24; ++d) out[d - 1] = n2_local(c, d);
    for (int k = 0; k < 32; ++k) out[24 + k] = __builtin_amdgcn_ldexpf(x, -k);
}

__global__ void k_div_pairs(const float* v, uint32_t nv, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nv * nv) out[i] = v[i / nv] / v[i % nv];
}

__global__ void k_byte(float* out) {
    const uint32_t b = threadIdx.x;
    out[b] = (float)(uint8_t)b / 255.f;
}

// vr_dev_rays.h setup_ray_from, the FP64 ray / box products: out[2 i], out[2 i + 1] = lower, upper slab of the
// triple i = (b, c, inv) of v^3
__global__ void k_box_t(const float* v, uint32_t nv, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv * nv * nv) return;
    const float b = v[i / (nv * nv)], c = v[(i / nv) % nv], inv = v[i % nv];
    out[2 * (size_t)i] = (float)((((double)b + 1e-6) - (double)c) * (double)inv);
    out[2 * (size_t)i + 1] = (float)((((double)b - 1e-6) - (double)c) * (double)inv);
}

// One operand set = 15 floats: m[9], v[3], w[3].  12 results: dda_unit(v, w), norm3(v), normalize3(v) x 3,
// mv3(m, v) x 3, dot3(v, w), cross3(v, w) x 3.
static const int kVecIn = 15, kVecOut = 12;
template <int FMA>
__global__ void k_vec(const float* in, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a[kVecIn];
    for (int j = 0; j < kVecIn; ++j) a[j] = in[(size_t)i * kVecIn + j];
    const float *m = a, *v = a + 9, *w = a + 12;
    float* o = out + (size_t)i * kVecOut;
    o[0] = vr::dda_unit<FMA>(v, w);
    o[1] = vr::norm3<FMA>(v);
    float nv[3] = {v[0], v[1], v[2]};
    vr::normalize3<FMA>(nv);
    for (int j = 0; j < 3; ++j) o[2 + j] = nv[j];
    vr::mv3<FMA>(m, v, o + 5);
    o[8] = vr::dot3<FMA>(v, w);
    vr::cross3<FMA>(v, w, o + 9);
}

template <int FMA, bool LOBES, int BD>
__global__ void k_basis(vr::KParams p, const float* dirs, uint32_t n, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float dir[3] = {dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]};
    float b[VR_MAX_BASIS];
#pragma unroll
    for (int j = 0; j < VR_MAX_BASIS; ++j) b[j] = 0.f;
    vr::precalc_basis<FMA, LOBES, BD>(p, dir, b);
#pragma unroll
    for (int j = 0; j < VR_MAX_BASIS; ++j) out[(size_t)i * VR_MAX_BASIS + j] = b[j];
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------

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
static inline bool is_nan_bits(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }
static inline bool same_bits(uint32_t a, uint32_t b) { return a == b || (is_nan_bits(a) && is_nan_bits(b)); }
static inline bool same(float a, float b) { return same_bits(bits(a), bits(b)); }

struct Check {
    std::string name;
    std::atomic<uint64_t> total{0}, bad{0};
    std::mutex mu;
    std::vector<std::string> first;

    explicit Check(const char* n) : name(n) {}
    void fail(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        if (bad++ >= 8) return;
        std::lock_guard<std::mutex> g(mu);
        char buf[320];
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

// runs f(a, e) on kHostThreads threads, [a, e) being thread t's share of [0, n) in pieces of at most `piece`
template <class F>
static void parallel_pieces(uint64_t n, uint64_t piece, F f) {
    std::vector<std::thread> ts;
    for (int t = 0; t < kHostThreads; ++t)
        ts.emplace_back([&, t] {
            const uint64_t a = n * t / kHostThreads, e = n * (t + 1) / kHostThreads;
            for (uint64_t i = a; i < e; i += piece) f(i, i + piece < e ? i + piece : e);
        });
    for (auto& th : ts) th.join();
}
template <class F>
static void parallel_for(uint64_t n, F f) {
    parallel_pieces(n, 1u << 16, [&](uint64_t a, uint64_t e) {
        for (uint64_t i = a; i < e; ++i) f(i);
    });
}

struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void report(const char* what) {
        printf("seconds %s %.2f\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        fflush(stdout);
    }
};

template <class T>
static T* device_copy(const std::vector<T>& h) {
    T* d;
    HIP_OK(hipMalloc(&d, sizeof(T) * h.size()));
    HIP_OK(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return d;
}
template <class T>
static std::vector<T> host_copy(const T* d, size_t n) {
    std::vector<T> h(n);
    HIP_OK(hipMemcpy(h.data(), d, sizeof(T) * n, hipMemcpyDeviceToHost));
    return h;
}
static unsigned blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

// A flushed mode on either side would turn the subnormal cases of every sweep into 0 == 0.
static void require_subnormals() {
    uint32_t* d;
    HIP_OK(hipMalloc(&d, 4));
    k_subnormals<<<1, 1>>>(d);
    HIP_OK(hipGetLastError());
    const uint32_t dev = host_copy(d, 1)[0];
    HIP_OK(hipFree(d));
    if (!dev || !ref_keeps_subnormals()) {
        fprintf(stderr, "binary32 subnormals are flushed (device keeps them: %u, host keeps them: %d)\n", dev,
                ref_keeps_subnormals());
        exit(3);
    }
}

// the terms of the folds of one x as the device forms them (k_fold_terms)
static std::vector<float> fold_terms(float x) {
    float* d;
    HIP_OK(hipMalloc(&d, sizeof(float) * 56));
    k_fold_terms<<<1, 1>>>(x, d);
    HIP_OK(hipGetLastError());
    std::vector<float> h = host_copy(d, 56);
    HIP_OK(hipFree(d));
    return h;
}

// ---- sweep ---------------------------------------------------------------------------------------------

static bool check_div_pairs(Check& c_div);  // (with the tables, below)

static const uint32_t kChunk = 1u << 23;  // patterns per pass of k_sweep: 2 x 512 MB of results in flight
static const uint32_t kPiece = 2048;      // patterns per call of ref_sweep (its scratch stays in the L2)
static const uint32_t kRow = kPiece + 16;  // words between the rows of that scratch: no multiple of 4 KB

// every x whose biased exponent is <= 32, either sign
static const uint32_t kSmallPatterns = 33u << 23;

// others_every: expf_nonan, quant8, recip, sqrt and n2_axis always take every pattern; the other forms take the
// patterns that are multiples of others_every (1: every pattern)
static bool check_sweep(uint32_t others_every) {
    Timer timer;
    Check c_expf("expf_nonan"), c_sig("sigmoid"), c_sig2("sigmoid2"), c_q("quant8"), c_recip("recip"), c_sqrt("sqrt"),
        c_floor("floor"), c_inv("invdir"), c_n2("n2_axis"), c_ld("ldexp_div"), c_div("div");
    struct Word {
        int w;
        Check* c;
        bool every;   // every pattern, whatever others_every
        bool nan_in;  // NaN inputs belong to the domain
        const char* what;
    };
    const Word words[] = {
        {W_EXPF_NONAN, &c_expf, true, false, "of -x"}, {W_QUANT8, &c_q, true, true, ""},
        {W_RECIP, &c_recip, true, true, ""},           {W_SQRT, &c_sqrt, true, true, ""},
        {W_SIGMOID, &c_sig, false, true, ""},          {W_FLOOR, &c_floor, false, true, ""},
        {W_INVDIR, &c_inv, false, true, ""},           {W_LDEXP, &c_ld, false, true, "k drawn"},
        {W_DIV0, &c_div, false, true, "a=-2"},         {W_DIV1, &c_div, false, true, "a=1e9"},
        {W_DIV2, &c_div, false, true, "a=1-ulp"},      {W_DIV3, &c_div, false, true, "a=subnormal"},
    };
    std::mutex mu;
    std::vector<uint32_t> bad_n2;  // first x of n2_axis mismatches, for the per-depth report

    uint32_t *d[2], *h[2];
    hipEvent_t ev[2];
    const size_t bytes = sizeof(uint32_t) * W_COUNT * (size_t)kChunk;
    for (int b = 0; b < 2; ++b) {
        HIP_OK(hipMalloc(&d[b], bytes));
        HIP_OK(hipHostMalloc(&h[b], bytes));
        HIP_OK(hipEventCreate(&ev[b]));
    }
    auto compare = [&](uint32_t base, const uint32_t* got) {
        parallel_pieces(kChunk, kPiece, [&](uint64_t a, uint64_t e) {
            const uint32_t n = (uint32_t)(e - a);
            uint32_t want[W_COUNT * kRow];
            ref_sweep(base + (uint32_t)a, n, kRow, others_every, want);
            auto G = [&](int w, uint32_t i) { return got[(size_t)w * kChunk + a + i]; };
            auto R = [&](int w, uint32_t i) { return want[(size_t)w * kRow + i]; };
            uint32_t non_nan = 0, others = 0;
            bool other[kPiece];  // the pattern is a multiple of others_every
            for (uint32_t i = 0, r = (base + (uint32_t)a) % others_every; i < n; ++i, r = r + 1 == others_every ? 0 : r + 1) {
                non_nan += !is_nan_bits(base + (uint32_t)a + i);
                others += other[i] = r == 0;
            }
            for (const Word& wd : words) {
                for (uint32_t i = 0; i < n; ++i) {
                    const uint32_t u = base + (uint32_t)a + i;
                    if (!wd.nan_in && is_nan_bits(u)) continue;
                    if (!wd.every && !other[i]) continue;
                    if (!same_bits(G(wd.w, i), R(wd.w, i)))
                        wd.c->fail("x=0x%08x %s got=0x%08x want=0x%08x", u, wd.what, G(wd.w, i), R(wd.w, i));
                }
                wd.c->total += !wd.every ? others : wd.nan_in ? n : non_nan;
            }
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t u = base + (uint32_t)a + i;
                if (other[i] && !same_bits(G(W_SIGMOID2_X, i), R(W_SIGMOID2_X, i)))
                    c_sig2.fail(".x x=0x%08x (.y 0x%08x) got=0x%08x want=0x%08x", u, forms_partner(u),
                                G(W_SIGMOID2_X, i), R(W_SIGMOID2_X, i));
                if (other[i] && !same_bits(G(W_SIGMOID2_Y, i), R(W_SIGMOID2_Y, i)))
                    c_sig2.fail(".y x=0x%08x (.x 0x%08x) got=0x%08x want=0x%08x", forms_partner(u), u,
                                G(W_SIGMOID2_Y, i), R(W_SIGMOID2_Y, i));
                // n2_axis: two integer words, exact.  NaN stays out: vr_dev_query.h:67-70 documents that the
                // median clamp sends a NaN coordinate to 0 where the reference's min / max send it to `hi`.
                if (is_nan_bits(u)) continue;
                if (G(W_N2_U, i) != R(W_N2_U, i) || G(W_N2_FOLD, i) != R(W_N2_FOLD, i)) {
                    std::lock_guard<std::mutex> g(mu);
                    if (bad_n2.size() < 8) bad_n2.push_back(u);
                    else c_n2.bad++;
                }
            }
            c_sig2.total += others;
            c_n2.total += non_nan;
        });
    };
    const uint32_t n_chunks = (uint32_t)((1ull << 32) / kChunk);
    for (uint32_t c = 0; c <= n_chunks; ++c) {
        if (c < n_chunks) {
            k_sweep<<<blocks(kChunk), 256>>>(c * kChunk, kChunk, d[c & 1]);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(h[c & 1], d[c & 1], bytes, hipMemcpyDeviceToHost, 0));
            HIP_OK(hipEventRecord(ev[c & 1], 0));
        }
        if (c > 0) {  // the previous chunk, while the device works on this one
            HIP_OK(hipEventSynchronize(ev[(c - 1) & 1]));
            compare((c - 1) * kChunk, h[(c - 1) & 1]);
        }
    }
    timer.report("sweep_every_pattern");

    // ldexp_div, the quotients that can be subnormal: every k for every x with a small exponent
    std::vector<uint32_t> bad_ld;
    for (uint32_t sign = 0; sign < 2; ++sign)
        for (uint32_t base = 0; base < kSmallPatterns; base += kChunk) {
            k_ldexp_fold<<<blocks(kChunk), 256>>>(base, kChunk, sign << 31, d[0]);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpy(h[0], d[0], sizeof(uint32_t) * kChunk, hipMemcpyDeviceToHost));
            parallel_for(kChunk, [&](uint64_t i) {
                const uint32_t u = (base + (uint32_t)i) | (sign << 31);
                if (h[0][i] != ref_ldexp_fold(fl(u))) {
                    std::lock_guard<std::mutex> g(mu);
                    if (bad_ld.size() < 8) bad_ld.push_back(u);
                    else c_ld.bad++;
                }
            });
            c_ld.total += 32ull * kChunk;
        }
    timer.report("sweep_with_ldexp_folds");

    // a fold that differs: which term
    for (uint32_t u : bad_n2) {
        const std::vector<float> got = fold_terms(fl(u));
        float want[24];
        uint32_t want_u;
        ref_n2_axis(fl(u), &want_u, want);
        int d = 0;
        while (d < 24 && bits(got[d]) == bits(want[d])) ++d;
        if (d < 24)
            c_n2.fail("x=0x%08x first differing depth %d: local got=0x%08x want=0x%08x (digits want=0x%06x)", u, d + 1,
                      bits(got[d]), bits(want[d]), want_u);
        else
            c_n2.fail("x=0x%08x local coordinates agree, the digits differ (want=0x%06x)", u, want_u);
    }
    for (uint32_t u : bad_ld) {
        const std::vector<float> got = fold_terms(fl(u));
        int k = 0;
        while (k < 32 && bits(got[24 + k]) == bits(ref_ldexp_div(fl(u), k))) ++k;
        c_ld.fail("x=0x%08x first differing k %d: got=0x%08x want=0x%08x", u, k, k < 32 ? bits(got[24 + k]) : 0u,
                  k < 32 ? bits(ref_ldexp_div(fl(u), k)) : 0u);
    }
    for (int b = 0; b < 2; ++b) {
        HIP_OK(hipFree(d[b]));
        HIP_OK(hipHostFree(h[b]));
        HIP_OK(hipEventDestroy(ev[b]));
    }

    bool ok = true;
    for (Check* c : {&c_expf, &c_sig, &c_sig2, &c_q, &c_recip, &c_sqrt, &c_floor, &c_inv, &c_n2, &c_ld})
        ok &= c->report();
    ok &= check_div_pairs(c_div);  // adds the table pairs and reports
    return ok;
}

// ---- tables --------------------------------------------------------------------------------------------

static const float kSpecial[] = {0.f, -0.f, INFINITY, -INFINITY, NAN, 1.40129846e-45f, -1.40129846e-45f,
                                 1.17549421e-38f /* largest subnormal */, 5.87747175e-39f, 1.f, -1.f, 3.0e38f,
                                 -3.0e38f, 1e34f, 6e33f, 1e-40f, 1e-30f, 1e-38f, 1.17549435e-38f, 65504.f,
                                 1.f / 65504.f, 0.5f};
static const int kSpecials = sizeof kSpecial / sizeof kSpecial[0];

static float any_bits(std::mt19937& rng) { return fl((uint32_t)rng()); }  // any exponent, NaNs included
static float moderate(std::mt19937& rng) {
    return std::ldexp(std::uniform_real_distribution<float>(-2.f, 2.f)(rng), (int)(rng() % 60) - 30);
}

// (b, c) operands as tests/cpp/device_math_check.hip draws them: every pair of special values (signed zeros,
// infinities, NaN, subnormals, magnitudes near both ends of the range) and 300 random pairs (any bit pattern;
// moderate magnitudes; a moderate b with a special c)
static void operand_table(std::vector<float>& b, std::vector<float>& c) {
    for (int i = 0; i < kSpecials; ++i)
        for (int k = 0; k < kSpecials; ++k) b.push_back(kSpecial[i]), c.push_back(kSpecial[k]);
    std::mt19937 rng(12345);
    for (int i = 0; i < 100; ++i) {
        b.push_back(any_bits(rng)), c.push_back(any_bits(rng));
        b.push_back(moderate(rng)), c.push_back(moderate(rng));
        b.push_back(moderate(rng)), c.push_back(kSpecial[i % kSpecials]);
    }
}
// every value of the table: what a two-operand form takes every pair of
static std::vector<float> table_values() {
    std::vector<float> b, c;
    operand_table(b, c);
    b.insert(b.end(), c.begin(), c.end());
    return b;
}
// three operands: every triple of these -- the special values, 53 moderate and 53 any-bits values
static std::vector<float> table3_values() {
    std::vector<float> v(kSpecial, kSpecial + kSpecials);
    std::mt19937 rng(2468);
    for (int i = 0; i < 53; ++i) v.push_back(moderate(rng)), v.push_back(any_bits(rng));
    return v;
}

static bool check_div_pairs(Check& c_div) {
    const std::vector<float> v = table_values();
    const uint32_t nv = (uint32_t)v.size();
    float *dv = device_copy(v), *dout;
    HIP_OK(hipMalloc(&dout, sizeof(float) * nv * nv));
    k_div_pairs<<<blocks((uint64_t)nv * nv), 256>>>(dv, nv, dout);
    HIP_OK(hipGetLastError());
    const std::vector<float> got = host_copy(dout, (size_t)nv * nv);
    parallel_for((uint64_t)nv * nv, [&](uint64_t i) {
        const float a = v[i / nv], b = v[i % nv], want = ref_div(a, b);
        if (!same(got[i], want))
            c_div.fail("a=0x%08x b=0x%08x got=0x%08x want=0x%08x", bits(a), bits(b), bits(got[i]), bits(want));
    });
    c_div.total += (uint64_t)nv * nv;
    HIP_OK(hipFree(dv));
    HIP_OK(hipFree(dout));
    printf("operands div %u table values\n", nv);
    return c_div.report();
}

static bool check_byte_and_box() {
    Check c_byte("byte_over_255"), c_box("box_t");
    float* d;
    HIP_OK(hipMalloc(&d, sizeof(float) * 256));
    k_byte<<<1, 256>>>(d);
    HIP_OK(hipGetLastError());
    const std::vector<float> gb = host_copy(d, 256);
    HIP_OK(hipFree(d));
    for (int b = 0; b < 256; ++b)
        if (!same(gb[b], ref_byte_over_255(b)))
            c_byte.fail("b=%d got=0x%08x want=0x%08x", b, bits(gb[b]), bits(ref_byte_over_255(b)));
    c_byte.total += 256;

    const std::vector<float> v = table3_values();
    const uint32_t nv = (uint32_t)v.size();
    const uint64_t n = (uint64_t)nv * nv * nv;
    float *dv = device_copy(v), *dout;
    HIP_OK(hipMalloc(&dout, sizeof(float) * 2 * n));
    k_box_t<<<blocks(n), 256>>>(dv, nv, dout);
    HIP_OK(hipGetLastError());
    const std::vector<float> got = host_copy(dout, 2 * n);
    parallel_for(n, [&](uint64_t i) {
        const float b = v[i / (nv * nv)], c = v[(i / nv) % nv], inv = v[i % nv];
        for (int s = 0; s < 2; ++s) {
            const float want = ref_box_t(b, c, inv, s == 0 ? 1 : -1);
            if (!same(got[2 * i + s], want))
                c_box.fail("%c1e-6 b=0x%08x c=0x%08x inv=0x%08x got=0x%08x want=0x%08x", s == 0 ? '+' : '-', bits(b),
                           bits(c), bits(inv), bits(got[2 * i + s]), bits(want));
        }
    });
    c_box.total += 2 * n;
    HIP_OK(hipFree(dv));
    HIP_OK(hipFree(dout));
    printf("operands box_t %u values cubed\n", nv);
    const bool a = c_byte.report();
    return c_box.report() && a;
}

static const uint32_t kVecSets = 1u << 22;

static bool check_vec() {
    Check c_dda("dda_unit"), c_norm("norm3"), c_nrm("normalize3"), c_mv("mv3"), c_dot("dot3"), c_cross("cross3");
    // a quarter of the sets any bit pattern; the rest moderate magnitudes, one value in eight a special one
    std::vector<float> in((size_t)kVecSets * kVecIn);
    std::mt19937 rng(97531);
    for (uint32_t i = 0; i < kVecSets; ++i)
        for (int j = 0; j < kVecIn; ++j) {
            float& x = in[(size_t)i * kVecIn + j];
            if (i % 4 == 0) x = any_bits(rng);
            else if (rng() % 8 == 0) x = kSpecial[rng() % kSpecials];
            else x = moderate(rng);
        }
    float *din = device_copy(in), *dout;
    HIP_OK(hipMalloc(&dout, sizeof(float) * kVecOut * (size_t)kVecSets));
    for (int fma = 0; fma < 2; ++fma) {
        if (fma) k_vec<1><<<blocks(kVecSets), 256>>>(din, kVecSets, dout);
        else k_vec<0><<<blocks(kVecSets), 256>>>(din, kVecSets, dout);
        HIP_OK(hipGetLastError());
        const std::vector<float> got = host_copy(dout, kVecOut * (size_t)kVecSets);
        parallel_for(kVecSets, [&](uint64_t i) {
            const float *m = &in[i * kVecIn], *v = m + 9, *w = m + 12, *o = &got[i * kVecOut];
            float want[kVecOut];
            want[0] = or_dda_unit(v, w, fma);
            want[1] = or_norm3(v, fma);
            want[2] = v[0], want[3] = v[1], want[4] = v[2];
            or_normalize3(want + 2, fma);
            or_mv3(m, v, fma, want + 5);
            want[8] = or_dot3(v, w, fma);
            or_cross3(v, w, fma, want + 9);
            Check* const cs[kVecOut] = {&c_dda, &c_norm, &c_nrm, &c_nrm, &c_nrm, &c_mv,
                                        &c_mv,  &c_mv,   &c_dot, &c_cross, &c_cross, &c_cross};
            bool bad[kVecOut] = {};
            for (int j = 0; j < kVecOut; ++j) bad[j] = !same(o[j], want[j]);
            for (int j = 0; j < kVecOut; ++j)
                if (bad[j])
                    cs[j]->fail("fma=%d set %llu output %d got=0x%08x want=0x%08x v=(0x%08x 0x%08x 0x%08x) "
                                "w=(0x%08x 0x%08x 0x%08x)", fma, (unsigned long long)i, j, bits(o[j]), bits(want[j]),
                                bits(v[0]), bits(v[1]), bits(v[2]), bits(w[0]), bits(w[1]), bits(w[2]));
        });
        for (Check* c : {&c_dda, &c_norm, &c_nrm, &c_mv, &c_dot, &c_cross}) c->total += kVecSets;
    }
    HIP_OK(hipFree(din));
    HIP_OK(hipFree(dout));
    bool ok = true;
    for (Check* c : {&c_dda, &c_norm, &c_nrm, &c_mv, &c_dot, &c_cross}) ok &= c->report();
    return ok;
}

// 2^20 lattice points normalised in binary32, the 26 axis and diagonal directions, the same with one component
// replaced by +-0 or a +-subnormal, and 2^12 vectors that are not unit or not finite
static std::vector<float> basis_directions() {
    std::vector<float> d;
    auto push = [&](float x, float y, float z) { d.push_back(x), d.push_back(y), d.push_back(z); };
    auto push_unit = [&](float x, float y, float z) {
        const float inv = 1.f / std::sqrt(x * x + y * y + z * z);
        push(x * inv, y * inv, z * inv);
    };
    const uint32_t n = 1u << 20;
    const double golden = 2.399963229728653;  // pi (3 - sqrt 5)
    for (uint32_t i = 0; i < n; ++i) {
        const double z = 1.0 - (2.0 * i + 1.0) / n, r = std::sqrt(1.0 - z * z), phi = golden * i;
        push_unit((float)(r * std::cos(phi)), (float)(r * std::sin(phi)), (float)z);
    }
    const float swap[] = {0.f, -0.f, 1e-40f, -1e-40f};
    for (int x = -1; x <= 1; ++x)
        for (int y = -1; y <= 1; ++y)
            for (int z = -1; z <= 1; ++z) {
                if (!x && !y && !z) continue;
                push_unit((float)x, (float)y, (float)z);
                for (int c = 0; c < 3; ++c)
                    for (float s : swap) {
                        push_unit((float)x, (float)y, (float)z);
                        d[d.size() - 3 + c] = s;
                    }
            }
    std::mt19937 rng(1357);
    for (int i = 0; i < 4096; ++i) {
        float v[3];
        for (float& x : v) x = i % 2 ? any_bits(rng) : (rng() % 4 == 0 ? kSpecial[rng() % kSpecials] : moderate(rng));
        push(v[0], v[1], v[2]);
    }
    return d;
}

struct BasisForm {
    const char* name;
    int format, basis_dim;
    void (*launch)(const vr::KParams&, const float*, uint32_t, float*);
};
template <int FMA, bool LOBES, int BD>
static void launch_basis(const vr::KParams& p, const float* dirs, uint32_t n, float* out) {
    k_basis<FMA, LOBES, BD><<<blocks(n), 256>>>(p, dirs, n, out);
}

static bool check_basis() {
    Check c("basis");
    const std::vector<float> dirs = basis_directions();
    const uint32_t n = (uint32_t)(dirs.size() / 3);
    // lobes: SG 7 x (lambda, mu), ASG 4 x (lambda_x, lambda_y, mu_x, mu_y, mu_z); seeded, moderate
    std::vector<float> extra(VR_MAX_BASIS * 11);
    std::mt19937 rng(8642);
    for (float& x : extra) x = std::uniform_real_distribution<float>(-3.f, 3.f)(rng);
    float *ddirs = device_copy(dirs), *dextra = device_copy(extra), *dout;
    HIP_OK(hipMalloc(&dout, sizeof(float) * VR_MAX_BASIS * (size_t)n));
#define SH_FORMS(FMA)                                                                                     \
    {"SH1 runtime fma=" #FMA, VR_FORMAT_SH, 1, launch_basis<FMA, true, 0>},                               \
        {"SH4 runtime fma=" #FMA, VR_FORMAT_SH, 4, launch_basis<FMA, true, 0>},                           \
        {"SH9 runtime fma=" #FMA, VR_FORMAT_SH, 9, launch_basis<FMA, true, 0>},                           \
        {"SH16 runtime fma=" #FMA, VR_FORMAT_SH, 16, launch_basis<FMA, true, 0>},                         \
        {"SH25 runtime fma=" #FMA, VR_FORMAT_SH, 25, launch_basis<FMA, true, 0>},                         \
        {"SH1 compile-time fma=" #FMA, VR_FORMAT_SH, 1, launch_basis<FMA, false, 1>},                     \
        {"SH4 compile-time fma=" #FMA, VR_FORMAT_SH, 4, launch_basis<FMA, false, 4>},                     \
        {"SH9 compile-time fma=" #FMA, VR_FORMAT_SH, 9, launch_basis<FMA, false, 9>},                     \
        {"SH16 compile-time fma=" #FMA, VR_FORMAT_SH, 16, launch_basis<FMA, false, 16>},                  \
        {"SH25 compile-time fma=" #FMA, VR_FORMAT_SH, 25, launch_basis<FMA, false, 25>},                  \
        {"SG7 fma=" #FMA, VR_FORMAT_SG, 7, launch_basis<FMA, true, 0>},                                   \
        {"ASG4 fma=" #FMA, VR_FORMAT_ASG, 4, launch_basis<FMA, true, 0>}
    const BasisForm forms[] = {SH_FORMS(0), SH_FORMS(1)};
#undef SH_FORMS
    const int per_model = (int)(sizeof forms / sizeof forms[0]) / 2;
    for (int f = 0; f < 2 * per_model; ++f) {
        const BasisForm& form = forms[f];
        const int fma = f / per_model;
        vr::KParams p;
        memset(&p, 0, sizeof p);
        p.basis_dim = form.basis_dim;
        p.format = form.format;
        p.extra = dextra;
        OrTree t;
        memset(&t, 0, sizeof t);
        t.basis_dim = form.basis_dim;
        t.format = form.format;  // (OR_FORMAT_* == VR_FORMAT_*)
        t.extra = extra.data();
        form.launch(p, ddirs, n, dout);
        HIP_OK(hipGetLastError());
        const std::vector<float> got = host_copy(dout, VR_MAX_BASIS * (size_t)n);
        parallel_for(n, [&](uint64_t i) {
            float want[25];
            or_basis(&t, &dirs[3 * i], fma, want);
            for (int j = 0; j < 25; ++j)
                if (!same(got[i * VR_MAX_BASIS + j], want[j])) {
                    c.fail("%s dir=(0x%08x 0x%08x 0x%08x) basis %d got=0x%08x want=0x%08x", form.name, bits(dirs[3 * i]),
                           bits(dirs[3 * i + 1]), bits(dirs[3 * i + 2]), j, bits(got[i * VR_MAX_BASIS + j]),
                           bits(want[j]));
                    break;
                }
        });
        c.total += n;
    }
    HIP_OK(hipFree(ddirs));
    HIP_OK(hipFree(dextra));
    HIP_OK(hipFree(dout));
    printf("operands basis %u directions x %d forms\n", n, 2 * per_model);
    return c.report();
}

int main(int argc, char** argv) {
    static_assert((int)OR_FORMAT_SH == (int)VR_FORMAT_SH && (int)OR_FORMAT_SG == (int)VR_FORMAT_SG &&
                      (int)OR_FORMAT_ASG == (int)VR_FORMAT_ASG, "the oracle's format numbers are the product's");
    const std::string what = argc > 1 ? argv[1] : "all";
    require_subnormals();
    bool ok = true;
    if (what == "all" || what == "table") {
        Timer t;
        ok &= check_byte_and_box();
        ok &= check_vec();
        ok &= check_basis();
        t.report("table");
    }
    if (what == "all" || what == "sweep") {
        const long every = argc > 2 ? atol(argv[2]) : 1;
        if (every < 1 || every % 2 == 0) {
            fprintf(stderr, "usage: device_forms_check [all|table|sweep] [others_every: odd, default 1]\n");
            return 2;
        }
        ok &= check_sweep((uint32_t)every);
    }
    return ok ? 0 : 1;
}
