// vr_dev_shade.h -- colour of a sample: the view-dependent basis, a leaf record in registers or in
// an LDS row, the per-channel dot products in the reference's association, RGBA8 quantisation.
// Device code only.  Built with -ffp-contract=off; see vr_device_math.h.
#pragma once
#include "vr_device_math.h"
#include "vr_dev_layout.h"

namespace vr {

namespace {

// ---------------------------------------------------------------------------
// view-dependent basis, lumisphere.hpp:9-87 (double literals => FP64 products)
// ---------------------------------------------------------------------------
// LOBES=false compiles the SH branch only (the hot configuration keeps zero
// scratch); LOBES=true adds the SG / ASG lobes read from tree.extra.
// BD > 0: the basis size is known at compile time (the render kernel's refill: SH only).
template <int FMA, bool LOBES, int BD = 0>
__device__ __forceinline__ void precalc_basis(const KParams& p, const float* dir, float* out) {
    using P = Policy<FMA>;
    const int basis_dim = BD > 0 ? BD : p.basis_dim;
    // NB: every index into out[] is a compile-time constant (loops fully
    // unrolled, predicated on basis_dim) so the array stays in VGPRs.
    if (LOBES && p.format == VR_FORMAT_ASG) {  // lumisphere.hpp:14-29
#pragma unroll
        for (int i = 0; i < VR_MAX_BASIS; ++i) {
            if (i < basis_dim) {
                const float* ptr = p.extra + i * 11;
                const float S = dot3<FMA>(dir, ptr + 8);
                const float dot_x = dot3<FMA>(dir, ptr + 2);
                const float dot_y = dot3<FMA>(dir, ptr + 5);
                const float arg = P::msub(-ptr[0] * dot_x, dot_x, ptr[1] * dot_y * dot_y);
                out[i] = S * vr_expf(arg) / (float)basis_dim;
            }
        }
    } else if (LOBES && p.format == VR_FORMAT_SG) {  // lumisphere.hpp:30-37
#pragma unroll
        for (int i = 0; i < VR_MAX_BASIS; ++i) {
            if (i < basis_dim) {
                const float* ptr = p.extra + i * 4;
                out[i] = vr_expf(ptr[0] * (dot3<FMA>(dir, ptr + 1) - 1.f)) / (float)basis_dim;
            }
        }
    } else if (BD > 0 || p.format == VR_FORMAT_SH) {  // lumisphere.hpp:38-81
        out[0] = (float)0.28209479177387814;
        const float x = dir[0], y = dir[1], z = dir[2];
        const float xx = x * x, yy = y * y, zz = z * z;
        const float xy = x * y, yz = y * z, xz = x * z;
        if (basis_dim == 25) {
            out[16] = (float)(2.5033429417967046 * (double)xy * (double)(xx - yy));
            out[17] = (float)(-1.7701307697799304 * (double)yz * (double)P::msub(3.f, xx, yy));
            out[18] = (float)(0.9461746957575601 * (double)xy * (double)P::msub(7.f, zz, 1.f));
            out[19] = (float)(-0.6690465435572892 * (double)yz * (double)P::msub(7.f, zz, 3.f));
            out[20] = (float)(0.10578554691520431 *
                              (double)P::madd(zz, P::msub(35.f, zz, 30.f), 3.f));
            out[21] = (float)(-0.6690465435572892 * (double)xz * (double)P::msub(7.f, zz, 3.f));
            out[22] =
                (float)(0.47308734787878004 * (double)(xx - yy) * (double)P::msub(7.f, zz, 1.f));
            out[23] = (float)(-1.7701307697799304 * (double)xz * (double)P::nmadd(3.f, yy, xx));
            const float a = P::nmadd(3.f, yy, xx);
            const float b = P::msub(3.f, xx, yy);
            out[24] = (float)(0.6258357354491761 * (double)P::msub(xx, a, yy * b));
        }
        if (basis_dim == 25 || basis_dim == 16) {
            out[9] = (float)(-0.5900435899266435 * (double)y * (double)P::msub(3.f, xx, yy));
            out[10] = (float)(2.890611442640554 * (double)xy * (double)z);
            out[11] = (float)(-0.4570457994644658 * (double)y * (double)(P::msub(4.f, zz, xx) - yy));
            out[12] = (float)(0.3731763325901154 * (double)z *
                              (double)P::nmadd(3.f, yy, P::msub(2.f, zz, 3.f * xx)));
            out[13] = (float)(-0.4570457994644658 * (double)x * (double)(P::msub(4.f, zz, xx) - yy));
            out[14] = (float)(1.445305721320277 * (double)z * (double)(xx - yy));
            out[15] = (float)(-0.5900435899266435 * (double)x * (double)P::nmadd(3.f, yy, xx));
        }
        if (basis_dim == 25 || basis_dim == 16 || basis_dim == 9) {
            out[4] = (float)(1.0925484305920792 * (double)xy);
            out[5] = (float)(-1.0925484305920792 * (double)yz);
            out[6] = (float)(0.31539156525252005 *
                             (P::dmsub(2.0, (double)zz, (double)xx) - (double)yy));
            out[7] = (float)(-1.0925484305920792 * (double)xz);
            out[8] = (float)(0.5462742152960396 * (double)(xx - yy));
        }
        if (basis_dim == 25 || basis_dim == 16 || basis_dim == 9 || basis_dim == 4) {
            out[1] = (float)(-0.4886025119029199 * (double)y);
            out[2] = (float)(0.4886025119029199 * (double)z);
            out[3] = (float)(-0.4886025119029199 * (double)x);
        }
    }
}

// ---------------------------------------------------------------------------
// One leaf record in registers.  NV = 16-byte vectors per record for the
// compile-time basis sizes; BASIS_1 / RGBA use narrower loads.
// ---------------------------------------------------------------------------
template <int BASIS>
struct RecTraits {
    static constexpr int kHalfs = BASIS > 1 ? 3 * BASIS : 3;
    static constexpr int kDwords = BASIS > 1 ? ((kHalfs * 2 + 15) / 16) * 4 : 2;
};

template <int BASIS>
struct Record {
    uint32_t w[RecTraits<BASIS>::kDwords];
    template <int E>  // the packed word that holds coefficient E
    __device__ __forceinline__ uint32_t word() const {
        return w[E >> 1];
    }
    // coefficient i (compile-time) as fp32
    __device__ __forceinline__ float at(int i) const {
        const uint32_t d = w[i >> 1];
        return h2f((uint16_t)((i & 1) ? (d >> 16) : (d & 0xFFFFu)));
    }
};

template <int BASIS>
__device__ __forceinline__ void load_record(const KParams& p, uint32_t leaf, Record<BASIS>& r) {
    const uint16_t* base = p.leaves + (uint64_t)leaf * (uint32_t)p.leaf_stride_h;
    if (BASIS == BASIS_RGBA) {
        const uint2 v = *reinterpret_cast<const uint2*>(base);  // stride >= 8 B
        r.w[0] = v.x;
        r.w[1] = v.y;
    } else if (BASIS == BASIS_1) {
        // runtime channel stride (basis_dim is not one of 4/9/16/25): only the
        // first coefficient of each channel is used, rt_core.cuh:131
        const uint32_t c0 = base[0], c1 = base[p.basis_dim], c2 = base[2 * p.basis_dim];
        r.w[0] = c0 | (c1 << 16);
        r.w[1] = c2;
    } else {
        const uint4* v = reinterpret_cast<const uint4*>(base);
#pragma unroll
        for (int j = 0; j < RecTraits<BASIS>::kDwords / 4; ++j) {
            const uint4 q = v[j];
            r.w[4 * j + 0] = q.x;
            r.w[4 * j + 1] = q.y;
            r.w[4 * j + 2] = q.z;
            r.w[4 * j + 3] = q.w;
        }
    }
}

// SH / SG colour of channel c: rt_core.cuh:125-165.  Group order 25 -> 16 -> 9
// -> 4, each group summed left to right, then added to tmp.  Coefficient e of the record is
// half (e & 1) of word e >> 1; products read it in place (mul_half / fma_half).
template <int E, typename SRC>
__device__ __forceinline__ float coef_mul(float b, const SRC& r) {
    return mul_half<E & 1>(b, r.template word<E>());
}
template <int FMA, int E, typename SRC>  // Policy<FMA>::madd(b, coefficient E, c)
__device__ __forceinline__ float coef_madd(float b, const SRC& r, float c) {
    if (FMA) return fma_half<E & 1>(b, r.template word<E>(), c);
    return mul_add_half<E & 1>(b, r.template word<E>(), c);
}
// g = b[LO]*v[LO] (+) b[LO+1]*v[LO+1] (+) ... (+) b[HI]*v[HI], coefficients at offset O
template <int FMA, int O, int LO, int HI>
struct DotGroup {
    template <int I, typename SRC>
    static __device__ __forceinline__ float step(const float* b, const SRC& r, float g) {
        if constexpr (I > HI) {
            return g;
        } else {
            return step<I + 1>(b, r, coef_madd<FMA, O + I>(b[I], r, g));
        }
    }
    template <typename SRC>
    static __device__ __forceinline__ float run(const float* b, const SRC& r) {
        const float first = coef_madd<FMA, O + LO>(b[LO], r, coef_mul<O + LO + 1>(b[LO + 1], r));
        return step<LO + 2>(b, r, first);
    }
};

// SRC = Record<BASIS> (whole record in registers) or GroupWin (words of a staged record)
template <int FMA, int BASIS, int C, typename SRC>
__device__ __forceinline__ float channel_dot(const float* basis_fn, const SRC& r) {
    static_assert(BASIS > 1, "SH / SG / ASG sizes only");
    constexpr int O = C * BASIS;
    float tmp = coef_mul<O>(basis_fn[0], r);
    if constexpr (BASIS == 25) tmp += DotGroup<FMA, O, 16, 24>::run(basis_fn, r);
    if constexpr (BASIS >= 16) tmp += DotGroup<FMA, O, 9, 15>::run(basis_fn, r);
    if constexpr (BASIS >= 9) tmp += DotGroup<FMA, O, 4, 8>::run(basis_fn, r);
    if constexpr (BASIS >= 4) tmp += DotGroup<FMA, O, 1, 3>::run(basis_fn, r);
    return tmp;
}

// The words of a staged record (LDS row) that hold coefficients LO..HI of channel C.
template <int BASIS, int C, int LO, int HI>
struct GroupWin {
    static constexpr int kW0 = (C * BASIS + LO) / 2, kW1 = (C * BASIS + HI) / 2;
    uint32_t w[kW1 - kW0 + 1];
    __device__ __forceinline__ void load(const char* row) {
        const uint32_t* r32 = reinterpret_cast<const uint32_t*>(row);
#pragma unroll
        for (int j = 0; j <= kW1 - kW0; ++j) w[j] = r32[kW0 + j];
    }
    template <int E>
    __device__ __forceinline__ uint32_t word() const {
        return w[(E >> 1) - kW0];
    }
};

// rt_core.cuh:131-160 for the three channels of one staged record, group by group: the group
// sums are independent subexpressions of `tmp`, so each group's basis values are fetched
// (get(i) = basis_fn[i] of the ray that owns the item) right before the three channels use
// them and are dead afterwards -- the same operations in the same association as
// channel_dot, with ~12 fewer live registers than gathering the whole basis up front.
template <int FMA, int BASIS, int LO, int HI, bool FENCE, typename GET>
__device__ __forceinline__ void add_group(const char* row, GET&& get, float* acc) {
    float b[VR_MAX_BASIS];
    // FENCE keeps the scheduler from hoisting the next group's fetches over this group's
    // arithmetic (lowest register use, but every group then waits for its own LDS round trip: for
    // flavours on a tighter register budget than they like -- none of the production ones)
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = LO; i <= HI; ++i) b[i] = get(i);
    {
        GroupWin<BASIS, 0, LO, HI> w;
        w.load(row);
        acc[0] += DotGroup<FMA, 0 * BASIS, LO, HI>::run(b, w);
    }
    {
        GroupWin<BASIS, 1, LO, HI> w;
        w.load(row);
        acc[1] += DotGroup<FMA, 1 * BASIS, LO, HI>::run(b, w);
    }
    {
        GroupWin<BASIS, 2, LO, HI> w;
        w.load(row);
        acc[2] += DotGroup<FMA, 2 * BASIS, LO, HI>::run(b, w);
    }
}

// The same sums where get() is an LDS round trip (the one-pass flavours of the render kernel: a ds_bpermute out
// of the owner lane's registers): a group that fetches its basis values, waits and then computes spends most of its
// time waiting, and a shade round is one dependent path per wave.  Here a group's basis values are requested one
// group AHEAD of their use and its record words in front of the next group's permutes: LDS returns in order, so
// the wait of a group's arithmetic counts down to the next group's permutes and leaves them in flight.  begin()
// asks for b0 and the first group; it needs no record and may stand in front of the wait for the record DMA.
// The operations and their association are add_group's, group order c0, 9..15, 4..8, 1..3.
// (Not the record words one group ahead as well: 6-8 registers over the caps of SH16 and SH9 -- scratch.  Not SH9's
// last group ahead: 2 registers over its cap.)
template <int BASIS, int LO, int HI>
struct AheadGroup {
    float b[VR_MAX_BASIS];  // (LO..HI used)
    GroupWin<BASIS, 0, LO, HI> w0;
    GroupWin<BASIS, 1, LO, HI> w1;
    GroupWin<BASIS, 2, LO, HI> w2;
    template <typename GET>
    __device__ __forceinline__ void fetch_basis(GET&& get) {
#pragma unroll
        for (int i = LO; i <= HI; ++i) b[i] = get(i);
    }
    __device__ __forceinline__ void fetch_words(const char* row) {
        w0.load(row);
        w1.load(row);
        w2.load(row);
    }
    template <int FMA>
    __device__ __forceinline__ void add(float* acc) const {
        acc[0] += DotGroup<FMA, 0 * BASIS, LO, HI>::run(b, w0);
        acc[1] += DotGroup<FMA, 1 * BASIS, LO, HI>::run(b, w1);
        acc[2] += DotGroup<FMA, 2 * BASIS, LO, HI>::run(b, w2);
    }
};

template <int FMA, int BASIS>
struct SumsAhead {
    static_assert(BASIS == 4 || BASIS == 9 || BASIS == 16, "the one-pass record sizes");
    AheadGroup<BASIS, 0, 0> g0;
    AheadGroup<BASIS, 9, 15> ga;
    AheadGroup<BASIS, 4, 8> gb;
    AheadGroup<BASIS, 1, 3> gc;
    // Nothing crosses: the scheduler, minimising registers under the flavour's cap, would sink every permute to its
    // first use.
    static __device__ __forceinline__ void fence() { __builtin_amdgcn_sched_barrier(0); }

    template <typename GET>
    __device__ __forceinline__ void begin(GET&& get) {
        g0.fetch_basis(get);
        if constexpr (BASIS >= 16) ga.fetch_basis(get);
        else if constexpr (BASIS >= 9) gb.fetch_basis(get);
        else gc.fetch_basis(get);
        fence();
    }
    template <typename GET>
    __device__ __forceinline__ void finish(const char* row, GET&& get, float* acc) {
        g0.fetch_words(row);
        fence();
        acc[0] = coef_mul<0 * BASIS>(g0.b[0], g0.w0);
        acc[1] = coef_mul<1 * BASIS>(g0.b[0], g0.w1);
        acc[2] = coef_mul<2 * BASIS>(g0.b[0], g0.w2);
        if constexpr (BASIS >= 16) {
            ga.fetch_words(row);
            gb.fetch_basis(get);
            fence();
            ga.template add<FMA>(acc);
        }
        if constexpr (BASIS >= 9) {
            gb.fetch_words(row);
            if constexpr (BASIS >= 16) gc.fetch_basis(get);
            fence();
            gb.template add<FMA>(acc);
            if constexpr (BASIS < 16) gc.fetch_basis(get);
        }
        gc.fetch_words(row);
        fence();
        gc.template add<FMA>(acc);
    }
};

template <int FMA, int BASIS, bool FENCE = false, typename GET>
__device__ __forceinline__ void channel_sums(const char* row, GET&& get, float* acc) {
    static_assert(BASIS > 1, "SH / SG / ASG sizes only");
    {
        const float b0 = get(0);
        GroupWin<BASIS, 0, 0, 0> w0;
        GroupWin<BASIS, 1, 0, 0> w1;
        GroupWin<BASIS, 2, 0, 0> w2;
        w0.load(row);
        w1.load(row);
        w2.load(row);
        acc[0] = coef_mul<0 * BASIS>(b0, w0);
        acc[1] = coef_mul<1 * BASIS>(b0, w1);
        acc[2] = coef_mul<2 * BASIS>(b0, w2);
    }
    if constexpr (BASIS == 25) add_group<FMA, BASIS, 16, 24, FENCE>(row, get, acc);
    if constexpr (BASIS >= 16) add_group<FMA, BASIS, 9, 15, FENCE>(row, get, acc);
    if constexpr (BASIS >= 9) add_group<FMA, BASIS, 4, 8, FENCE>(row, get, acc);
    if constexpr (BASIS >= 4) add_group<FMA, BASIS, 1, 3, FENCE>(row, get, acc);
}

// rt_core.cuh:161 / volrend.cu:126: the colour of a channel sum, in the three spellings the kernels use.
// (tests/cpp/device_forms_check.hip runs them over every float.)
__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + vr_expf(-x)); }
__device__ __forceinline__ float weighted_sigmoid(float weight, float x) {
    return weight / (1.f + vr_expf(-x));
}
// two channels at once: their exponentials share packed mul / fma / add instructions
__device__ __forceinline__ float2v weighted_sigmoid2(float weight, float x0, float x1) {
    const float2v e01 = vr_expf2((float2v){-x0, -x1}) + splat2(1.f);
    return (float2v){weight / e01.x, weight / e01.y};
}

__device__ __forceinline__ uint32_t quant8(float v) {
    // float -> uint8 the way a host build of the reference converts
    // (truncate to int32, keep the low byte); volrend.cu:166
    const float s = v * 255.f;
    if (s != s) return 0u;
    if (s >= 2147483648.f || s < -2147483648.f) return 0u;
    return (uint32_t)(int32_t)s & 0xFFu;
}

}  // namespace

}  // namespace vr
