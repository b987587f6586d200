/* forms_reference.c -- the host side of tests/cpp/device_forms_check.hip: the plain C operators (/, sqrtf,
 * floorf, casts, FP64 products) as this file's compiler rounds them under the oracle's flags (tests/build_util.py
 * c_library: -ffp-contract=off), and the oracle's own functions (liboracle.so) where it has one.  The words and
 * the operand draws are those of device_forms.h. */
#include <math.h>
#include <stdint.h>

#include "device_forms.h"
#include "vr_detmath.h" /* vr_minf / vr_maxf, vr_bits2f / vr_f2bits */
#include "vr_oracle.h"

static float pow2(int k) { return vr_bits2f((uint32_t)(127 + k) << 23); } /* 2^k, -126 <= k <= 127 */

/* 1 unless a binary32 subnormal is flushed to zero on the way in or out of a multiply */
int ref_keeps_subnormals(void) {
    volatile float tiny = 1e-40f, one = 1.f;
    return tiny * one != 0.f;
}

/* One axis of n3tree_query.hpp:17-33 for N = 2: the clamp, then 24 rounds of the literal float descent.
 * Round d: the digit goes to bit 24 - d of *digits, the coordinate after it into the fold. */
static inline float n2_clamp(float x) {
    const float hi = 1.f - 1e-6f;
    return vr_maxf(vr_minf(x, hi), 0.f);
}
static inline float n2_round(float c, int d, uint32_t* digits, uint32_t* fold) {
    c *= 2.f;
    const float k = floorf(c);
    c -= k;
    *digits |= (uint32_t)k << (24 - d);
    *fold += forms_rotl(vr_f2bits(c), d);
    return c;
}

/* -> the fold; *u: the digits; local[d - 1] (may be NULL): the coordinate after round d */
uint32_t ref_n2_axis(float x, uint32_t* u, float* local) {
    float c = n2_clamp(x);
    uint32_t digits = 0, fold = 0;
    for (int d = 1; d <= 24; ++d) {
        c = n2_round(c, d, &digits, &fold);
        if (local) local[d - 1] = c;
    }
    *u = digits;
    return fold;
}

/* ref_n2_axis for the n patterns from base on, a block of coordinates at a time: round d of the whole block
 * before round d + 1, so that the 24 dependent rounds of one coordinate overlap with its neighbours' -- the
 * operations on each coordinate are the same.  Neighbouring patterns that clamp to the same coordinate (every
 * x <= 0, every x >= hi) share one evaluation: the recurrence is a function of the clamped coordinate alone. */
static void n2_axis_n(uint32_t base, uint32_t n, uint32_t* u, uint32_t* fold) {
    enum { BLOCK = 64 };
    for (uint32_t i0 = 0; i0 < n; i0 += BLOCK) {
        const uint32_t m = n - i0 < BLOCK ? n - i0 : BLOCK;
        float c[BLOCK];
        uint32_t dg[BLOCK], fo[BLOCK], distinct = 0;
        uint8_t which[BLOCK];
        for (uint32_t j = 0; j < m; ++j) {
            const float cj = n2_clamp(vr_bits2f(base + i0 + j));
            if (distinct == 0 || vr_f2bits(cj) != vr_f2bits(c[distinct - 1])) {
                c[distinct] = cj, dg[distinct] = 0, fo[distinct] = 0;
                ++distinct;
            }
            which[j] = (uint8_t)(distinct - 1);
        }
        for (int d = 1; d <= 24; ++d)
            for (uint32_t j = 0; j < distinct; ++j) c[j] = n2_round(c[j], d, &dg[j], &fo[j]);
        for (uint32_t j = 0; j < m; ++j) u[i0 + j] = dg[which[j]], fold[i0 + j] = fo[which[j]];
    }
}

float ref_ldexp_div(float x, int k) { return x / pow2(k); }

/* sum over k = 0..31 of rotl(bits(x / 2^k), k) */
uint32_t ref_ldexp_fold(float x) {
    uint32_t fold = 0;
    for (int k = 0; k < 32; ++k) fold += forms_rotl(vr_f2bits(x / pow2(k)), k);
    return fold;
}

float ref_div(float a, float b) { return a / b; }
float ref_byte_over_255(int b) { return (float)b / 255.f; }

/* rt_core.cuh:23-24, one slab: sign > 0 the lower bound (+ 1e-6), else the upper (- 1e-6) */
float ref_box_t(float b, float c, float inv, int sign) {
    if (sign > 0) return (float)((((double)b + 1e-6) - (double)c) * (double)inv);
    return (float)((((double)b - 1e-6) - (double)c) * (double)inv);
}

/* out[w * stride + i] = word w of pattern base + i (device_forms.h), i < n <= stride.  (A stride that is no
 * multiple of 4 KB keeps the 16 rows out of each other's cache sets.)  W_EXPF_NONAN, W_QUANT8, W_RECIP, W_SQRT and
 * W_N2_* are formed for every pattern, the other words for the patterns that are multiples of others_every. */
void ref_sweep(uint32_t base, uint32_t n, uint32_t stride, uint32_t others_every, uint32_t* out) {
    for (uint32_t i = 0, r = base % others_every; i < n; ++i, r = r + 1 == others_every ? 0 : r + 1) {
        const uint32_t u = base + i; /* r = u % others_every */
        const float x = vr_bits2f(u), y = vr_bits2f(forms_partner(u));
        const float e = or_expf(-x);
#define OUT_F(w, v) out[(size_t)(w) * stride + i] = vr_f2bits(v)
        OUT_F(W_EXPF_NONAN, e);
        out[(size_t)W_QUANT8 * stride + i] = or_quant8(x, OR_FP_STRICT);
        OUT_F(W_RECIP, 1.f / x);
        OUT_F(W_SQRT, sqrtf(x));
        if (r) continue;
        OUT_F(W_SIGMOID, 1.f / (1.f + e));
        OUT_F(W_SIGMOID2_X, 1.f / (1.f + e));
        OUT_F(W_SIGMOID2_Y, 1.f / (1.f + or_expf(-y)));
        OUT_F(W_FLOOR, floorf(x));
        OUT_F(W_INVDIR, (float)(1.0 / ((double)x + 1e-9)));
        OUT_F(W_LDEXP, x / pow2(forms_k(u)));
        for (int j = 0; j < 4; ++j) OUT_F(W_DIV0 + j, vr_bits2f(forms_div_a_bits(j)) / x);
#undef OUT_F
    }
    n2_axis_n(base, n, out + (size_t)W_N2_U * stride, out + (size_t)W_N2_FOLD * stride);
}
