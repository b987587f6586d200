/* device_forms.h -- what tests/cpp/device_forms_check.hip (device side, C++) and tests/cpp/forms_reference.c
 * (host reference, C with the oracle's flags) must agree on: the words of the one-argument sweep and how the
 * second operand of a form is drawn from the bit pattern of the first. */
#ifndef DEVICE_FORMS_H_
#define DEVICE_FORMS_H_
#include <stdint.h>

#ifdef __HIPCC__
#define FORMS_HD __host__ __device__ static inline
#else
#define FORMS_HD static inline
#endif

/* One 32-bit word per form and bit pattern u (x = the float with the bits u).
 * W_EXPF_NONAN is taken at -x: -x runs over every pattern as x does, and the or_expf(-x) of the sigmoid
 * then serves both. */
enum {
    W_EXPF_NONAN, /* vr_expf_nonan(-x)                                   | or_expf(-x) */
    W_SIGMOID,    /* sigmoid(x)                                          | 1 / (1 + or_expf(-x)) */
    W_SIGMOID2_X, /* weighted_sigmoid2(1, x, partner(x)): .x, .y         | the same, per component */
    W_SIGMOID2_Y,
    W_QUANT8,     /* quant8(x)                                           | or_quant8(x) */
    W_RECIP,      /* 1.f / x */
    W_SQRT,       /* __builtin_sqrtf(x)                                  | sqrtf(x) */
    W_FLOOR,      /* __builtin_floorf(x)                                 | floorf(x) */
    W_INVDIR,     /* (float)(1.0 / ((double)x + 1e-9)) */
    W_N2_U,       /* query_n2's digits of one axis: (uint32_t)(c * 2^24) | the digits of the float recurrence */
    W_N2_FOLD,    /* sum over d = 1..24 of rotl(bits(local coordinate at depth d), d) */
    W_LDEXP,      /* ldexp(x, -k), k = forms_k(u)                        | x / 2^k */
    W_DIV0,       /* forms_div_a(j) / x, j = 0..3 */
    W_DIV1,
    W_DIV2,
    W_DIV3,
    W_COUNT
};

/* the second pattern of a packed pair: odd multiplier + xor-shift, a bijection of uint32 */
FORMS_HD uint32_t forms_partner(uint32_t u) {
    u *= 0x9E3779B1u;
    return u ^ (u >> 15);
}

/* the exponent 0..31 that goes with pattern u in the ldexp / division comparison */
FORMS_HD int forms_k(uint32_t u) { return (int)((u * 0x9E3779B1u) >> 27); }

/* bit patterns of the dividends of W_DIV*: -2, 1e9f, the largest float below 1, a subnormal */
FORMS_HD uint32_t forms_div_a_bits(int j) {
    return j == 0 ? 0xC0000000u : j == 1 ? 0x4E6E6B28u : j == 2 ? 0x3F7FFFFFu : 0x00012345u;
}

FORMS_HD uint32_t forms_rotl(uint32_t v, int d) { return (v << (d & 31)) | (v >> ((32 - d) & 31)); }

#endif
