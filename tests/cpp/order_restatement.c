/*
 * order_restatement.c -- the yardstick of the vr_order_rays tests (TEST INFRASTRUCTURE).
 *
 * The key of one ray of a list, from the oracle's own functions (oracle/vr_oracle_core.inc, both FP models,
 * included as march_restatement.h includes it): the ray is set up as a pixel's ray is behind screen2worlddir's
 * matrix product -- direction normalised, maybe_world2ndc, offset + scale * cen, _get_delta_scale, the ray/box
 * test against render_bbox with t_max = 1e9 -- and then
 *   a ray that does not enter (tree N <= 0, or the ray/box test fails)       key = 0xFFFFFFFF
 *   otherwise e[c] = madd(tmin, dir[c], cen[c]), x[c] = madd(tmax, dir[c], cen[c]) (the march's position formula),
 *   each of (e0, e1, e2, x0, x1, x2) quantised to `bits` bits: q = (uint32_t)min(max(v * 2^bits, 0.f), 2^bits - 1),
 *   truncating, NaN -> 0; bit 6 * b + c of the key = bit b of coordinate c.
 *
 * Build: tests/build_util.py c_library(..., oracle=True).
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "vr_oracle.h"
#include "vr_detmath.h"

#define VR_FMA 0
#include "vr_oracle_core.inc"
#undef VR_FMA
#undef FN
#undef MADD
#undef MSUB
#undef NMADD
#undef DMADD
#undef DMSUB
#define VR_FMA 1
#include "vr_oracle_core.inc"
#undef VR_FMA

static inline float madd_strict(float a, float b, float c) { return a * b + c; }
static inline float madd_fma(float a, float b, float c) { return fmaf(a, b, c); }

static uint32_t quantise(float v, int bits) {
    const float scale = (float)(1 << bits);
    const float s = v * scale;
    if (!(s > 0.f)) return 0u; /* negative, -0, NaN */
    return (uint32_t)(s < scale - 1.f ? s : scale - 1.f);
}

static uint32_t morton6(const uint32_t* q, int bits) {
    uint32_t key = 0;
    for (int b = 0; b < bits; ++b)
        for (int c = 0; c < 6; ++c) key |= ((q[c] >> b) & 1u) << (6 * b + c);
    return key;
}

#define DEFINE_ORDER_KEY(M)                                                                              \
    static uint32_t order_key_##M(const OrTree* tree, const OrOptions* opt, const float* origin,          \
                                  const float* direction, int bits, float* seg) {                         \
        float dir[3] = {direction[0], direction[1], direction[2]};                                        \
        float cen[3] = {origin[0], origin[1], origin[2]};                                                 \
        for (int i = 0; i < 6; ++i) seg[i] = 0.f;                                                         \
        if (!(tree->N > 0)) return 0xFFFFFFFFu;                                                           \
        normalize3_##M(dir);                                                                              \
        maybe_world2ndc_##M(tree, dir, cen);                                                              \
        for (int i = 0; i < 3; ++i) cen[i] = madd_##M(tree->scale[i], cen[i], tree->offset[i]);           \
        float tmax_bg = 1e9f;                                                                             \
        dir[0] *= tree->scale[0];                                                                         \
        dir[1] *= tree->scale[1];                                                                         \
        dir[2] *= tree->scale[2];                                                                         \
        const float delta_scale = 1.f / norm3_##M(dir);                                                   \
        dir[0] *= delta_scale;                                                                            \
        dir[1] *= delta_scale;                                                                            \
        dir[2] *= delta_scale;                                                                            \
        tmax_bg /= delta_scale;                                                                           \
        float tmin, tmax, invdir[3];                                                                      \
        for (int i = 0; i < 3; ++i) invdir[i] = (float)(1.0 / ((double)dir[i] + 1e-9));                   \
        dda_world_##M(cen, invdir, &tmin, &tmax, opt->render_bbox);                                       \
        tmax = vr_minf(tmax, tmax_bg);                                                                    \
        if (tmax < 0 || tmin > tmax) return 0xFFFFFFFFu;                                                  \
        uint32_t q[6];                                                                                    \
        for (int c = 0; c < 3; ++c) {                                                                     \
            seg[c] = madd_##M(tmin, dir[c], cen[c]);                                                      \
            seg[3 + c] = madd_##M(tmax, dir[c], cen[c]);                                                  \
        }                                                                                                 \
        for (int c = 0; c < 6; ++c) q[c] = quantise(seg[c], bits);                                        \
        return morton6(q, bits);                                                                          \
    }

DEFINE_ORDER_KEY(strict)
DEFINE_ORDER_KEY(fma)

/* The coordinate rule alone, for the tests that pin it on values. */
uint32_t order_quantise(float v, int bits) { return quantise(v, bits); }

/* keys[i] of rays i = 0 .. n-1 (origins, dirs: [n][3]); segments: [n][6] = (e0, e1, e2, x0, x1, x2) of the rays
 * that enter (zeros otherwise), or NULL.  Returns 0, or 1 on a bad argument. */
int order_keys(const OrTree* tree, const OrOptions* opt, int fp_mode, int64_t n, const float* origins,
               const float* dirs, int bits, uint32_t* keys, float* segments) {
    if (!tree || !opt || !origins || !dirs || !keys || bits < 1 || bits > 5 || n < 0) return 1;
    for (int64_t i = 0; i < n; ++i) {
        float seg[6];
        keys[i] = fp_mode == OR_FP_FMA ? order_key_fma(tree, opt, origins + 3 * i, dirs + 3 * i, bits, seg)
                                       : order_key_strict(tree, opt, origins + 3 * i, dirs + 3 * i, bits, seg);
        if (segments) memcpy(segments + 6 * i, seg, sizeof seg);
    }
    return 0;
}
