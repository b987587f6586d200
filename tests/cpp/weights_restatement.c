/*
 * weights_restatement.c -- the yardstick of the vr_accumulate_weights tests (TEST INFRASTRUCTURE).
 *
 * The oracle renders pixels; it has no per-leaf output.  This file restates the loop of trace_ray
 * (oracle/vr_oracle_core.inc, rt_core.cuh:108-175) WITHOUT the colour and hands out, for one frame,
 *   per leaf slot (node * N^3 + child slot in the file's numbering: what the oracle's query returns)
 *     max_weight = the largest weight = light_intensity * (1.f - att) of a sample with sigma > sigma_thresh
 *                  that fell into the slot, over the weights > 0 (a weight <= 0 or NaN only counts),
 *     hits       = the number of such samples, modulo 2^32,
 *   both ACCUMULATED into what the arrays hold (the caller zeroes them once; frames are added call by call);
 *   per pixel D, T and stop as tests/cpp/aov_restatement.c defines them (the tie to the oracle's pixels);
 *   the number of hit samples whose weight was <= 0 or NaN.
 * Everything around the loop -- ray generation, NDC warp, the ray/box test, the tree query, the step -- is
 * the oracle's own code, included and called.  The frame is offscreen: tmax comes from render_bbox alone.
 *
 * Build: gcc -O2 -std=c11 -ffp-contract=off -mfma -fPIC -shared -I oracle (the oracle's flags).
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vr_oracle.h"
#include "vr_detmath.h"

#define VR_FMA 0
#include "vr_oracle_core.inc"
#undef VR_FMA
#define VR_FMA 1
#include "vr_oracle_core.inc"
#undef VR_FMA

static inline float madd_strict(float a, float b, float c) { return a * b + c; }
static inline float madd_fma(float a, float b, float c) { return fmaf(a, b, c); }

typedef struct {
    float* max_weight;
    uint32_t* hits;
    uint64_t nonpositive;
} LeafOut;

#define DEFINE_WEIGHTS_PIXEL(M)                                                                      \
    static void weights_pixel_##M(const OrTree* tree, const OrCamera* cam, const OrOptions* opt,      \
                                  int x, int y, LeafOut* lo, float* D_out, float* T_out,              \
                                  uint8_t* stop_out) {                                                \
        float D = 0.f, light = 1.f, dir[3], cen[3];                                                   \
        *D_out = 0.f;                                                                                 \
        *T_out = 1.f;                                                                                 \
        *stop_out = 0;                                                                                \
        if (!(tree->N > 0)) return;                                                                   \
        /* render_pixel, volrend.cu:135-148 */                                                        \
        screen2worlddir_##M(x, y, cam, dir, cen);                                                     \
        maybe_world2ndc_##M(tree, dir, cen);                                                          \
        for (int i = 0; i < 3; ++i) cen[i] = madd_##M(tree->scale[i], cen[i], tree->offset[i]);       \
        float tmax_bg = 1e9f;                                                                         \
        /* trace_ray up to the ray/box test, rt_core.cuh:52-92 */                                     \
        dir[0] *= tree->scale[0];                                                                     \
        dir[1] *= tree->scale[1];                                                                     \
        dir[2] *= tree->scale[2];                                                                     \
        const float delta_scale = 1.f / norm3_##M(dir);                                               \
        dir[0] *= delta_scale;                                                                        \
        dir[1] *= delta_scale;                                                                        \
        dir[2] *= delta_scale;                                                                        \
        tmax_bg /= delta_scale;                                                                       \
        float tmin, tmax, invdir[3];                                                                  \
        for (int i = 0; i < 3; ++i) invdir[i] = (float)(1.0 / ((double)dir[i] + 1e-9));               \
        dda_world_##M(cen, invdir, &tmin, &tmax, opt->render_bbox);                                   \
        tmax = vr_minf(tmax, tmax_bg);                                                                \
        if (tmax < 0 || tmin > tmax) return;                                                          \
        /* the loop, rt_core.cuh:108-175, without the colour */                                       \
        float t = tmin, cube_sz, pos[3];                                                              \
        while (t < tmax) {                                                                            \
            pos[0] = madd_##M(t, dir[0], cen[0]);                                                     \
            pos[1] = madd_##M(t, dir[1], cen[1]);                                                     \
            pos[2] = madd_##M(t, dir[2], cen[2]);                                                     \
            int levels;                                                                               \
            const int64_t leaf = query_##M(tree, pos, &cube_sz, &levels);                             \
            const uint16_t* tree_val = tree->data + leaf * tree->data_dim;                            \
            const float t_subcube = dda_unit_##M(pos, invdir) / cube_sz;                              \
            const float delta_t = t_subcube + opt->step_size;                                         \
            const float sigma = vr_half_bits_to_float(tree_val[tree->data_dim - 1]);                  \
            if (sigma > opt->sigma_thresh) {                                                          \
                const float att = vr_det_expf(-delta_t * delta_scale * sigma);                        \
                const float weight = light * (1.f - att);                                             \
                /* the per-sample rule of vr_accumulate_weights */                                    \
                lo->hits[leaf] += 1u;                                                                 \
                if (weight > 0.f) {                                                                   \
                    if (weight > lo->max_weight[leaf]) lo->max_weight[leaf] = weight;                 \
                } else {                                                                              \
                    lo->nonpositive += 1u;                                                            \
                }                                                                                     \
                D = madd_##M(weight, t, D);                                                           \
                light *= att;                                                                         \
                if (light < opt->stop_thresh) {                                                       \
                    *stop_out = 1;                                                                    \
                    break;                                                                            \
                }                                                                                     \
            }                                                                                         \
            t += delta_t;                                                                             \
        }                                                                                             \
        *D_out = D;                                                                                   \
        *T_out = light;                                                                               \
    }

DEFINE_WEIGHTS_PIXEL(strict)
DEFINE_WEIGHTS_PIXEL(fma)

/* All pixels of one frame.  max_weight / hits: [capacity * N^3], accumulated into; D, T: [height][width]
 * floats, stop: [height][width] bytes; *nonpositive: hit samples with weight <= 0 or NaN (set, not added). */
int weights_restate(const OrTree* tree, const OrCamera* cam, const OrOptions* opt, int fp_mode,
                    float* max_weight, uint32_t* hits, float* D, float* T, uint8_t* stop,
                    uint64_t* nonpositive) {
    if (!tree || !cam || !opt || !max_weight || !hits || !D || !T || !stop || !nonpositive) return 1;
    LeafOut lo = {max_weight, hits, 0};
    for (int y = 0; y < cam->height; ++y)
        for (int x = 0; x < cam->width; ++x) {
            const size_t i = (size_t)y * (size_t)cam->width + (size_t)x;
            if (fp_mode == OR_FP_FMA) weights_pixel_fma(tree, cam, opt, x, y, &lo, D + i, T + i, stop + i);
            else weights_pixel_strict(tree, cam, opt, x, y, &lo, D + i, T + i, stop + i);
        }
    *nonpositive = lo.nonpositive;
    return 0;
}
