/*
 * march_restatement.h -- the one restatement of trace_ray's loop (TEST INFRASTRUCTURE).
 *
 * The oracle renders pixels: it hands out no depth sum, no final transmittance, no leaf of a sample.  This
 * header restates the march of trace_ray (oracle/vr_oracle_core.inc, rt_core.cuh:52-175) WITHOUT the colour,
 * once per FP model, and gives per ray a MarchRay and per hit sample (sigma > sigma_thresh) a call of `hit`.
 * Everything around the loop -- ray generation, NDC warp, the ray/box test, the tree query, the step, the
 * attenuation -- is the oracle's own code, included here (both FP models) and called.  The consumers are
 * aov_restatement.c (per-pixel planes), weights_restatement.c (per-leaf weights) and grad_restatement.c (the
 * record of the hits); tests/test_{aov,weights,grad}_restatement.py tie each of them back to or_render on
 * every pixel.
 *
 * Build: tests/build_util.py c_library (the oracle's flags).
 */
#ifndef MARCH_RESTATEMENT_H
#define MARCH_RESTATEMENT_H

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
#define VR_FMA 1
#include "vr_oracle_core.inc"
#undef VR_FMA

static inline float madd_strict(float a, float b, float c) { return a * b + c; }
static inline float madd_fma(float a, float b, float c) { return fmaf(a, b, c); }

typedef struct {
    float D;           /* sum of weight * t over the hit samples, in order: D = madd(weight, t, D) */
    float T;           /* light_intensity when the ray leaves the loop */
    float delta_scale; /* of the ray, also when it misses the box; 1 for a tree with N <= 0 */
    int entered;       /* the ray passed the ray/box test */
    int stopped;       /* stop_thresh ended it */
    float vdir[3];     /* the view direction before the NDC warp (what precalc_basis takes) */
} MarchRay;

/* Called for every sample with sigma > sigma_thresh, before light *= att; leaf is the oracle's query result
 * (node * N^3 + child slot, file numbering), delta = fl(delta_t * delta_scale), weight = light * (1.f - att).
 * A non-zero return aborts the march. */
typedef int (*MarchHit)(void* ctx, int64_t leaf, float t, float delta, float weight);

/* One pixel.  offscreen != 0 or depth_init == NULL: tmax comes from render_bbox alone; otherwise depth_init
 * ([height][width]) bounds it.  hit may be NULL.  Returns what hit returned, else 0. */
#define DEFINE_MARCH_PIXEL(M)                                                                         \
    static int march_pixel_##M(const OrTree* tree, const OrCamera* cam, const OrOptions* opt,         \
                               int offscreen, const float* depth_init, int x, int y, MarchRay* out,   \
                               MarchHit hit, void* ctx) {                                             \
        float D = 0.f, light = 1.f, dir[3], cen[3];                                                   \
        memset(out, 0, sizeof *out);                                                                  \
        out->T = 1.f;                                                                                 \
        out->delta_scale = 1.f;                                                                       \
        if (!(tree->N > 0)) return 0;                                                                 \
        /* render_pixel, volrend.cu:135-148 */                                                        \
        screen2worlddir_##M(x, y, cam, dir, cen);                                                     \
        for (int i = 0; i < 3; ++i) out->vdir[i] = dir[i];                                            \
        maybe_world2ndc_##M(tree, dir, cen);                                                          \
        for (int i = 0; i < 3; ++i) cen[i] = madd_##M(tree->scale[i], cen[i], tree->offset[i]);       \
        float tmax_bg = 1e9f;                                                                         \
        if (!offscreen && depth_init) tmax_bg = depth_init[(size_t)y * (size_t)cam->width + x];       \
        /* trace_ray up to the ray/box test, rt_core.cuh:52-92 */                                     \
        dir[0] *= tree->scale[0];                                                                     \
        dir[1] *= tree->scale[1];                                                                     \
        dir[2] *= tree->scale[2];                                                                     \
        const float delta_scale = 1.f / norm3_##M(dir);                                               \
        dir[0] *= delta_scale;                                                                        \
        dir[1] *= delta_scale;                                                                        \
        dir[2] *= delta_scale;                                                                        \
        tmax_bg /= delta_scale;                                                                       \
        out->delta_scale = delta_scale;                                                               \
        float tmin, tmax, invdir[3];                                                                  \
        for (int i = 0; i < 3; ++i) invdir[i] = (float)(1.0 / ((double)dir[i] + 1e-9));               \
        dda_world_##M(cen, invdir, &tmin, &tmax, opt->render_bbox);                                   \
        tmax = vr_minf(tmax, tmax_bg);                                                                \
        if (tmax < 0 || tmin > tmax) return 0;                                                        \
        out->entered = 1;                                                                             \
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
                if (hit) {                                                                            \
                    const int rc = hit(ctx, leaf, t, delta_t * delta_scale, weight);                  \
                    if (rc) return rc;                                                                \
                }                                                                                     \
                D = madd_##M(weight, t, D);                                                           \
                light *= att;                                                                         \
                if (light < opt->stop_thresh) {                                                       \
                    out->stopped = 1;                                                                 \
                    break;                                                                            \
                }                                                                                     \
            }                                                                                         \
            t += delta_t;                                                                             \
        }                                                                                             \
        out->D = D;                                                                                   \
        out->T = light;                                                                               \
        return 0;                                                                                     \
    }

DEFINE_MARCH_PIXEL(strict)
DEFINE_MARCH_PIXEL(fma)

static int march_pixel(const OrTree* tree, const OrCamera* cam, const OrOptions* opt, int fp_mode,
                       int offscreen, const float* depth_init, int x, int y, MarchRay* out, MarchHit hit,
                       void* ctx) {
    return fp_mode == OR_FP_FMA ? march_pixel_fma(tree, cam, opt, offscreen, depth_init, x, y, out, hit, ctx)
                                : march_pixel_strict(tree, cam, opt, offscreen, depth_init, x, y, out, hit, ctx);
}

#endif
