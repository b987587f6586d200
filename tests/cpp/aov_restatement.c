/*
 * aov_restatement.c -- the yardstick of the vr_render_aov tests (TEST INFRASTRUCTURE).
 *
 * The oracle has no depth sum D and no final transmittance T of their own: its depth mode only shows
 * min(0.3 * D, 1), rescaled at an early stop.  This file hands out, per pixel, what the one restatement of
 * the march (march_restatement.h) gives of a ray: D, T, ds = delta_scale and stop.
 * tests/test_aov_restatement.py ties D, T and stop back to or_render on every pixel.
 */
#include "march_restatement.h"

/* All pixels of a frame; D, T, ds: [height][width] floats, stop: [height][width] bytes. */
int aov_restate(const OrTree* tree, const OrCamera* cam, const OrOptions* opt, int fp_mode, int offscreen,
                const float* depth_init, float* D, float* T, float* ds, uint8_t* stop) {
    if (!tree || !cam || !opt || !D || !T || !ds || !stop) return 1;
    for (int y = 0; y < cam->height; ++y)
        for (int x = 0; x < cam->width; ++x) {
            const size_t i = (size_t)y * (size_t)cam->width + (size_t)x;
            MarchRay ray;
            march_pixel(tree, cam, opt, fp_mode, offscreen, depth_init, x, y, &ray, NULL, NULL);
            D[i] = ray.D;
            T[i] = ray.T;
            ds[i] = ray.delta_scale;
            stop[i] = (uint8_t)ray.stopped;
        }
    return 0;
}
