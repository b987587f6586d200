/*
 * weights_restatement.c -- the yardstick of the vr_accumulate_weights tests (TEST INFRASTRUCTURE).
 *
 * The oracle renders pixels; it has no per-leaf output.  This file applies the per-sample rule of
 * vr_accumulate_weights to the hit samples of the one restatement of the march (march_restatement.h) and hands
 * out, for one offscreen frame,
 *   per leaf slot (node * N^3 + child slot in the file's numbering: what the oracle's query returns)
 *     max_weight = the largest weight = light_intensity * (1.f - att) of a sample with sigma > sigma_thresh
 *                  that fell into the slot, over the weights > 0 (a weight <= 0 or NaN only counts),
 *     hits       = the number of such samples, modulo 2^32,
 *   both ACCUMULATED into what the arrays hold (the caller zeroes them once; frames are added call by call);
 *   per pixel D, T and stop of the ray (the tie to the oracle's pixels);
 *   the number of hit samples whose weight was <= 0 or NaN.
 */
#include "march_restatement.h"

typedef struct {
    float* max_weight;
    uint32_t* hits;
    uint64_t nonpositive;
} LeafOut;

static int leaf_hit(void* ctx, int64_t leaf, float t, float delta, float weight) {
    LeafOut* lo = (LeafOut*)ctx;
    (void)t;
    (void)delta;
    lo->hits[leaf] += 1u;
    if (weight > 0.f) {
        if (weight > lo->max_weight[leaf]) lo->max_weight[leaf] = weight;
    } else {
        lo->nonpositive += 1u;
    }
    return 0;
}

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
            MarchRay ray;
            march_pixel(tree, cam, opt, fp_mode, 1, NULL, x, y, &ray, leaf_hit, &lo);
            D[i] = ray.D;
            T[i] = ray.T;
            stop[i] = (uint8_t)ray.stopped;
        }
    *nonpositive = lo.nonpositive;
    return 0;
}
