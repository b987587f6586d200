/*
 * grad_restatement.c -- the yardstick of the vr_render_backward tests (TEST INFRASTRUCTURE).
 *
 * Two steps.
 *   grad_trace_frame   marches every pixel of one offscreen frame with the one restatement of the march
 *                      (march_restatement.h, either FP model) and RECORDS what the differentiation treats as
 *                      constants: per ray its pixel, its basis values (the oracle's precalc_basis; zero for a ray
 *                      that misses the box), whether stop_thresh ended it, and per hit sample (sigma >
 *                      sigma_thresh) the leaf slot in the file's numbering and delta = fl(delta_t * delta_scale).
 *   grad_eval64 / grad_eval32   evaluate the formulas of include/volrend_hip.h (vr_render_backward) on such a
 *                      record, with the VALUES (sigma and the record entries) taken from an array the caller
 *                      hands in -- so a caller can perturb a value with every decision frozen.
 *       grad_eval64    everything in binary64: out[4] per pixel, sum of the weights per pixel, the gradient
 *                      per element of data (added into), and per element the magnitude M: the same sum with
 *                      every factor and term replaced by its absolute value and every difference by a sum
 *                      (w_i = T_i - T_{i+1} counts as T_i + T_{i+1}, 1 - c as 1 + c; s is a factor), and
 *                      the underflow magnitude U: M with every transmittance factor (T_i, w_i, T_{K+1}) replaced
 *                      by 1 -- binary32 carries a transmittance below 2^-126 with an ABSOLUTE error of up to
 *                      that much (a light that decays to 1e-60 sticks at a subnormal), which no bound relative
 *                      to M covers; 2^-126 U does.  U also carries eight smallest subnormals per contribution
 *                      (SUBNORMAL_UNITS): a product that comes out below 2^-149 is zero in binary32.
 *                      Two more magnitudes, for records whose sigmoid argument u is large (optional outputs):
 *                      M_c is M with every colour-dependent factor of sample i, channel ch -- the c (1 + c) of
 *                      the coefficient terms, the |g_ch c_ch| inside G_abs, R_abs and C^_abs -- multiplied by
 *                      1 + A_{i,ch}, A_{i,ch} = sum_b |B_b| |k_{i,ch,b}| (0 for RGBA): the binary32 dot product
 *                      u carries an absolute error of about 2^-24 A, which is the RELATIVE error of exp(-u)
 *                      and so of 1 - c or c, whichever is small.  U_c is U with every colour factor replaced
 *                      by 1 as well (the coefficient term 2 |g_ch s B_b|, the sigma term with |g_ch| for
 *                      |g_ch c_ch|): binary32 gives c = 1 / (1 + inf) = 0 where binary64 gives 1e-48.
 *       grad_eval32    the same formulas in binary32, rays taken in a caller-given order and every
 *                      contribution added into a binary32 array as it comes.  -DGRAD_MUTANT=n (1..3) builds
 *                      this entry point -- and only this one -- with one deliberate mistake, for the tests
 *                      that show the error unit still sees it:
 *                        1  dc formed without the (1 - c) factor
 *                        2  R_i formed in binary32 as total minus running prefix
 *                        3  the not-stopped tail g_3 T_{K+1} used for stopped rays
 */
#include "march_restatement.h"

/* A contribution is a chain of binary32 products; one whose result is subnormal carries an absolute error of half
 * the smallest subnormal, 2^-150.  Per contribution U gets 2^-20: 2^-126 * 2^-20 = eight smallest subnormals. */
#define SUBNORMAL_UNITS 0x1p-20

#ifndef GRAD_MUTANT
#define GRAD_MUTANT 0
#endif

typedef struct {
    int64_t slot;  /* node * N^3 + child slot, file numbering */
    float delta;   /* fl(delta_t * delta_scale) */
} GradHit;

typedef struct {
    int32_t pixel;    /* y * width + x */
    int32_t stopped;  /* stop_thresh ended the ray at its last hit */
    int32_t entered;  /* the ray passed the ray/box test: the device gives it a lane */
    int64_t first, n; /* its hits: hits[first .. first + n) */
    float basis[25];
} GradRay;

typedef struct {
    GradRay* rays;
    int64_t n_rays, cap_rays;
    GradHit* hits;
    int64_t n_hits, cap_hits;
    int32_t width, height;
    int32_t data_dim, basis_dim, n_basis; /* n_basis: basis functions the renderer uses; 0 = RGBA */
} GradTrace;

/* MarchHit: records the sample */
static int push_hit(void* ctx, int64_t slot, float t, float delta, float weight) {
    GradTrace* tr = (GradTrace*)ctx;
    (void)t;
    (void)weight;
    if (tr->n_hits == tr->cap_hits) {
        const int64_t cap = tr->cap_hits ? tr->cap_hits * 2 : 4096;
        GradHit* h = (GradHit*)realloc(tr->hits, (size_t)cap * sizeof(GradHit));
        if (!h) return 1;
        tr->hits = h;
        tr->cap_hits = cap;
    }
    tr->hits[tr->n_hits].slot = slot;
    tr->hits[tr->n_hits].delta = delta;
    tr->n_hits++;
    return 0;
}

void grad_trace_free(GradTrace* tr) {
    if (!tr) return;
    free(tr->rays);
    free(tr->hits);
    free(tr);
}

/* One frame, scanline order: ray r is pixel r. */
GradTrace* grad_trace_frame(const OrTree* tree, const OrCamera* cam, const OrOptions* opt, int fp_mode) {
    if (!tree || !cam || !opt) return NULL;
    GradTrace* tr = (GradTrace*)calloc(1, sizeof(GradTrace));
    if (!tr) return NULL;
    tr->width = cam->width;
    tr->height = cam->height;
    tr->data_dim = tree->data_dim;
    tr->basis_dim = tree->basis_dim;
    if (tree->basis_dim < 0) tr->n_basis = 0;
    else if (tree->basis_dim == 4 || tree->basis_dim == 9 || tree->basis_dim == 16 || tree->basis_dim == 25)
        tr->n_basis = tree->basis_dim;
    else tr->n_basis = 1;
    tr->n_rays = tr->cap_rays = (int64_t)cam->width * cam->height;
    tr->rays = (GradRay*)calloc((size_t)tr->n_rays, sizeof(GradRay));
    if (!tr->rays) {
        grad_trace_free(tr);
        return NULL;
    }
    for (int y = 0; y < cam->height; ++y)
        for (int x = 0; x < cam->width; ++x) {
            GradRay* ray = tr->rays + ((int64_t)y * cam->width + x); /* (calloc: basis is zero for a miss) */
            MarchRay m;
            ray->pixel = y * cam->width + x;
            ray->first = tr->n_hits;
            if (march_pixel(tree, cam, opt, fp_mode, 1, NULL, x, y, &m, push_hit, tr)) {
                grad_trace_free(tr);
                return NULL;
            }
            ray->n = tr->n_hits - ray->first;
            ray->stopped = m.stopped;
            ray->entered = m.entered;
            if (m.entered && tr->n_basis > 0) {
                if (fp_mode == OR_FP_FMA) precalc_basis_fma(tree, m.vdir, ray->basis);
                else precalc_basis_strict(tree, m.vdir, ray->basis);
            }
        }
    return tr;
}

/* Per pixel: hit samples, and whether the ray was stopped. */
void grad_trace_rays(const GradTrace* tr, int64_t* n_hits, uint8_t* stopped) {
    for (int64_t r = 0; r < tr->n_rays; ++r) {
        n_hits[r] = tr->rays[r].n;
        stopped[r] = (uint8_t)tr->rays[r].stopped;
    }
}

/* Per pixel: whether the ray entered the volume (a ray that did not is never marched). */
void grad_trace_entered(const GradTrace* tr, uint8_t* entered) {
    for (int64_t r = 0; r < tr->n_rays; ++r) entered[r] = (uint8_t)(tr->rays[r].entered != 0);
}

/* The slots of ray r's hits, in march order (out: ray's n entries). */
void grad_trace_slots(const GradTrace* tr, int64_t r, int64_t* out) {
    const GradRay* ray = tr->rays + r;
    for (int64_t i = 0; i < ray->n; ++i) out[i] = tr->hits[ray->first + i].slot;
}

/* The slots of every ray's hits, ray after ray (out: the sum of grad_trace_rays' n_hits entries). */
void grad_trace_all_slots(const GradTrace* tr, int64_t* out) {
    for (int64_t r = 0; r < tr->n_rays; ++r) {
        const GradRay* ray = tr->rays + r;
        for (int64_t i = 0; i < ray->n; ++i) *out++ = tr->hits[ray->first + i].slot;
    }
}

/* Colour of one sample in binary64; dc = d colour / d (record entry of basis function b) without B_b;
 * amp = 1 + A, A = sum_b |B_b| |k_b| (the size of the terms of u; 1 for RGBA). */
static void colour64(const GradTrace* tr, const GradRay* ray, const double* v, double* c, double* dc, double* amp) {
    for (int ch = 0; ch < 3; ++ch) {
        if (tr->n_basis == 0) {
            c[ch] = v[ch];
            dc[ch] = 1.0;
            amp[ch] = 1.0;
        } else {
            double u = 0.0, A = 0.0;
            for (int b = 0; b < tr->n_basis; ++b) {
                u += (double)ray->basis[b] * v[ch * tr->basis_dim + b];
                A += fabs((double)ray->basis[b] * v[ch * tr->basis_dim + b]);
            }
            amp[ch] = 1.0 + A;
            c[ch] = 1.0 / (1.0 + exp(-u));
            dc[ch] = c[ch] * (1.0 - c[ch]);
        }
    }
}

/*
 * data: [n_slots * data_dim] binary64 values (file order).  g: [height * width * 4] binary64.
 * out: [height * width * 4] or NULL; wsum: [height * width] (sum of the w_i) or NULL;
 * grad, mag, under: [n_slots * data_dim] ADDED INTO, or all NULL (forward only).
 */
int grad_eval64(const GradTrace* tr, const double* data, const double* g_all, double* out, double* wsum,
                double* grad, double* mag, double* under) {
    if (!tr || !data) return 1;
    const int dd = tr->data_dim, nb = tr->n_basis, bd = tr->basis_dim;
    double* suf = NULL;
    int64_t suf_cap = 0;
    for (int64_t r = 0; r < tr->n_rays; ++r) {
        const GradRay* ray = tr->rays + r;
        const GradHit* h = tr->hits + ray->first;
        const int64_t K = ray->n;
        /* forward: totals */
        double T = 1.0, C[3] = {0, 0, 0}, Chat = 0.0, Chat_abs = 0.0, Gsum_abs = 0.0;
        const double* g = g_all ? g_all + 4 * (int64_t)ray->pixel : NULL;
        for (int64_t i = 0; i < K; ++i) {
            const double* v = data + h[i].slot * dd;
            const double a = exp(-(double)h[i].delta * v[dd - 1]);
            const double w = T - T * a;
            double c[3], dc[3], amp[3];
            colour64(tr, ray, v, c, dc, amp);
            for (int ch = 0; ch < 3; ++ch) C[ch] += w * c[ch];
            if (g) {
                Chat += w * (g[0] * c[0] + g[1] * c[1] + g[2] * c[2]);
                Chat_abs += (T + T * a) * (fabs(g[0] * c[0]) + fabs(g[1] * c[1]) + fabs(g[2] * c[2]));
                Gsum_abs += 2.0 * (fabs(g[0] * c[0]) + fabs(g[1] * c[1]) + fabs(g[2] * c[2]));
            }
            T *= a;
        }
        const double Tend = T;
        const double s = ray->stopped ? 1.0 / (1.0 - Tend) : 1.0;
        if (out) {
            double* o = out + 4 * (int64_t)ray->pixel;
            o[0] = s * C[0];
            o[1] = s * C[1];
            o[2] = s * C[2];
            o[3] = ray->stopped ? 1.0 : (K > 0 ? 1.0 - Tend : 0.0);
        }
        if (wsum) wsum[ray->pixel] = 1.0 - Tend;
        if (!grad || !mag || !under || !g) continue;
        /* backward: R_i = what is still to come behind sample i, summed last sample first (three suffix sums per
         * hit: of w G, of |w| |G| and of |G|) */
        if (K > suf_cap) {
            free(suf);
            suf_cap = 2 * K;
            suf = (double*)malloc((size_t)suf_cap * 3 * sizeof(double));
            if (!suf) return 1;
        }
        T = 1.0;
        for (int64_t i = 0; i < K; ++i) {
            const double* v = data + h[i].slot * dd;
            const double a = exp(-(double)h[i].delta * v[dd - 1]);
            const double w = T - T * a;
            double c[3], dc[3], amp[3];
            colour64(tr, ray, v, c, dc, amp);
            const double G_abs = fabs(g[0] * c[0]) + fabs(g[1] * c[1]) + fabs(g[2] * c[2]);
            suf[3 * i + 0] = w * (g[0] * c[0] + g[1] * c[1] + g[2] * c[2]);
            suf[3 * i + 1] = (T + T * a) * G_abs;
            suf[3 * i + 2] = 2.0 * G_abs;
            T *= a;
        }
        {
            double acc[3] = {0, 0, 0};
            for (int64_t i = K - 1; i >= 0; --i)
                for (int q = 0; q < 3; ++q) {
                    const double term = suf[3 * i + q];
                    suf[3 * i + q] = acc[q];
                    acc[q] += term;
                }
        }
        T = 1.0;
        for (int64_t i = 0; i < K; ++i) {
            const int64_t base = h[i].slot * dd;
            const double* v = data + base;
            const double delta = (double)h[i].delta;
            const double a = exp(-delta * v[dd - 1]);
            const double w = T - T * a, Tn = T * a;
            double c[3], dc[3], amp[3];
            colour64(tr, ray, v, c, dc, amp);
            const double G = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];
            const double G_abs = fabs(g[0] * c[0]) + fabs(g[1] * c[1]) + fabs(g[2] * c[2]);
            const double R = suf[3 * i + 0], R_abs = suf[3 * i + 1], R_one = suf[3 * i + 2];
            for (int ch = 0; ch < 3; ++ch) {
                if (nb == 0) {
                    grad[base + ch] += g[ch] * s * w;
                    mag[base + ch] += fabs(g[ch] * s) * (T + Tn);
                    under[base + ch] += 2.0 * fabs(g[ch] * s) + SUBNORMAL_UNITS;
                } else {
                    for (int b = 0; b < nb; ++b) {
                        const double t = g[ch] * s * w * dc[ch] * (double)ray->basis[b];
                        grad[base + ch * bd + b] += t;
                        const double m1 = fabs(g[ch] * s * (double)ray->basis[b]) * c[ch] * (1.0 + c[ch]);
                        mag[base + ch * bd + b] += m1 * (T + Tn);
                        under[base + ch * bd + b] += 2.0 * m1 + SUBNORMAL_UNITS;
                    }
                }
            }
            if (!ray->stopped) {
                grad[base + dd - 1] += delta * (Tn * G - R + g[3] * Tend);
                mag[base + dd - 1] += fabs(delta) * (fabs(Tn) * G_abs + R_abs + fabs(g[3] * Tend));
                under[base + dd - 1] += fabs(delta) * (G_abs + R_one + fabs(g[3])) + SUBNORMAL_UNITS;
            } else {
                grad[base + dd - 1] += delta * (s * (Tn * G - R) - s * s * Tend * Chat);
                mag[base + dd - 1] += fabs(delta) * (fabs(s) * (fabs(Tn) * G_abs + R_abs) + s * s * fabs(Tend) * Chat_abs);
                under[base + dd - 1] += fabs(delta) * (fabs(s) * (G_abs + R_one) + s * s * Gsum_abs) + SUBNORMAL_UNITS;
            }
            T = Tn;
        }
    }
    free(suf);
    return 0;
}

/*
 * The edge-aware magnitudes M_c and U_c (the comment at the top) of the same record, ADDED INTO mag_c and under_c
 * ([n_slots * data_dim]).  A sibling of grad_eval64 so that grad, M and U keep the bits they had.
 */
int grad_edge64(const GradTrace* tr, const double* data, const double* g_all, double* mag_c, double* under_c) {
    if (!tr || !data || !g_all || !mag_c || !under_c) return 1;
    const int dd = tr->data_dim, nb = tr->n_basis, bd = tr->basis_dim;
    double* suf = NULL; /* per hit, behind it: the sums of (T_j + T_{j+1}) G_c,j and of 2 G_one */
    int64_t suf_cap = 0;
    for (int64_t r = 0; r < tr->n_rays; ++r) {
        const GradRay* ray = tr->rays + r;
        const GradHit* h = tr->hits + ray->first;
        const int64_t K = ray->n;
        const double* g = g_all + 4 * (int64_t)ray->pixel;
        const double G_one = fabs(g[0]) + fabs(g[1]) + fabs(g[2]);
        if (K > suf_cap) {
            free(suf);
            suf_cap = 2 * K;
            suf = (double*)malloc((size_t)suf_cap * 2 * sizeof(double));
            if (!suf) return 1;
        }
        double T = 1.0;
        for (int64_t i = 0; i < K; ++i) {
            const double* v = data + h[i].slot * dd;
            const double a = exp(-(double)h[i].delta * v[dd - 1]);
            double c[3], dc[3], amp[3];
            colour64(tr, ray, v, c, dc, amp);
            const double G_c = fabs(g[0] * c[0]) * amp[0] + fabs(g[1] * c[1]) * amp[1] + fabs(g[2] * c[2]) * amp[2];
            suf[2 * i + 0] = (T + T * a) * G_c;
            suf[2 * i + 1] = 2.0 * G_one;
            T *= a;
        }
        const double Tend = T;
        const double s = ray->stopped ? 1.0 / (1.0 - Tend) : 1.0;
        double acc[2] = {0, 0};
        for (int64_t i = K - 1; i >= 0; --i)
            for (int q = 0; q < 2; ++q) {
                const double term = suf[2 * i + q];
                suf[2 * i + q] = acc[q];
                acc[q] += term;
            }
        const double Chat_c = acc[0], Gsum_one = acc[1];
        T = 1.0;
        for (int64_t i = 0; i < K; ++i) {
            const int64_t base = h[i].slot * dd;
            const double* v = data + base;
            const double delta = (double)h[i].delta;
            const double a = exp(-delta * v[dd - 1]);
            const double Tn = T * a;
            double c[3], dc[3], amp[3];
            colour64(tr, ray, v, c, dc, amp);
            const double G_c = fabs(g[0] * c[0]) * amp[0] + fabs(g[1] * c[1]) * amp[1] + fabs(g[2] * c[2]) * amp[2];
            const double R_c = suf[2 * i + 0], R_one = suf[2 * i + 1];
            for (int ch = 0; ch < 3; ++ch) {
                if (nb == 0) {
                    mag_c[base + ch] += fabs(g[ch] * s) * (T + Tn);
                    under_c[base + ch] += 2.0 * fabs(g[ch] * s) + SUBNORMAL_UNITS;
                } else {
                    for (int b = 0; b < nb; ++b) {
                        const double gsb = fabs(g[ch] * s * (double)ray->basis[b]);
                        mag_c[base + ch * bd + b] += gsb * c[ch] * (1.0 + c[ch]) * amp[ch] * (T + Tn);
                        under_c[base + ch * bd + b] += 2.0 * gsb + SUBNORMAL_UNITS;
                    }
                }
            }
            if (!ray->stopped) {
                mag_c[base + dd - 1] += fabs(delta) * (fabs(Tn) * G_c + R_c + fabs(g[3] * Tend));
                under_c[base + dd - 1] += fabs(delta) * (G_one + R_one + fabs(g[3])) + SUBNORMAL_UNITS;
            } else {
                mag_c[base + dd - 1] += fabs(delta) * (fabs(s) * (fabs(Tn) * G_c + R_c) + s * s * fabs(Tend) * Chat_c);
                under_c[base + dd - 1] += fabs(delta) * (fabs(s) * (G_one + R_one) + s * s * Gsum_one) + SUBNORMAL_UNITS;
            }
            T = Tn;
        }
    }
    free(suf);
    return 0;
}

/*
 * The same formulas in binary32 (the suffix sum R_i formed directly, last sample first), rays in the order
 * order[0 .. n_order), every contribution added into the binary32 array grad as it comes.
 * data: [n_slots * data_dim] binary32 values; g: [height * width * 4] binary32.
 */
int grad_eval32(const GradTrace* tr, const float* data, const float* g_all, const int64_t* order, int64_t n_order,
                float* grad) {
    if (!tr || !data || !g_all || !order || !grad) return 1;
    const int dd = tr->data_dim, nb = tr->n_basis, bd = tr->basis_dim;
    int64_t cap = 0;
    float* buf = NULL; /* per hit: w, Tn, G, R, c(1-c) x 3 */
    for (int64_t q = 0; q < n_order; ++q) {
        const GradRay* ray = tr->rays + order[q];
        const GradHit* h = tr->hits + ray->first;
        const int64_t K = ray->n;
        if (K == 0) continue;
        if (K > cap) {
            free(buf);
            cap = K * 2;
            buf = (float*)malloc((size_t)cap * 7 * sizeof(float));
            if (!buf) return 1;
        }
        const float* g = g_all + 4 * (int64_t)ray->pixel;
        float T = 1.f;
        for (int64_t i = 0; i < K; ++i) {
            const float* v = data + h[i].slot * dd;
            const float a = expf(-h[i].delta * v[dd - 1]);
            float* e = buf + 7 * i;
            float c[3];
            for (int ch = 0; ch < 3; ++ch) {
                if (nb == 0) {
                    c[ch] = v[ch];
                    e[4 + ch] = 1.f;
                } else {
                    float u = 0.f;
                    for (int b = 0; b < nb; ++b) u += ray->basis[b] * v[ch * bd + b];
                    c[ch] = 1.f / (1.f + expf(-u));
#if GRAD_MUTANT == 1
                    e[4 + ch] = c[ch];
#else
                    e[4 + ch] = c[ch] * (1.f - c[ch]);
#endif
                }
            }
            e[0] = T * (1.f - a);
            e[1] = T * a;
            e[2] = g[0] * c[0] + g[1] * c[1] + g[2] * c[2];
            T = e[1];
        }
        const float Tend = T;
        float R = 0.f;
        for (int64_t i = K - 1; i >= 0; --i) {
            buf[7 * i + 3] = R;
            R += buf[7 * i + 0] * buf[7 * i + 2];
        }
        const float Chat = R;
#if GRAD_MUTANT == 2
        {
            float prefix = 0.f;
            for (int64_t i = 0; i < K; ++i) {
                prefix += buf[7 * i + 0] * buf[7 * i + 2];
                buf[7 * i + 3] = Chat - prefix;
            }
        }
#endif
        const float s = ray->stopped ? 1.f / (1.f - Tend) : 1.f;
        for (int64_t i = 0; i < K; ++i) {
            const int64_t base = h[i].slot * dd;
            const float* e = buf + 7 * i;
            for (int ch = 0; ch < 3; ++ch) {
                if (nb == 0) {
                    grad[base + ch] += g[ch] * s * e[0];
                } else {
                    const float f = g[ch] * s * e[0] * e[4 + ch];
                    for (int b = 0; b < nb; ++b) grad[base + ch * bd + b] += f * ray->basis[b];
                }
            }
            if (!ray->stopped) grad[base + dd - 1] += h[i].delta * (e[1] * e[2] - e[3] + g[3] * Tend);
#if GRAD_MUTANT == 3
            else grad[base + dd - 1] += h[i].delta * (s * (e[1] * e[2] - e[3]) + g[3] * Tend);
#else
            else grad[base + dd - 1] += h[i].delta * (s * (e[1] * e[2] - e[3]) - s * s * Tend * Chat);
#endif
        }
    }
    free(buf);
    return 0;
}
