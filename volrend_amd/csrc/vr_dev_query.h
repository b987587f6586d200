// vr_dev_query.h -- point query: which leaf holds a position.  The literal float descent of the
// reference (any N) and the N == 2 lookup through the top grid and the bricks (vr_dev_layout.h).
// Device code only.
#pragma once
#include "vr_device_math.h"
#include "vr_dev_layout.h"

namespace vr {

namespace {

// octree point query, n3tree_query.hpp:13-48 -- literal float descent (any N).
// xyz is rewritten to leaf-local coordinates; returns the leaf slot index.
template <int FMA, bool COUNT = false>
__device__ __forceinline__ int64_t query_generic(const KParams& p, float* xyz, float* cube_sz,
                                                 int* levels, uint32_t* word) {
    using P = Policy<FMA>;
    const float fN = (float)p.N;
    const float hi = 1.f - 1e-6f;
#pragma unroll
    for (int i = 0; i < 3; ++i) xyz[i] = vmax(vmin(xyz[i], hi), 0.f);
    int64_t node = 0;
    *cube_sz = fN;
    int64_t sub_ptr = 0;
    uint32_t w = kLeafBit;
    int l = 0;
    for (; l < 64; ++l) {
        float index = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xyz[i] *= fN;
            const float k = __builtin_floorf(xyz[i]);
            index = P::madd(index, fN, k);
            xyz[i] -= k;
        }
        sub_ptr = node * p.N3 + (int32_t)index;
        w = p.nodes[sub_ptr];
        if (COUNT) touch(p, TOUCH_NODES, (uint64_t)sub_ptr * 4u, 4u);
        if (w & kLeafBit) break;
        *cube_sz *= fN;
        node = (int64_t)w;
    }
    *levels = l + 1;
    *word = w;
    return sub_ptr;
}

// Per-lane traversal cache for the N == 2 lookup: the top cell of the previous sample and
// its entry.
struct Cursor {
    uint32_t cell = 0xFFFFFFFFu;  // top cell index (no sample yet: matches nothing)
    uint32_t e0 = 0, e1 = 0;      // top[cell]
};

// N == 2: the float recurrence {x*=2; k=floor(x); x-=k} is exact in binary32, so
// the level-l digit is bit (23-l) of floor(x * 2^24) and the leaf-local
// coordinate is fract(x * 2^d) for a leaf of depth d -- same leaf, same bits, no float
// chain, and the digits of several levels index a table at once.
// Valid while the deepest leaf has d <= 24 (checked at upload); tests/test_gpu_device_forms.py (n2_axis)
// compares clamp, digits and the local coordinate of every depth 1..24 with the recurrence for every non-NaN x.
// Returns the leaf id; *depth = d (child words the reference reads = d), *word low 16 bits = sigma.
// BLK: entry order of the bricks -- 0 x-major, 1 blocked (both compile-time: the production flavours
// exist once per order, a launch-uniform branch in the march round costs C1 1.5 %), -1 = as
// KParams.brick_blocked says (the instrumented flavours).
template <bool COUNT = false, int BLK = -1>
__device__ __forceinline__ uint32_t query_n2(const KParams& p, float* xyz, int* depth,
                                             uint32_t* word, Cursor& cur) {
    // clamp to [0, 1 - 1e-6] (n3tree_query.hpp:17-19) as ONE v_med3_f32 per axis: identical to
    // max(min(x, hi), 0) for every non-NaN x (-0 -> +0 included).  Deviation, non-finite poses
    // only: the reference's max(min(NaN, hi), 0) is `hi` (fminf / fmaxf drop the NaN), the
    // median of (NaN, 0, hi) is 0 -- such a ray samples the other corner of the volume
    const float hi = 1.f - 1e-6f;
    xyz[0] = __builtin_amdgcn_fmed3f(xyz[0], 0.f, hi);
    xyz[1] = __builtin_amdgcn_fmed3f(xyz[1], 0.f, hi);
    xyz[2] = __builtin_amdgcn_fmed3f(xyz[2], 0.f, hi);
    const uint32_t ux = (uint32_t)(xyz[0] * 16777216.f);
    const uint32_t uy = (uint32_t)(xyz[1] * 16777216.f);
    const uint32_t uz = (uint32_t)(xyz[2] * 16777216.f);
    const uint32_t g0 = (uint32_t)p.top_levels, sh0 = 24u - g0;
    const uint32_t cell = ((((ux >> sh0) << g0) | (uy >> sh0)) << g0) | (uz >> sh0);
    if (cell != cur.cell) {
        // 32-bit byte offsets from a uniform base (top: <= 128 MB; bricks: < 4 GB, upload)
        const uint2 e = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(p.top) + (cell << 3));
        if (COUNT) touch(p, TOUCH_TOP, (uint64_t)cell * 8u, 8u);
        cur.cell = cell;
        cur.e0 = e.x;
        cur.e1 = e.y;
    }
    uint32_t w = cur.e0, id = cur.e1;
    int d;
    if (w & kLeafBit) {
        d = (int)__builtin_amdgcn_ubfe(w, 16u, 5u);
    } else {
        const uint32_t bl = (uint32_t)p.brick_levels, sh1 = sh0 - bl;
        uint32_t sub;
        if (BLK > 0 || (BLK < 0 && p.brick_blocked)) {  // (compile-time, or launch-uniform)
            // 8^3 bricks in entry order [x2 y2 z2 z1 | x1 x0 y1 y0 z0]: a 128-byte line holds a
            // 4 x 4 x 2 block of entries instead of a 1 x 4 x 8 slab -- a ray crosses 3.5 lines of
            // a brick instead of 4.8 (chosen per tree at upload: layout comment at the top)
            const uint32_t lo = (((__builtin_amdgcn_ubfe(ux, sh1, 2u) << 2) |
                                  __builtin_amdgcn_ubfe(uy, sh1, 2u)) << 1) |
                                __builtin_amdgcn_ubfe(uz, sh1, 1u);
            const uint32_t hi = (((__builtin_amdgcn_ubfe(ux, sh1 + 2u, 1u) << 1) |
                                  __builtin_amdgcn_ubfe(uy, sh1 + 2u, 1u)) << 2) |
                                __builtin_amdgcn_ubfe(uz, sh1 + 1u, 2u);
            sub = (hi << 5) | lo;
        } else {
            sub = (((__builtin_amdgcn_ubfe(ux, sh1, bl) << bl) | __builtin_amdgcn_ubfe(uy, sh1, bl)) << bl) |
                  __builtin_amdgcn_ubfe(uz, sh1, bl);
        }
        const uint32_t entry = (w << (3u * bl)) + sub;
        if (COUNT) touch(p, TOUCH_BRICKS, (uint64_t)entry * 4u, 4u);
        w = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.bricks) + (entry << 2));
        if (w & kLeafBit) {
            d = (int)(g0 + 1u + __builtin_amdgcn_ubfe(w, 29u, 2u));
            id = (id << 3) + __builtin_amdgcn_ubfe(w, 16u, 13u);  // (root + delta) * 8 + slot
        } else {
            // deeper than the brick: one child word per level (32-bit byte offsets: the node
            // array is < 4 GB, checked at upload)
            const char* nodes_base = reinterpret_cast<const char*>(p.nodes);
            uint32_t node = w, slot;
            int l = (int)(g0 + bl);
            for (;; ++l) {
                const uint32_t sh = (uint32_t)(23 - l);
                slot = (__builtin_amdgcn_ubfe(ux, sh, 1u) << 2) |
                       (__builtin_amdgcn_ubfe(uy, sh, 1u) << 1) | __builtin_amdgcn_ubfe(uz, sh, 1u);
                w = *reinterpret_cast<const uint32_t*>(nodes_base + (node * 8u + slot) * 4u);
                if (COUNT) touch(p, TOUCH_NODES, (uint64_t)(node * 8u + slot) * 4u, 4u);
                if ((w & kLeafBit) || l >= 23) break;
                node = w;
            }
            d = l + 1;
            id = node * 8u + slot;
        }
    }
    *depth = d;
    *word = w;
    const float cs = u2f((uint32_t)(127 + d) << 23);  // 2^d
    xyz[0] = __builtin_amdgcn_fractf(xyz[0] * cs);
    xyz[1] = __builtin_amdgcn_fractf(xyz[1] * cs);
    xyz[2] = __builtin_amdgcn_fractf(xyz[2] * cs);
    return id;
}

// rt_core.cuh:37-49
template <int FMA>
__device__ __forceinline__ float dda_unit(const float* cen, const float* invdir) {
    using P = Policy<FMA>;
    float tmax = 1e4f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t1 = -cen[i] * invdir[i];
        const float t2 = FMA ? P::madd(-cen[i], invdir[i], invdir[i]) : (t1 + invdir[i]);
        tmax = vmin(tmax, vmax(t1, t2));
    }
    return tmax;
}

}  // namespace

}  // namespace vr
