// vr_query.hip -- bulk point queries (vr_query_points / vr_query_grid): which leaf holds a point,
// what is stored there, and the colour a sample at that point has along a direction.  Every output
// is a pure function of one point (and one direction): no march, no compositing, no launch slot.
// The lookups and the colour are the device functions the render kernels use (vr_dev_query.h,
// vr_dev_shade.h), in the STRICT model.  Built with -ffp-contract=off; see vr_device_math.h.
#include "vr_dev_query.h"
#include "vr_dev_shade.h"
#include "vr_query.h"

namespace vr {

namespace {

// How a kernel flavour finds the leaf: the two lookups differ materially (one or two cached loads
// against a float chain with a load per level), so the flavours that are bound by the lookup exist
// once per kind; the colour flavours are bound by the record read and branch launch-uniformly.
enum { kLookupDescent = 0, kLookupN2 = 1, kLookupAny = -1 };
constexpr int kNoColour = 0;  // COL: 0, or the basis flavour (BASIS_*, vr_internal.h) of the tree

// The up to 64 consecutive output indices [first, first + count) a wave handles at once.
struct Chunk {
    int64_t first;
    int count;
    int gi, gj, gk0;  // grid source: the row (i, j) and its first k
};

template <int SRC>
__device__ __forceinline__ Chunk chunk_at(const QueryArgs& q, int64_t c) {
    Chunk ch;
    if (SRC == kPointsArray) {
        ch.first = c << 6;
        const int64_t left = q.n - ch.first;
        ch.count = left < kWave ? (int)left : kWave;
        ch.gi = ch.gj = ch.gk0 = 0;
    } else {
        const int64_t t = c / q.res[1];
        ch.gj = (int)(c - t * q.res[1]);
        ch.gi = (int)(t / q.k_blocks);
        ch.gk0 = (int)(t - (int64_t)ch.gi * q.k_blocks) << 6;
        ch.first = ((int64_t)ch.gi * q.res[1] + ch.gj) * q.res[2] + ch.gk0;
        const int left = q.res[2] - ch.gk0;
        ch.count = left < kWave ? left : kWave;
    }
    return ch;
}

// [count][3] floats of global memory <-> one triple per lane, through LDS: the wave reads and
// writes whole lines (3 x 256 contiguous bytes) instead of 64 pieces 12 bytes apart.  The block is
// one wave; every lane calls these.
__device__ __forceinline__ void load_triples(const float* src, int count, float* tr, float* v) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int f = c * kWave + lane;
        if (f < count * 3) tr[f] = src[f];
    }
    __syncthreads();
    if (lane < count) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = tr[lane * 3 + c];
    }
    __syncthreads();
}
__device__ __forceinline__ void store_triples(float* dst, int count, float* tr, const float* v) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) tr[lane * 3 + c] = v[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int f = c * kWave + lane;
        if (f < count * 3) dst[f] = tr[f];
    }
    __syncthreads();
}

// rt_core.cuh:125-163 for one sample: the colour of record `leaf` along `dir`, STRICT.
template <int COL>
__device__ __forceinline__ void colour_of(const KParams& p, uint32_t leaf, const float* dir, float* rgb) {
    Record<COL> rec;
    load_record<COL>(p, leaf, rec);
    if constexpr (COL == BASIS_RGBA) {
        rgb[0] = rec.at(0);
        rgb[1] = rec.at(1);
        rgb[2] = rec.at(2);
    } else if constexpr (COL == BASIS_1) {
        // a basis size the reference's switch does not know: basis 0 of each channel (rt_core.cuh:131)
        const float b0 = (float)0.28209479177387814;
        rgb[0] = sigmoid(b0 * rec.at(0));
        rgb[1] = sigmoid(b0 * rec.at(1));
        rgb[2] = sigmoid(b0 * rec.at(2));
    } else {
        float basis_fn[VR_MAX_BASIS];
        precalc_basis<0, false, COL>(p, dir, basis_fn);
        rgb[0] = sigmoid(channel_dot<0, COL, 0>(basis_fn, rec));
        rgb[1] = sigmoid(channel_dot<0, COL, 1>(basis_fn, rec));
        rgb[2] = sigmoid(channel_dot<0, COL, 2>(basis_fn, rec));
    }
}

// The records of the wave's points as floats, [count][K] contiguous in `dst`: the wave walks that
// range 64 pieces at a time, each lane fetching the leaf id of the point its piece belongs to from
// the lane that looked it up.  A piece is V floats of one record: V = 4 (an 8-byte load, a 16-byte
// store: every store instruction writes 1 KB contiguous, 12 lanes share an SH16 record) when K is a
// multiple of 4 and the output is 16-byte aligned, else V = 1 (RGBA, SH1 / 9 / 25, odd pointers).
template <int V>
__device__ __forceinline__ void store_records(const KParams& p, uint32_t leaf, int count, float* dst) {
    const int lane = threadIdx.x;
    const int K = (p.data_dim - 1) / V;  // pieces per record
    const int total = count * K;
    const int dj = kWave / K, di = kWave - dj * K;
    int j = lane / K, i = lane - j * K;
    constexpr int kBatch = 4;  // loads in flight per lane before the first store waits
    for (int f0 = 0; f0 < total; f0 += kBatch * kWave) {  // (wave-uniform trip count: the shuffle needs every lane)
        uint2 h[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t lf = (uint32_t)__shfl((int)leaf, j & (kWave - 1));
            h[u] = make_uint2(0u, 0u);
            if (f0 + u * kWave + lane < total) {
                const uint16_t* src = p.leaves + (uint64_t)lf * (uint32_t)p.leaf_stride_h + (uint32_t)(i * V);
                if (V == 4) h[u] = *reinterpret_cast<const uint2*>(src);  // records are 16-byte aligned
                else h[u].x = *src;
            }
            j += dj;
            i += di;
            if (i >= K) {
                i -= K;
                ++j;
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int f = f0 + u * kWave + lane;
            if (f >= total) continue;
            if (V == 4)
                reinterpret_cast<float4*>(dst)[f] =
                    make_float4(h2f((uint16_t)(h[u].x & 0xFFFFu)), h2f((uint16_t)(h[u].x >> 16)),
                                h2f((uint16_t)(h[u].y & 0xFFFFu)), h2f((uint16_t)(h[u].y >> 16)));
            else
                dst[f] = h2f((uint16_t)h[u].x);
        }
    }
}

// One wave per block.  Block b takes the chunks [b * per, (b + 1) * per): consecutive chunks of a
// wave are neighbours in space when the points are (a grid always, an array when the caller's
// order is), which is what the Cursor of query_n2 pays for.
template <int SRC, int LOOKUP, bool COEFFS, int COL>
__global__ __launch_bounds__(kWave) void query_kernel(const KParams p, const QueryArgs q) {
    __shared__ float tr[3 * kWave];
    const int lane = threadIdx.x;
    const int64_t per = (q.n_chunks + gridDim.x - 1) / gridDim.x;
    int64_t c = per * blockIdx.x, c_end = c + per;
    if (c_end > q.n_chunks) c_end = q.n_chunks;
    const bool n2 = LOOKUP == kLookupAny ? (p.N == 2 && p.top_levels > 0) : LOOKUP == kLookupN2;
    Cursor cur;
    for (; c < c_end; ++c) {
        const Chunk ch = chunk_at<SRC>(q, c);
        const bool active = lane < ch.count;
        float x[3] = {0.5f, 0.5f, 0.5f};  // (idle lanes of the last chunk look up the centre and store nothing)
        if (SRC == kPointsArray) {
            load_triples(q.xyz + ch.first * 3, ch.count, tr, x);
        } else if (active) {
            // one rounding per operator: the coordinate the header documents
            x[0] = q.lo[0] + ((float)ch.gi + 0.5f) * q.cell[0];
            x[1] = q.lo[1] + ((float)ch.gj + 0.5f) * q.cell[1];
            x[2] = q.lo[2] + ((float)(ch.gk0 + lane) + 0.5f) * q.cell[2];
        }
        if (q.space == VR_SPACE_WORLD) {  // volrend.cu:178-180, as probe_kernel
#pragma unroll
            for (int i = 0; i < 3; ++i) x[i] = p.offset[i] + p.scale[i] * x[i];
        }
        // n3tree_query.hpp:17-19 as written there: a NaN becomes 1 - 1e-6f, -0 becomes +0.  The
        // clamp inside the lookups is then the identity (query_n2's median would send NaN to 0).
        const float hi = 1.f - 1e-6f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float v = x[i] < hi ? x[i] : hi;
            x[i] = v > 0.f ? v : 0.f;
        }
        uint32_t leaf, word;
        int depth;
        if (n2) {
            leaf = query_n2<false, -1>(p, x, &depth, &word, cur);
            depth -= 1;  // child words read - 1: what or_query and VrTreeInfo.max_depth count
        } else {
            float cube_sz;
            leaf = (uint32_t)query_generic<0>(p, x, &cube_sz, &depth, &word);
            depth -= 1;
        }
        if (q.sigma && active) q.sigma[ch.first + lane] = h2f((uint16_t)(word & 0xFFFFu));
        if (q.depth && active) q.depth[ch.first + lane] = depth;
        if (q.local) store_triples(q.local + ch.first * 3, ch.count, tr, x);
        if (COEFFS && q.coeffs) {
            float* const dst = q.coeffs + ch.first * (int64_t)(p.data_dim - 1);
            if (q.coeffs_vec4) store_records<4>(p, leaf, ch.count, dst);  // (launch-uniform)
            else store_records<1>(p, leaf, ch.count, dst);
        }
        if constexpr (COL != kNoColour) {
            float dir[3] = {q.dir[0], q.dir[1], q.dir[2]};
            if (SRC == kPointsArray) load_triples(q.dirs + ch.first * 3, ch.count, tr, dir);
            float rgb[3] = {0.f, 0.f, 0.f};
            if (active) colour_of<COL>(p, leaf, dir, rgb);
            store_triples(q.rgb + ch.first * 3, ch.count, tr, rgb);
        }
    }
}

template <int SRC, int LOOKUP, bool COEFFS, int COL>
void enqueue(const KParams& p, const QueryArgs& q, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((query_kernel<SRC, LOOKUP, COEFFS, COL>), dim3(blocks), dim3(kWave), 0, s, p, q);
}

template <int SRC>
void enqueue_source(const KParams& p, const QueryArgs& q, unsigned blocks, hipStream_t s) {
    if (q.rgb) {  // (+ the record when it is wanted as well)
        switch (basis_flavour(p.format, p.basis_dim)) {
            case BASIS_RGBA: enqueue<SRC, kLookupAny, true, BASIS_RGBA>(p, q, blocks, s); break;
            case BASIS_25: enqueue<SRC, kLookupAny, true, BASIS_25>(p, q, blocks, s); break;
            case BASIS_16: enqueue<SRC, kLookupAny, true, BASIS_16>(p, q, blocks, s); break;
            case BASIS_9: enqueue<SRC, kLookupAny, true, BASIS_9>(p, q, blocks, s); break;
            case BASIS_4: enqueue<SRC, kLookupAny, true, BASIS_4>(p, q, blocks, s); break;
            default: enqueue<SRC, kLookupAny, true, BASIS_1>(p, q, blocks, s); break;
        }
        return;
    }
    const bool n2 = uses_lookup(p);
    if (q.coeffs) {
        if (n2) enqueue<SRC, kLookupN2, true, kNoColour>(p, q, blocks, s);
        else enqueue<SRC, kLookupDescent, true, kNoColour>(p, q, blocks, s);
    } else {
        if (n2) enqueue<SRC, kLookupN2, false, kNoColour>(p, q, blocks, s);
        else enqueue<SRC, kLookupDescent, false, kNoColour>(p, q, blocks, s);
    }
}

}  // namespace

hipError_t launch_query(const KParams& p, const QueryArgs& q, int source, int n_cus, hipStream_t stream) {
    if (q.n_chunks <= 0) return hipSuccess;
    // enough one-wave blocks to fill every SIMD several times over (the lookups are latency-bound),
    // few enough that each keeps a run of consecutive chunks
    const int64_t cap = (int64_t)(n_cus > 0 ? n_cus : 256) * 64;
    const unsigned blocks = (unsigned)(q.n_chunks < cap ? q.n_chunks : cap);
    if (source == kPointsGrid) enqueue_source<kPointsGrid>(p, q, blocks, stream);
    else enqueue_source<kPointsArray>(p, q, blocks, stream);
    return hipGetLastError();
}

}  // namespace vr
