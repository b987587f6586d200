// vr_geometry.hip -- vr_tree_geometry / vr_slot_points: where a slot is.  Geometry: a fill of the parent array with
// -1, one scatter over the slots (a link names its target's parent slot), and one lane per node walking up its
// parent chain in a loop COUNTED to kGeomMaxDepth -- never a loop on data, so no input keeps a wave running.  Points:
// a streaming kernel, a wave per 64 consecutive (slot, q) outputs, the triples leaving as whole lines through LDS.
// The points are binary64 arithmetic written out operator by operator (include/volrend_hip.h); built with
// -ffp-contract=off.  No scratch; 64-bit element indices; every kernel strides over its work.
#include "vr_geometry.h"

namespace vr {

namespace {

constexpr int kGeomBlock = 256;               // threads per workgroup of the scatter and the walk
constexpr int64_t kGeomMaxBlocks = 1 << 20;   // the kernels stride beyond that
constexpr int kPointsWave = 64;               // the points kernel: one wave per workgroup
constexpr unsigned kPointsMaxBlocks = 256 * 64;

inline unsigned geom_blocks(int64_t items) {
    const int64_t b = (items + kGeomBlock - 1) / kGeomBlock;
    return (unsigned)(b < 1 ? 1 : b < kGeomMaxBlocks ? b : kGeomMaxBlocks);
}

// Lanes across slots: a link child[s] != 0 to a node m in [1, capacity) makes s the parent slot of m.  Links to
// anywhere else are not followed.  (n_slots <= 2^31: s fits the int32 it is stored as.)
__global__ __launch_bounds__(kGeomBlock) void geometry_parent_kernel(const GeometryArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kGeomBlock;
    for (int64_t s = (int64_t)blockIdx.x * kGeomBlock + threadIdx.x; s < a.n_slots; s += stride) {
        const int32_t c = a.child[s];
        if (c == 0) continue;
        const int64_t m = (int64_t)((uint32_t)s / (uint32_t)a.N3) + (int64_t)c;  // (s < 2^31: a 32-bit division)
        if (m >= 1 && m < a.capacity) a.parent[m] = (int32_t)s;
    }
}

// One lane per node.  Every parent[] entry is -1 or a slot index below n_slots that the scatter wrote, so the node
// s / N3 it names is below capacity.  Link i of the chain (i = 0: the link into m itself) has N^i cells of m's level
// per cell of its own: the weights run 1, N, N^2, ... in uint64, wrapping, which leaves the sum exact modulo 2^32.
__global__ __launch_bounds__(kGeomBlock) void geometry_walk_kernel(const GeometryArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kGeomBlock;
    const int32_t N = a.N, NN = a.N * a.N;
    for (int64_t m = (int64_t)blockIdx.x * kGeomBlock + threadIdx.x; m < a.capacity; m += stride) {
        int32_t cur = (int32_t)m, depth = 0;
        unsigned long long ox = 0, oy = 0, oz = 0, w = 1;
        for (int i = 0; i < kGeomMaxDepth; ++i) {
            if (cur == 0) break;
            const int32_t s = a.parent[cur];
            if (s < 0) break;  // (cur != 0 stays: no chain to the root)
            const int32_t node = s / a.N3, j = s - node * a.N3;
            const int32_t ix = j / NN, iy = (j - ix * NN) / N, iz = j - (j / N) * N;
            ox += (unsigned long long)ix * w;
            oy += (unsigned long long)iy * w;
            oz += (unsigned long long)iz * w;
            w *= (unsigned long long)N;
            ++depth;
            cur = node;
        }
        if (cur != 0) depth = -1;
        if (a.node_depth) a.node_depth[m] = depth;
        if (a.node_origin) {
            a.node_origin[m * 3 + 0] = (uint32_t)ox;
            a.node_origin[m * 3 + 1] = (uint32_t)oy;
            a.node_origin[m * 3 + 2] = (uint32_t)oz;
        }
    }
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// binary64 (>= 0, finite) -> binary32 toward zero: the cast rounds to nearest, one step down where that went up.
__device__ __forceinline__ float to_float_rz(double x) {
    const float f = (float)x;
    return (double)f > x ? __uint_as_float(__float_as_uint(f) - 1u) : f;
}

// One wave per block, as query_kernel (vr_query.hip): block b takes the chunks [b * per, (b + 1) * per), a chunk
// being 64 consecutive outputs e = i * k + q.  The triples of a chunk go to LDS one per lane and leave as 3 x 256
// contiguous bytes.  depth[i] and side[i] are written by the lane of q == 0.
__global__ __launch_bounds__(kPointsWave) void slot_points_kernel(const SlotPointsArgs a) {
    __shared__ float tr[3 * kPointsWave];
    const int lane = threadIdx.x;
    const int64_t per = (a.n_chunks + gridDim.x - 1) / gridDim.x;
    int64_t c = per * blockIdx.x, c_end = c + per;
    if (c_end > a.n_chunks) c_end = a.n_chunks;
    const float nan = __uint_as_float(0x7FC00000u);
    const int32_t N = a.N, NN = a.N * a.N;
    for (; c < c_end; ++c) {
        const int64_t first = c << 6;
        const int64_t left = a.total - first;
        const int count = left < kPointsWave ? (int)left : kPointsWave;
        const int64_t i0 = first / a.k;  // wave-uniform: the one 64-bit division of a chunk
        const uint32_t r0 = (uint32_t)(first - i0 * a.k);
        float v[3] = {nan, nan, nan};
        if (lane < count) {
            const uint32_t t = r0 + (uint32_t)lane, ti = t / (uint32_t)a.k;  // (t < k + 64)
            const int64_t i = i0 + ti;
            const uint32_t q = t - ti * (uint32_t)a.k;
            const int32_t s = a.slots[i];
            int32_t d = -1;
            float side = nan;
            if (s >= 0 && (int64_t)s < a.n_slots) {
                const int32_t m = s / a.N3, j = s - m * a.N3;
                const int32_t dm = a.node_depth[m];
                if (dm >= 0 && dm <= kGeomMaxDepth) {
                    d = dm;
                    double D = 1.0;
                    for (int l = 0; l <= dm; ++l) D *= (double)N;  // at most kGeomMaxDepth + 1 steps
                    side = (float)(1.0 / D);
                    const int32_t ix = j / NN, iy = (j - ix * NN) / N, iz = j - (j / N) * N;
                    const int32_t digit[3] = {ix, iy, iz};
                    const uint32_t h0 = mix32(a.seed + 0x9e3779b9u * (uint32_t)s);
                    const uint32_t h1 = mix32(h0 + q);
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const unsigned long long I =
                            (unsigned long long)a.node_origin[(int64_t)m * 3 + ax] * (unsigned long long)N +
                            (unsigned long long)digit[ax];
                        const double u = a.jitter ? (double)(mix32(h1 + (uint32_t)ax) >> 8) * 0x1p-24 : 0.5;
                        v[ax] = to_float_rz(((double)I + u) / D);
                    }
                }
            }
            if (q == 0) {
                if (a.depth) a.depth[i] = d;
                if (a.side) a.side[i] = side;
            }
        }
        if (a.points) {  // (launch-uniform)
            float* const dst = a.points + first * 3;
#pragma unroll
            for (int t = 0; t < 3; ++t) tr[lane * 3 + t] = v[t];
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int f = t * kPointsWave + lane;
                if (f < count * 3) dst[f] = tr[f];
            }
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_tree_geometry(const GeometryArgs& a, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(a.parent, 0xFF, (size_t)a.capacity * sizeof(int32_t), stream);  // every word -1
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(geometry_parent_kernel, dim3(geom_blocks(a.n_slots)), dim3(kGeomBlock), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!a.node_depth && !a.node_origin) return hipSuccess;
    hipLaunchKernelGGL(geometry_walk_kernel, dim3(geom_blocks(a.capacity)), dim3(kGeomBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_slot_points(const SlotPointsArgs& a, hipStream_t stream) {
    const unsigned blocks = (unsigned)(a.n_chunks < (int64_t)kPointsMaxBlocks ? a.n_chunks : (int64_t)kPointsMaxBlocks);
    hipLaunchKernelGGL(slot_points_kernel, dim3(blocks), dim3(kPointsWave), 0, stream, a);
    return hipGetLastError();
}

}  // namespace vr
