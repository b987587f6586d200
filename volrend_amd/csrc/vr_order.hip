// vr_order.hip -- vr_order_rays: the order that makes a ray list coherent.  Three steps on one stream: a key per
// ray from the setup the ray-list launches give it (list_ray, vr_dev_rays.h), a stable sort of (key, index) pairs
// (rocPRIM's radix sort, header-only), and one gather pass that writes the order, the sorted keys and the
// reordered arrays.  No march, no launch slot, no scratch of the library's: the caller's workspace holds the
// pairs and the sort's temporary storage (vr_order.h).  Built with -ffp-contract=off; see vr_device_math.h.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "vr_dev_rays.h"
#include "vr_order.h"

namespace vr {

namespace {

// One coordinate of the key: (uint32_t)min(max(v * 2^bits, 0.f), 2^bits - 1), truncating, NaN -> 0.  Written
// with the comparison that a NaN fails (fminf / fmaxf would drop the NaN and keep the OTHER operand, a median
// instruction depends on the mode register).
__device__ __forceinline__ uint32_t order_quant(float v, float scale) {
    const float s = v * scale;
    return s > 0.f ? (uint32_t)vmin(s, scale - 1.f) : 0u;
}

// Bit 6 * b + c of the key = bit b of coordinate c.
__device__ __forceinline__ uint32_t order_morton(const uint32_t* q, int bits) {
    uint32_t key = 0;
    for (int b = 0; b < bits; ++b) {
#pragma unroll
        for (int c = 0; c < 6; ++c) key |= ((q[c] >> b) & 1u) << (6 * b + c);
    }
    return key;
}

// Ray (workgroup, wave, lane) of the list -> key[id], idx[id] = id.  Every lane runs list_ray (its barrier).
template <int FMA, int GW>
__global__ __launch_bounds__(kWave* GW) void order_key_kernel(const KParams p, const RayList rl, const OrderArgs a) {
    using P = Policy<FMA>;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t id;
    Ray ray;
    float vdir[3];
    if (!list_ray<FMA, GW>(p, rl, lane, wave, id, ray, vdir)) return;
    uint32_t key = kOrderMissKey;
    if (ray.entered) {  // (false for every ray of a tree with N <= 0: list_ray leaves the reset ray)
        const float scale = (float)(1 << a.bits);
        uint32_t q[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            q[c] = order_quant(P::madd(ray.t, ray.dir[c], ray.cen[c]), scale);         // entry
            q[3 + c] = order_quant(P::madd(ray.tmax, ray.dir[c], ray.cen[c]), scale);  // exit
        }
        key = order_morton(q, a.bits);
    }
    a.key[0][id] = key;
    a.idx[0][id] = id;
}

// One wave per block and 64 consecutive sorted positions: order, keys, and the rows of origins / dirs / payload
// the positions name.  The reads of a row are a gather (12 .. 32 bytes each); the writes leave as whole lines
// through LDS, as query_kernel writes its triples.  Outputs that are not wanted: launch-uniform NULL tests.
__device__ __forceinline__ void gather_rows(const float* src, float* dst, int dim, uint32_t from, int64_t first,
                                            int count, float* rows) {
    const int lane = threadIdx.x;
    if (lane < count) {
        const float* const s = src + (size_t)from * (size_t)dim;
        for (int c = 0; c < dim; ++c) rows[lane * dim + c] = s[c];
    }
    __syncthreads();
    float* const d = dst + (size_t)first * (size_t)dim;
    for (int f = lane; f < count * dim; f += kWave) d[f] = rows[f];
    __syncthreads();
}

__global__ __launch_bounds__(kWave) void order_gather_kernel(const OrderArgs a, const uint32_t* keys_sorted,
                                                             const uint32_t* idx_sorted, int64_t n) {
    __shared__ float rows[kOrderMaxPayload * kWave];
    const int lane = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * kWave;
    const int64_t left = n - first;
    const int count = left < kWave ? (int)left : kWave;
    uint32_t from = 0;
    if (lane < count) {
        from = idx_sorted[first + lane];
        a.order[first + lane] = from;
        if (a.keys) a.keys[first + lane] = keys_sorted[first + lane];
    }
    if (a.origins_out) gather_rows(a.origins, a.origins_out, 3, from, first, count, rows);
    if (a.dirs_out) gather_rows(a.dirs, a.dirs_out, 3, from, first, count, rows);
    if (a.payload_out) gather_rows(a.payload, a.payload_out, a.payload_dim, from, first, count, rows);
}

template <int FMA>
void enqueue_keys(const KParams& p, const RayList& rl, const OrderArgs& a, hipStream_t s) {
    constexpr int GW = kOrderKeyWaves;
    const unsigned blocks = (unsigned)((rl.n + kWave * GW - 1) / (kWave * GW));
    hipLaunchKernelGGL((order_key_kernel<FMA, GW>), dim3(blocks), dim3(kWave * GW), 0, s, p, rl, a);
}

}  // namespace

hipError_t launch_order(const KParams& p, const RayList& rl, const OrderArgs& a, int fp_mode, size_t* sort_need,
                        hipStream_t stream) {
    *sort_need = 0;
    if (rl.n <= 0) return hipSuccess;
    const unsigned n = (unsigned)rl.n;  // < 2^30
    // (all 32 bits: the miss key has every bit set; radix sorts are stable, which is the tie rule)
    rocprim::double_buffer<uint32_t> keys(a.key[0], a.key[1]), idx(a.idx[0], a.idx[1]);
    hipError_t e = rocprim::radix_sort_pairs(nullptr, *sort_need, keys, idx, n, 0u, 32u, stream);
    if (e != hipSuccess) return e;
    if (*sort_need > a.sort_tmp_bytes) return hipErrorInvalidValue;
    if (fp_mode == VR_FP_FMA) enqueue_keys<1>(p, rl, a, stream);
    else enqueue_keys<0>(p, rl, a, stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = a.sort_tmp_bytes;
    if ((e = rocprim::radix_sort_pairs(a.sort_tmp, bytes, keys, idx, n, 0u, 32u, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(order_gather_kernel, dim3((n + kWave - 1) / kWave), dim3(kWave), 0, stream, a, keys.current(),
                       idx.current(), rl.n);
    return hipGetLastError();
}

}  // namespace vr
