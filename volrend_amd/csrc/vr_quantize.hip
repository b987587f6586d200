// vr_quantize.hip -- vr_quantize: the median cut of include/volrend_hip.h on the device.  Per quantised basis
// function: the three channels of every slot become one packed record of order-preserving 16-bit images; then, level
// by level, per-box extents (integer atomic min over values that can still lower it), the split axis per box, a
// stable radix sort of (box << 16 | image on the axis, slot) from ascending slot order, and the new box of every
// sorted position.  The boxes of a level hold ceil(n/2) and floor(n/2) of their parent's n points and lie in box order
// behind the sort, so the box of a sorted position is a function of the position and the kept count alone: no
// histogram, no scan, and nothing the host has to read.  The box id of a slot lives in its quant_map word throughout.
// Codebook sums are int64 multiples of 2^-24, added in runs of sorted positions.  No scratch, no LDS; 64-bit element
// indices; every kernel strides over its work.  Every store is a plain vector store.
#include <rocprim/device/device_radix_sort.hpp>

#include "vr_quantize.h"

namespace vr {

namespace {

constexpr int kQBlock = 256;
constexpr int64_t kQMaxBlocks = 1 << 16;
constexpr int kQRun = 8;  // sorted positions per lane of the codebook pass

inline unsigned q_blocks(int64_t items) {
    const int64_t b = (items + kQBlock - 1) / kQBlock;
    return (unsigned)(b < 1 ? 1 : b < kQMaxBlocks ? b : kQMaxBlocks);
}

// binary16 bits -> the unsigned image whose order is the sign-magnitude order of the bits (-0 before +0), and back.
__device__ __forceinline__ uint32_t ord16(uint32_t h) { return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u); }
__device__ __forceinline__ uint32_t unord16(uint32_t u) { return (u & 0x8000u) ? (u & 0x7FFFu) : (~u & 0xFFFFu); }

__device__ __forceinline__ float half_bits_to_float(uint32_t h) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

// A finite binary16 as an integer multiple of 2^-24; a non-finite one (outside the contract) counts as 0.
__device__ __forceinline__ long long half_fixed(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    long long v = e == 0 ? (long long)m : e == 31 ? 0ll : (long long)(1024u + m) << (e - 1);
    return (h & 0x8000u) ? -v : v;
}

// The box, at `level` (boxes below 2^level), of sorted position p < n_kept: a box of n points hands its first
// ceil(n/2) to box 2k and the rest to 2k + 1.
__device__ __forceinline__ uint32_t box_of(uint32_t p, int level, uint32_t n_kept) {
    uint32_t lo = 0, n = n_kept, k = 0;
    for (int i = 0; i < level; ++i) {
        const uint32_t h = (n + 1) >> 1;
        if (p < lo + h) { k = 2 * k; n = h; }
        else { k = 2 * k + 1; lo += h; n -= h; }
    }
    return k;
}

// The number of points of box k at `level`.
__device__ __forceinline__ uint32_t box_count(uint32_t k, int level, uint32_t n_kept) {
    uint32_t n = n_kept;
    for (int i = level - 1; i >= 0; --i) {
        const uint32_t h = (n + 1) >> 1;
        n = ((k >> i) & 1u) ? n - h : h;
    }
    return n;
}

__device__ __forceinline__ bool slot_kept(const QuantizeArgs& a, int64_t s, uint32_t& sig) {
    sig = a.data[s * a.data_dim + (a.data_dim - 1)];
    return half_bits_to_float(sig) > a.sigma_thresh;  // (false for a NaN sigma)
}

// Once per call: sigma, data_retained, and the kept count.
__global__ __launch_bounds__(kQBlock) void quant_kept_kernel(const QuantizeArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kQBlock;
    uint32_t mine = 0;
    for (int64_t s = (int64_t)blockIdx.x * kQBlock + threadIdx.x; s < a.n_slots; s += stride) {
        uint32_t sig;
        const bool kept = slot_kept(a, s, sig);
        a.sigma[s] = kept ? (uint16_t)sig : (uint16_t)0;
        for (int r = 0; r < a.n_retained; ++r)
            for (int c = 0; c < 3; ++c)
                a.data_retained[((int64_t)r * a.n_slots + s) * 3 + c] =
                    kept ? a.data[s * a.data_dim + r + c * a.n_basis] : (uint16_t)0;
        mine += kept ? 1u : 0u;
    }
    // (a wave's count in one atomic: integer adds, so the order does not matter)
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(a.n_kept, mine);
}

// Per basis function b: the packed record of every slot.
__global__ __launch_bounds__(kQBlock) void quant_extract_kernel(const QuantizeArgs a, const int b) {
    const int64_t stride = (int64_t)gridDim.x * kQBlock;
    for (int64_t s = (int64_t)blockIdx.x * kQBlock + threadIdx.x; s < a.n_slots; s += stride) {
        uint32_t sig;
        const bool kept = slot_kept(a, s, sig);
        const uint16_t* row = a.data + s * a.data_dim + b;
        const uint32_t r = ord16(row[0]), g = ord16(row[a.n_basis]), bl = ord16(row[2 * a.n_basis]);
        a.pts[s] = make_uint2(r | (g << 16), bl | (kept ? 0x10000u : 0u));
    }
}

// The extents of the boxes of a level.  boxes[] was filled with 0xFF: word c holds the least image on axis c, word
// 3 + c the least 0xFFFF - image.  A lane first looks at the word and only sends the atomic that can lower it (a
// stale look only sends one that was not needed).
__global__ __launch_bounds__(kQBlock) void quant_extent_kernel(const QuantizeArgs a, const uint16_t* map) {
    const int64_t stride = (int64_t)gridDim.x * kQBlock;
    for (int64_t s = (int64_t)blockIdx.x * kQBlock + threadIdx.x; s < a.n_slots; s += stride) {
        const uint2 p = a.pts[s];
        if (!(p.y & 0x10000u)) continue;
        const uint32_t k = map[s] & (uint32_t)(kQuantMaxSortBoxes - 1);
        uint32_t* w = a.boxes + (size_t)k * kQuantBoxWords;
        const uint32_t v[3] = {p.x & 0xFFFFu, p.x >> 16, p.y & 0xFFFFu};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (v[c] < __builtin_nontemporal_load(w + c)) atomicMin(w + c, v[c]);
            if (0xFFFFu - v[c] < __builtin_nontemporal_load(w + 3 + c)) atomicMin(w + 3 + c, 0xFFFFu - v[c]);
        }
    }
}

// The split axis of every box of a level: the largest max - min in binary64, ties to the lowest axis.
__global__ __launch_bounds__(kQBlock) void quant_axis_kernel(const QuantizeArgs a, const int n_boxes) {
    const int k = blockIdx.x * kQBlock + threadIdx.x;
    if (k >= n_boxes) return;
    const uint32_t* w = a.boxes + (size_t)k * kQuantBoxWords;
    double range[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t lo = w[c] & 0xFFFFu, hi = 0xFFFFu - (w[3 + c] & 0xFFFFu);
        range[c] = (double)half_bits_to_float(unord16(hi)) - (double)half_bits_to_float(unord16(lo));
    }
    int best = 0;
    if (range[1] > range[0]) best = 1;
    if (range[2] > range[best]) best = 2;
    a.axis[k] = (uint32_t)best;
}

// The sort's input of a level, in ascending slot order: the key of a kept slot is box << 16 | image on its box's
// axis, below 2^(16 + level); every other slot gets 2^(16 + level) and sorts behind them.
__global__ __launch_bounds__(kQBlock) void quant_key_kernel(const QuantizeArgs a, const uint16_t* map, const int level) {
    const int64_t stride = (int64_t)gridDim.x * kQBlock;
    for (int64_t s = (int64_t)blockIdx.x * kQBlock + threadIdx.x; s < a.n_slots; s += stride) {
        const uint2 p = a.pts[s];
        uint32_t key = 1u << (16 + level);
        if (p.y & 0x10000u) {
            const uint32_t k = map[s] & (uint32_t)(kQuantMaxSortBoxes - 1);
            const uint32_t ax = a.axis[k];
            const uint32_t v = ax == 0 ? (p.x & 0xFFFFu) : ax == 1 ? (p.x >> 16) : (p.y & 0xFFFFu);
            key = (k << 16) | v;
        }
        a.key[0][s] = key;
        a.idx[0][s] = (uint32_t)s;
    }
}

// Behind the sort of level `level`: sorted position p < n_kept is in box box_of(p, level + 1).
__global__ __launch_bounds__(kQBlock) void quant_assign_kernel(const QuantizeArgs a, uint16_t* map,
                                                               const uint32_t* sorted, const int level) {
    const uint32_t n_kept = *a.n_kept;
    const int64_t stride = (int64_t)gridDim.x * kQBlock;
    for (int64_t p = (int64_t)blockIdx.x * kQBlock + threadIdx.x; p < (int64_t)n_kept; p += stride) {
        const uint32_t s = sorted[p];
        if ((int64_t)s < a.n_slots) map[s] = (uint16_t)box_of((uint32_t)p, level + 1, n_kept);
    }
}

// Behind the last sort: the codebook sums.  A lane walks kQRun consecutive sorted positions, whose boxes do not
// decrease, and sends one atomic per channel and run of equal boxes.
__global__ __launch_bounds__(kQBlock) void quant_sum_kernel(const QuantizeArgs a, const uint16_t* map,
                                                            const uint32_t* sorted) {
    const uint32_t n_kept = *a.n_kept;
    const int64_t runs = ((int64_t)n_kept + kQRun - 1) / kQRun;
    const int64_t stride = (int64_t)gridDim.x * kQBlock;
    for (int64_t r = (int64_t)blockIdx.x * kQBlock + threadIdx.x; r < runs; r += stride) {
        long long acc[3] = {0, 0, 0};
        uint32_t cur = 0;
        bool any = false;
        for (int i = 0; i < kQRun; ++i) {
            const int64_t p = r * kQRun + i;
            if (p >= (int64_t)n_kept) break;
            const uint32_t s = sorted[p];
            if ((int64_t)s >= a.n_slots) continue;
            const uint32_t k = map[s];
            if (any && k != cur) {
#pragma unroll
                for (int c = 0; c < 3; ++c) atomicAdd((unsigned long long*)(a.sums + (size_t)cur * 3 + c), (unsigned long long)acc[c]);
                acc[0] = acc[1] = acc[2] = 0;
            }
            cur = k;
            any = true;
            const uint2 q = a.pts[s];
            acc[0] += half_fixed(unord16(q.x & 0xFFFFu));
            acc[1] += half_fixed(unord16(q.x >> 16));
            acc[2] += half_fixed(unord16(q.y & 0xFFFFu));
        }
        if (any) {
#pragma unroll
            for (int c = 0; c < 3; ++c) atomicAdd((unsigned long long*)(a.sums + (size_t)cur * 3 + c), (unsigned long long)acc[c]);
        }
    }
}

// All kQuantRows rows of codebook j: sum / count in binary64, times 2^-24, to binary32, to binary16, each to nearest
// even; zero bits for an empty box and for rows at or beyond 2^bits.
__global__ __launch_bounds__(kQBlock) void quant_codebook_kernel(const QuantizeArgs a, const int j) {
    const int k = blockIdx.x * kQBlock + threadIdx.x;
    if (k >= kQuantRows) return;
    const uint32_t n_kept = *a.n_kept;
    const uint32_t cnt = k < (1 << a.bits) ? box_count((uint32_t)k, a.bits, n_kept) : 0u;
    uint16_t* row = a.quant_colors + ((size_t)j * kQuantRows + k) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint16_t bits = 0;
        if (cnt) {
            const double mean = ((double)a.sums[(size_t)k * 3 + c] / (double)cnt) * 0x1p-24;
            bits = __builtin_bit_cast(unsigned short, (_Float16)(float)mean);
        }
        row[c] = bits;
    }
}

}  // namespace

hipError_t launch_quantize(const QuantizeArgs& a, size_t* sort_need, hipStream_t stream) {
    const unsigned n = (unsigned)a.n_slots;  // < 2^31
    *sort_need = 0;
    for (int l = 0; l < a.bits; ++l) {
        rocprim::double_buffer<uint32_t> keys(a.key[0], a.key[1]), idx(a.idx[0], a.idx[1]);
        size_t need = 0;
        const hipError_t e = rocprim::radix_sort_pairs(nullptr, need, keys, idx, n, 0u, (unsigned)(17 + l), stream);
        if (e != hipSuccess) return e;
        if (need > *sort_need) *sort_need = need;
    }
    if (*sort_need > a.sort_tmp_bytes) return hipErrorInvalidValue;

    hipError_t e;
    const unsigned slot_blocks = q_blocks(a.n_slots);
    if ((e = hipMemsetAsync(a.n_kept, 0, sizeof(uint32_t), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.quant_map, 0, (size_t)a.n_quant * (size_t)a.n_slots * sizeof(uint16_t), stream)) !=
        hipSuccess)
        return e;
    hipLaunchKernelGGL(quant_kept_kernel, dim3(slot_blocks), dim3(kQBlock), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (int j = 0; j < a.n_quant; ++j) {
        uint16_t* const map = a.quant_map + (size_t)j * (size_t)a.n_slots;
        if ((e = hipMemsetAsync(a.sums, 0, kQuantSumBytes, stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(quant_extract_kernel, dim3(slot_blocks), dim3(kQBlock), 0, stream, a, a.n_retained + j);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const uint32_t* sorted = nullptr;
        for (int l = 0; l < a.bits; ++l) {
            const int n_boxes = 1 << l;
            if ((e = hipMemsetAsync(a.boxes, 0xFF, (size_t)n_boxes * kQuantBoxWords * 4, stream)) != hipSuccess) return e;
            hipLaunchKernelGGL(quant_extent_kernel, dim3(slot_blocks), dim3(kQBlock), 0, stream, a, map);
            hipLaunchKernelGGL(quant_axis_kernel, dim3((n_boxes + kQBlock - 1) / kQBlock), dim3(kQBlock), 0, stream, a,
                               n_boxes);
            hipLaunchKernelGGL(quant_key_kernel, dim3(slot_blocks), dim3(kQBlock), 0, stream, a, map, l);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            // (stable, from ascending slot order: ties go by slot index)
            rocprim::double_buffer<uint32_t> keys(a.key[0], a.key[1]), idx(a.idx[0], a.idx[1]);
            size_t bytes = a.sort_tmp_bytes;
            if ((e = rocprim::radix_sort_pairs(a.sort_tmp, bytes, keys, idx, n, 0u, (unsigned)(17 + l), stream)) !=
                hipSuccess)
                return e;
            sorted = idx.current();
            hipLaunchKernelGGL(quant_assign_kernel, dim3(slot_blocks), dim3(kQBlock), 0, stream, a, map, sorted, l);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(quant_sum_kernel, dim3(q_blocks((a.n_slots + kQRun - 1) / kQRun)), dim3(kQBlock), 0, stream,
                           a, map, sorted);
        hipLaunchKernelGGL(quant_codebook_kernel, dim3(kQuantRows / kQBlock), dim3(kQBlock), 0, stream, a, j);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vr
