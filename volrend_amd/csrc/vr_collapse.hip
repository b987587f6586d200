// vr_collapse.hip -- vr_collapse_plan / vr_collapse_apply: a tree restated with selected frontier nodes merged into
// their parent slots and the node array compacted, as arrays in the FILE's layout.  Plan: the collapse words and the
// popcounts of the keep words (one kernel), an exclusive scan of the counts (rocPRIM, header-only).  Apply: the new
// child array and the maps (one kernel over the old slots), and per companion array one gather of the kept nodes
// and, for ZERO / MEAN, one kernel over the merged slots behind it.  No LDS, no scratch, no atomics; 64-bit element
// indices throughout; every kernel strides over its work, so no size overflows a grid.
#include <rocprim/device/device_scan.hpp>

#include "vr_collapse.h"

namespace vr {

namespace {

constexpr int kCollapseBlock = 256;             // threads per workgroup of all kernels
constexpr int kCollapseWaves = kCollapseBlock / 64;
constexpr int64_t kCollapseMaxBlocks = 1 << 20;  // the kernels stride beyond that

inline unsigned collapse_blocks(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b < kCollapseMaxBlocks ? b : kCollapseMaxBlocks);
}

// The bits of word w whose node exists (w < words, so at least one does).
__device__ __forceinline__ uint32_t valid_bits(int64_t capacity, int64_t w) {
    const int64_t left = capacity - w * 32;
    return left >= 32 ? ~0u : (1u << left) - 1u;
}

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// The new index of a KEPT node n whose collapse word is cw.  Unsigned, and compared so: whatever a workspace that is
// not the plan's holds, an index is either below n_keep or refused.
__device__ __forceinline__ unsigned long long new_index(const CollapseArgs& a, int64_t n, uint32_t cw) {
    return a.first[n >> 5] + (unsigned long long)__popc(~cw & ((1u << (uint32_t)(n & 31)) - 1u));
}

// One wave per word of 32 nodes: their 32 * N3 child words are consecutive and the lanes run across them.  Words
// without a selected node are not read.  N = 2: a load covers eight nodes and a ballot says which of them have a
// link; otherwise every lane collects the nodes of its elements in a mask and the wave ORs the masks.
// col[w] = sel AND frontier (bit 0 of word 0 and the tail cleared), count[w] = the number of kept nodes of the word,
// count[words] = 0.
__global__ __launch_bounds__(kCollapseBlock) void collapse_mask_kernel(const CollapseArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t stride = (int64_t)gridDim.x * kCollapseWaves;
    for (int64_t w = (int64_t)blockIdx.x * kCollapseWaves + (threadIdx.x >> 6); w <= a.words; w += stride) {
        if (w == a.words) {
            if (lane == 0) a.count[w] = 0;
            break;
        }
        const uint32_t valid = valid_bits(a.capacity, w);
        uint32_t want = __builtin_amdgcn_readfirstlane(a.sel[w]) & valid;
        if (w == 0) want &= ~1u;
        uint32_t inner = 0;  // the nodes of the word that have a link
        if (want) {
            const int64_t base = w * 32 * a.N3;
            const int64_t left = a.n_slots - base;
            const uint32_t count = (uint32_t)(left < 32 * (int64_t)a.N3 ? left : 32 * (int64_t)a.N3);
            if (a.N3 == 8) {
                for (uint32_t t = 0; t < 4; ++t) {
                    const uint32_t e = t * 64 + lane;
                    const int32_t c = e < count ? a.child[base + e] : 0;
                    const unsigned long long linked = __ballot(c != 0);
                    for (uint32_t k = 0; k < 8; ++k)
                        if ((linked >> (8 * k)) & 0xFFull) inner |= 1u << (8 * t + k);
                }
            } else {
                uint32_t mine = 0;
                for (uint32_t e = lane; e < count; e += 64)
                    if (a.child[base + e] != 0) mine |= 1u << (e / (uint32_t)a.N3);
                for (int d = 32; d; d >>= 1) mine |= (uint32_t)__shfl_xor((int)mine, d);
                inner = __builtin_amdgcn_readfirstlane(mine);
            }
        }
        const uint32_t col = want & ~inner;
        if (lane == 0) {
            a.col[w] = col;
            a.count[w] = (unsigned long long)__popc(~col & valid);
        }
    }
}

// Lanes across the OLD slots.  The first slot of a node writes node_map and src_node; a slot of a kept node of new
// index p writes its word of child_out: 0 for a leaf and for a link to a collapsed node m (then it is the merged slot
// of m and names itself in into_slot[m]: a plain store), the new relative offset otherwise.  A link outside
// [1, capacity) is not followed.  A new index >= n_keep (not the plan's workspace, or not its n_keep) writes nothing.
__global__ __launch_bounds__(kCollapseBlock) void collapse_child_kernel(const CollapseArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kCollapseBlock;
    const bool narrow = a.n_slots <= 0xFFFFFFFFll;
    for (int64_t s = (int64_t)blockIdx.x * kCollapseBlock + threadIdx.x; s < a.n_slots; s += stride) {
        const int64_t n = narrow ? (int64_t)((uint32_t)s / (uint32_t)a.N3) : s / a.N3;
        const int64_t j = s - n * a.N3;
        const uint32_t cw = a.col[n >> 5];
        if ((cw >> (uint32_t)(n & 31)) & 1u) {
            if (j == 0 && a.node_map) a.node_map[n] = -1;
            continue;
        }
        const unsigned long long rank = new_index(a, n, cw);
        if (rank >= (unsigned long long)a.n_keep) continue;
        const int64_t p = (int64_t)rank;
        if (j == 0) {
            if (a.node_map) a.node_map[n] = (int32_t)p;
            if (a.src_node) a.src_node[p] = (int32_t)n;
        }
        const int32_t c = a.child[s];
        int32_t out = 0;
        if (c != 0) {
            const int64_t m = n + c;
            if (m >= 1 && m < a.capacity) {
                const uint32_t mw = a.col[m >> 5];
                if ((mw >> (uint32_t)(m & 31)) & 1u) {
                    if (a.into_slot) a.into_slot[m] = (int32_t)(p * a.N3 + j);
                } else {
                    out = (int32_t)((int64_t)new_index(a, m, mw) - p);
                }
            }
        }
        a.child_out[p * a.N3 + j] = out;
    }
}

// `count` consecutive elements, the lanes across them; src, dst and count are wave-uniform.  Where the two addresses
// agree modulo 16 the body moves as 16-byte vectors between a head and a tail of single elements; the two arrays do
// not overlap, so four loads of a lane are in flight before its first store.
template <typename T>
__device__ __forceinline__ void copy_run(const T* __restrict__ src, T* __restrict__ dst, int64_t count, uint32_t lane) {
    constexpr int64_t kPerVec = 16 / sizeof(T);
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src), da = reinterpret_cast<uintptr_t>(dst);
    int64_t head = 0, vecs = 0;
    if (((sa ^ da) & 15u) == 0) {
        head = (int64_t)(((16u - (uint32_t)(sa & 15u)) & 15u) / sizeof(T));
        if (head > count) head = count;
        vecs = (count - head) / kPerVec;
    }
    if ((int64_t)lane < head) dst[lane] = src[lane];  // (head < kPerVec <= 8)
    const uint4* __restrict__ const s4 = reinterpret_cast<const uint4*>(src + head);
    uint4* __restrict__ const d4 = reinterpret_cast<uint4*>(dst + head);
    int64_t i = lane;
    for (; i + 192 < vecs; i += 256) {
        const uint4 v0 = s4[i], v1 = s4[i + 64], v2 = s4[i + 128], v3 = s4[i + 192];
        d4[i] = v0;
        d4[i + 64] = v1;
        d4[i + 128] = v2;
        d4[i + 192] = v3;
    }
    for (; i < vecs; i += 64) d4[i] = s4[i];
    for (int64_t e = head + vecs * kPerVec + lane; e < count; e += 64) dst[e] = src[e];
}

// One wave per word of 32 old nodes: its kept nodes have consecutive new indices (first[w], first[w] + 1, ...), so
// every maximal run of kept nodes of the word is ONE run of consecutive elements in src and in dst -- a word nobody
// collapses in is a single copy of 32 * N3 * dim elements.  The word, the new index and the loop over the runs are
// wave-uniform; nothing is stored at or beyond new node n_keep.
template <typename T>
__global__ __launch_bounds__(kCollapseBlock) void collapse_gather_kernel(const CollapseArgs a, const T* src, T* dst,
                                                                         uint32_t dim) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t stride = (int64_t)gridDim.x * kCollapseWaves;
    const int64_t run = (int64_t)a.N3 * dim;
    for (int64_t w = (int64_t)blockIdx.x * kCollapseWaves + (threadIdx.x >> 6); w < a.words; w += stride) {
        uint32_t keep = ~__builtin_amdgcn_readfirstlane(a.col[w]) & valid_bits(a.capacity, w);
        const unsigned long long n_keep = (unsigned long long)a.n_keep;
        unsigned long long r = uniform64(a.first[w]);
        while (keep && r < n_keep) {
            const uint32_t b = (uint32_t)__ffs(keep) - 1u;
            const uint32_t gaps = ~(keep >> b);  // (b > 0: the bits shifted in are gaps)
            const uint32_t len = gaps ? (uint32_t)__ffs(gaps) - 1u : 32u;
            const int64_t nodes = (int64_t)(n_keep - r < len ? n_keep - r : len);
            copy_run(src + (w * 32 + b) * run, dst + (int64_t)r * run, nodes * run, lane);
            r += len;
            keep = b + len >= 32u ? 0u : keep & ~((1u << (b + len)) - 1u);
        }
    }
}

template <typename T>
__device__ __forceinline__ float element_value(T x);
template <>
__device__ __forceinline__ float element_value<uint16_t>(uint16_t x) { return (float)__builtin_bit_cast(_Float16, x); }
template <>
__device__ __forceinline__ float element_value<uint32_t>(uint32_t x) { return __builtin_bit_cast(float, x); }
// binary32 -> the element, binary16 to nearest even (v_cvt_f16_f32 in the default rounding mode: subnormal halves
// are produced, overflow goes to +-inf), as vr_tree_update_data(VR_DATA_F32) rounds.
template <typename T>
__device__ __forceinline__ T element_bits(float f);
template <>
__device__ __forceinline__ uint16_t element_bits<uint16_t>(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
template <>
__device__ __forceinline__ uint32_t element_bits<uint32_t>(float f) { return __builtin_bit_cast(uint32_t, f); }

// The merged slots of a ZERO / MEAN array, behind its gather.  One wave per collapse word; a collapsed node m with
// into_slot[m] = t >= 0 writes the dim elements of dst slot t, the lanes across them: records of up to 32 elements
// pack 64 / dim nodes into a pass.  MEAN: every lane adds ITS element over the N3 slots of m in ascending order
// (each of the N3 loads reads one child record, coalesced), then divides: no cross-lane step, so the summation order
// is the header's.  A t outside the n_keep * N3 output slots writes nothing.
template <typename T>
__global__ __launch_bounds__(kCollapseBlock) void collapse_merge_kernel(const CollapseArgs a, const T* src, T* dst,
                                                                        uint32_t dim, int mean) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t stride = (int64_t)gridDim.x * kCollapseWaves;
    const bool packed = dim <= 32u;
    const uint32_t per = packed ? 64u / dim : 1u;
    const uint32_t q = packed ? lane / dim : 0u;
    const uint32_t e0 = packed ? lane - q * dim : lane;
    const uint32_t e_step = packed ? dim : 64u;
    const int64_t out_slots = a.n_keep * a.N3;
    const float n3 = (float)a.N3;
    for (int64_t w = (int64_t)blockIdx.x * kCollapseWaves + (threadIdx.x >> 6); w < a.words; w += stride) {
        uint32_t mask = __builtin_amdgcn_readfirstlane(a.col[w]) & valid_bits(a.capacity, w);
        while (mask) {
            uint32_t my = mask;
            for (uint32_t i = 0; i < q && my; ++i) my &= my - 1u;
            if (q < per && my) {
                const int64_t m = w * 32 + (__ffs(my) - 1);
                const int64_t t = a.into_slot[m];
                if (t >= 0 && t < out_slots) {
                    const T* const rec = src + m * a.N3 * dim;
                    T* const out = dst + t * dim;
                    for (uint32_t e = e0; e < dim; e += e_step) {
                        T bits = 0;
                        if (mean) {
                            float sum = element_value<T>(rec[e]);
                            for (int32_t k0 = 1; k0 < a.N3; k0 += 8) {  // eight loads in flight, added in order
                                T v[8];
#pragma unroll
                                for (int32_t i = 0; i < 8; ++i) v[i] = k0 + i < a.N3 ? rec[(int64_t)(k0 + i) * dim + e] : (T)0;
#pragma unroll
                                for (int32_t i = 0; i < 8; ++i)
                                    if (k0 + i < a.N3) sum += element_value<T>(v[i]);
                            }
                            bits = element_bits<T>(sum / n3);
                        }
                        out[e] = bits;
                    }
                }
            }
            for (uint32_t i = 0; i < per && mask; ++i) mask &= mask - 1u;
        }
    }
}

template <typename T>
hipError_t enqueue_array(const CollapseArgs& a, const CollapseArray& arr, hipStream_t s) {
    const dim3 grid(collapse_blocks(a.words, kCollapseWaves)), block(kCollapseBlock);
    hipLaunchKernelGGL((collapse_gather_kernel<T>), grid, block, 0, s, a, static_cast<const T*>(arr.src),
                       static_cast<T*>(arr.dst), (uint32_t)arr.dim);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || arr.rule == VR_COLLAPSE_KEEP || a.n_keep == a.capacity) return e;
    hipLaunchKernelGGL((collapse_merge_kernel<T>), grid, block, 0, s, a, static_cast<const T*>(arr.src),
                       static_cast<T*>(arr.dst), (uint32_t)arr.dim, arr.rule == VR_COLLAPSE_MEAN);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_collapse_plan(const CollapseArgs& a, size_t* scan_need, hipStream_t stream) {
    *scan_need = 0;
    const size_t n = (size_t)a.words + 1;
    const rocprim::plus<unsigned long long> plus;
    hipError_t e = rocprim::exclusive_scan(nullptr, *scan_need, a.count, a.first, 0ull, n, plus, stream);
    if (e != hipSuccess) return e;
    if (*scan_need > a.scan_tmp_bytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(collapse_mask_kernel, dim3(collapse_blocks((int64_t)n, kCollapseWaves)), dim3(kCollapseBlock), 0,
                       stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = a.scan_tmp_bytes;
    return rocprim::exclusive_scan(a.scan_tmp, bytes, a.count, a.first, 0ull, n, plus, stream);
}

hipError_t launch_collapse_apply(const CollapseArgs& a, const CollapseArray* arrays, int n_arrays, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (a.into_slot) e = hipMemsetAsync(a.into_slot, 0xFF, (size_t)a.capacity * 4, stream);  // -1: nobody links to it
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(collapse_child_kernel, dim3(collapse_blocks(a.n_slots, kCollapseBlock)), dim3(kCollapseBlock), 0,
                       stream, a);
    e = hipGetLastError();
    for (int i = 0; i < n_arrays && e == hipSuccess; ++i)
        e = arrays[i].elem_bytes == 2 ? enqueue_array<uint16_t>(a, arrays[i], stream)
                                      : enqueue_array<uint32_t>(a, arrays[i], stream);
    return e;
}

}  // namespace vr
