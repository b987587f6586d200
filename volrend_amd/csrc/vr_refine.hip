// vr_refine.hip -- vr_refine_plan / vr_refine_apply: a tree restated with selected leaves subdivided, as arrays in
// the FILE's layout.  Plan: the effective mask words and their popcounts (one kernel), an exclusive scan of the
// counts (rocPRIM, header-only).  Apply: the new child array and src_slot (one kernel), and per companion array one
// device-to-device copy of the old part and one kernel that writes the slots of the new nodes.  No LDS, no scratch;
// 64-bit element indices throughout; every kernel strides over its work, so no size overflows a grid.
#include <rocprim/device/device_scan.hpp>

#include "vr_refine.h"

namespace vr {

namespace {

constexpr int kRefineBlock = 256;             // threads per workgroup of all three kernels
constexpr int kRefineWaves = kRefineBlock / 64;
constexpr int64_t kRefineMaxBlocks = 1 << 20;  // the kernels stride beyond that

inline unsigned refine_blocks(int64_t items, int per_block) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b < kRefineMaxBlocks ? b : kRefineMaxBlocks);
}

// Lanes across words: mask[w] = the bits of sel[w] whose slot exists and is a leaf, count[w] = their number;
// count[words] = 0.  Only the child words of selected slots are read.
__global__ __launch_bounds__(kRefineBlock) void refine_mask_kernel(const RefineArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kRefineBlock;
    for (int64_t w = (int64_t)blockIdx.x * kRefineBlock + threadIdx.x; w <= a.words; w += stride) {
        if (w == a.words) {
            a.count[w] = 0;
            break;
        }
        uint32_t m = a.sel[w];
        const int64_t left = a.n_slots - w * 32;  // >= 1
        if (left < 32) m &= (1u << left) - 1u;
        uint32_t keep = 0;
        for (uint32_t rest = m; rest; rest &= rest - 1u) {
            const int b = __ffs(rest) - 1;
            if (a.child[w * 32 + b] == 0) keep |= 1u << b;
        }
        a.mask[w] = keep;
        a.count[w] = (unsigned long long)__popc(keep);
    }
}

// Lanes across the elements of child_out.  A refined slot s of rank r points at node capacity + r and names itself
// in src_slot[r]; a rank >= n_new (not the plan's workspace, or not its n_new) leaves the slot what it was.
__global__ __launch_bounds__(kRefineBlock) void refine_child_kernel(const RefineArgs a) {
    const int64_t n_out = (a.capacity + a.n_new) * a.N3;
    const int64_t stride = (int64_t)gridDim.x * kRefineBlock;
    for (int64_t s = (int64_t)blockIdx.x * kRefineBlock + threadIdx.x; s < n_out; s += stride) {
        int32_t c = 0;
        if (s < a.n_slots) {
            c = a.child[s];
            const uint32_t m = a.mask[s >> 5];
            const int b = (int)(s & 31);
            if ((m >> b) & 1u) {
                const unsigned long long r = a.first[s >> 5] + (unsigned long long)__popc(m & ((1u << b) - 1u));
                if (r < (unsigned long long)a.n_new) {
                    c = (int32_t)(a.capacity + (int64_t)r - s / a.N3);
                    if (a.src_slot) a.src_slot[r] = (int32_t)s;
                }
            }
        }
        a.child_out[s] = c;
    }
}

// One wave per mask word: the new nodes of its refined slots are consecutive (ranks first[w], first[w] + 1, ...), and
// for each the lanes run across the N3 * dim CONSECUTIVE output elements of the node; element e takes src[s * dim +
// e % dim] (the remainder is stepped, not divided), so every store instruction writes 64 consecutive elements and
// the record being replicated comes from cache.  The word, its rank and the loop over its bits are wave-uniform.
template <typename T>
__global__ __launch_bounds__(kRefineBlock) void refine_expand_kernel(const RefineArgs a, const T* __restrict__ src,
                                                                     T* __restrict__ dst, uint32_t dim, int zero) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t stride = (int64_t)gridDim.x * kRefineWaves;
    const int64_t run = (int64_t)a.N3 * dim;
    const uint32_t lane_rem = lane % dim, step_rem = 64u % dim;
    for (int64_t w = (int64_t)blockIdx.x * kRefineWaves + (threadIdx.x >> 6); w < a.words; w += stride) {
        uint32_t m = __builtin_amdgcn_readfirstlane(a.mask[w]);
        if (!m) continue;
        unsigned long long r = a.first[w];
        for (; m; m &= m - 1u, ++r) {
            const int64_t s = w * 32 + (__ffs(m) - 1);
            if (r >= (unsigned long long)a.n_new || s >= a.n_slots) break;  // never beyond what apply was told
            T* const out = dst + (a.n_slots + (int64_t)r * a.N3) * dim;
            const T* const rec = src + s * dim;
            uint32_t rem = lane_rem;
            for (int64_t e = lane; e < run; e += 64) {
                out[e] = zero ? (T)0 : rec[rem];
                rem += step_rem;
                if (rem >= dim) rem -= dim;
            }
        }
    }
}

template <typename T>
void enqueue_expand(const RefineArgs& a, const RefineArray& arr, hipStream_t s) {
    hipLaunchKernelGGL((refine_expand_kernel<T>), dim3(refine_blocks(a.words, kRefineWaves)), dim3(kRefineBlock), 0, s, a,
                       static_cast<const T*>(arr.src), static_cast<T*>(arr.dst), (uint32_t)arr.dim, arr.zero);
}

}  // namespace

hipError_t launch_refine_plan(const RefineArgs& a, size_t* scan_need, hipStream_t stream) {
    *scan_need = 0;
    const size_t n = (size_t)a.words + 1;
    const rocprim::plus<unsigned long long> plus;
    hipError_t e = rocprim::exclusive_scan(nullptr, *scan_need, a.count, a.first, 0ull, n, plus, stream);
    if (e != hipSuccess) return e;
    if (*scan_need > a.scan_tmp_bytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refine_mask_kernel, dim3(refine_blocks((int64_t)n, kRefineBlock)), dim3(kRefineBlock), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = a.scan_tmp_bytes;
    return rocprim::exclusive_scan(a.scan_tmp, bytes, a.count, a.first, 0ull, n, plus, stream);
}

hipError_t launch_refine_apply(const RefineArgs& a, const RefineArray* arrays, int n_arrays, hipStream_t stream) {
    const int64_t n_out = (a.capacity + a.n_new) * a.N3;
    hipLaunchKernelGGL(refine_child_kernel, dim3(refine_blocks(n_out, kRefineBlock)), dim3(kRefineBlock), 0, stream, a);
    hipError_t e = hipGetLastError();
    for (int i = 0; i < n_arrays && e == hipSuccess; ++i) {
        const RefineArray& arr = arrays[i];
        e = hipMemcpyAsync(arr.dst, arr.src, (size_t)a.n_slots * (size_t)arr.dim * (size_t)arr.elem_bytes,
                           hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess || a.n_new == 0) continue;
        if (arr.elem_bytes == 2) enqueue_expand<uint16_t>(a, arr, stream);
        else enqueue_expand<uint32_t>(a, arr, stream);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace vr
