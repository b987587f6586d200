// vr_update.hip -- gfx950 kernels of vr_tree_update_data / vr_tree_read_data: the values of an uploaded tree
// moved between the file's array (node numbering and record [R.., G.., B.., sigma] of VrTreeDesc.data) and
// the device layout (vr_dev_layout.h), in either direction, and the refresh of the sigma fields of the
// lookup structure.  The topology is never touched: which slot is a leaf is read from the node words.
#include "vr_internal.h"
#include "vr_dev_layout.h"

namespace vr {

namespace {

// Values pass.  A unit of work is a DEVICE node m: on the file side the contiguous run of N3 * data_dim
// elements at node file_node[m], on the device side the N3 * stride bytes of leaves[] and the N3 words of
// nodes[] at m.  Both sides move as whole 16-byte pieces; LDS in between turns [data_dim] records into
// padded records (and back).  One wave per node, kValueWaves nodes per workgroup pass.
constexpr int kValueWaves = 4;
constexpr int kRunHalfs = 1024;  // LDS halfs per wave: the longest run the staged kernels take (N = 2: data_dim <= 128)

// binary32 -> binary16, to nearest even (v_cvt_f16_f32 in the default rounding mode: subnormal halves are
// produced, overflow gives +-inf, the sign of zero is kept, NaN stays NaN), and the exact widening
__device__ __forceinline__ uint32_t half_bits(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
__device__ __forceinline__ float half_value(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }

// the word of a leaf slot with its sigma replaced; internal words are left alone
__device__ __forceinline__ void put_sigma(uint32_t* word, uint32_t sigma) {
    const uint32_t w = *word;
    if (w & kLeafBit) *word = (w & 0xFFFF0000u) | sigma;
}
// the sigma a slot holds: internal slots read as +0
__device__ __forceinline__ uint32_t get_sigma(uint32_t w) { return (w & kLeafBit) ? (w & 0xFFFFu) : 0u; }

// Staged forms: the run is a multiple of 8 elements, fits kRunHalfs and the caller's array is 16-byte
// aligned (launch_*_values checks).  The trip count of the node loop is the same for every wave of a
// workgroup, so the barriers are met by all of them.
template <bool F32>
__global__ __launch_bounds__(kValueWaves * kWave) void update_values_kernel(UpdateArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[kValueWaves][kRunHalfs];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    uint16_t* run = lds[wave];
    const int run_halfs = a.N3 * a.data_dim;
    const int chunks = a.stride_h >> 3;  // 16-byte pieces of a padded record
    const int n_chunks = a.N3 * chunks;
    const int n_coeff = a.data_dim - 1;
    for (int64_t first = (int64_t)blockIdx.x * kValueWaves; first < a.capacity;
         first += (int64_t)gridDim.x * kValueWaves) {
        const int64_t m = first + wave;
        const bool active = m < a.capacity;
        if (active) {
            const int64_t src = (int64_t)a.file_node[m] * run_halfs;
            if (F32) {
                const float4* in = reinterpret_cast<const float4*>(static_cast<const float*>(a.data) + src);
                for (int i = lane; i < (run_halfs >> 2); i += kWave) {
                    const float4 v = in[i];
                    reinterpret_cast<uint2*>(run)[i] = make_uint2(half_bits(v.x) | (half_bits(v.y) << 16),
                                                                  half_bits(v.z) | (half_bits(v.w) << 16));
                }
            } else {
                const uint4* in = reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(a.data) + src);
                for (int i = lane; i < (run_halfs >> 3); i += kWave) reinterpret_cast<uint4*>(run)[i] = in[i];
            }
        }
        __syncthreads();
        if (active) {
            uint4* out = reinterpret_cast<uint4*>(a.leaves + m * a.N3 * a.stride_h);
            for (int i = lane; i < n_chunks; i += kWave) {
                const int s = i / chunks, c = i - s * chunks;
                const uint16_t* rec = run + s * a.data_dim;
                uint32_t h[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int e = c * 8 + j;
                    h[j] = e < n_coeff ? (uint32_t)rec[e] : 0u;  // the padding of a record stays zero
                }
                out[i] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
            for (int s = lane; s < a.N3; s += kWave) put_sigma(a.nodes + m * a.N3 + s, run[s * a.data_dim + n_coeff]);
        }
        __syncthreads();
    }
}

template <bool F32>
__global__ __launch_bounds__(kValueWaves * kWave) void read_values_kernel(UpdateArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[kValueWaves][kRunHalfs];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    uint16_t* run = lds[wave];
    const int run_halfs = a.N3 * a.data_dim;
    const int chunks = a.stride_h >> 3;
    const int n_chunks = a.N3 * chunks;
    const int n_coeff = a.data_dim - 1;
    for (int64_t first = (int64_t)blockIdx.x * kValueWaves; first < a.capacity;
         first += (int64_t)gridDim.x * kValueWaves) {
        const int64_t m = first + wave;
        const bool active = m < a.capacity;
        if (active) {
            const uint4* in = reinterpret_cast<const uint4*>(a.leaves + m * a.N3 * a.stride_h);
            for (int i = lane; i < n_chunks; i += kWave) {
                const int s = i / chunks, c = i - s * chunks;
                uint16_t* rec = run + s * a.data_dim;
                const uint4 q = in[i];
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int e = c * 8 + j;
                    if (e < n_coeff) rec[e] = (uint16_t)(w[j >> 1] >> ((j & 1) * 16));
                }
            }
            for (int s = lane; s < a.N3; s += kWave)
                run[s * a.data_dim + n_coeff] = (uint16_t)get_sigma(a.nodes[m * a.N3 + s]);
        }
        __syncthreads();
        if (active) {
            const int64_t dst = (int64_t)a.file_node[m] * run_halfs;
            if (F32) {
                float4* out = reinterpret_cast<float4*>(static_cast<float*>(a.data) + dst);
                for (int i = lane; i < (run_halfs >> 2); i += kWave) {
                    const uint2 h = reinterpret_cast<const uint2*>(run)[i];
                    out[i] = make_float4(half_value(h.x & 0xFFFFu), half_value(h.x >> 16), half_value(h.y & 0xFFFFu),
                                         half_value(h.y >> 16));
                }
            } else {
                uint4* out = reinterpret_cast<uint4*>(static_cast<uint16_t*>(a.data) + dst);
                for (int i = lane; i < (run_halfs >> 3); i += kWave) out[i] = reinterpret_cast<const uint4*>(run)[i];
            }
        }
        __syncthreads();
    }
}

// Generic forms, for runs the staged kernels do not take (N != 2 with an odd data_dim: the run is not a
// whole number of 16-byte pieces; very long records; an array that is not 16-byte aligned): element-wide
// accesses on the file side, no LDS.
template <bool F32>
__device__ __forceinline__ uint32_t load_half(const void* data, int64_t i) {
    return F32 ? half_bits(static_cast<const float*>(data)[i]) : (uint32_t) static_cast<const uint16_t*>(data)[i];
}

// one work item per 16-byte piece of the padded record array; piece 0 of a record also writes the slot's word
template <bool F32>
__global__ void update_values_generic_kernel(UpdateArgs a) {
    const int chunks = a.stride_h >> 3;
    const int n_coeff = a.data_dim - 1;
    const int64_t total = a.capacity * a.N3 * chunks;
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = gid / chunks;
        const int c = (int)(gid - slot * chunks);
        const int64_t m = slot / a.N3;
        const int64_t src = ((int64_t)a.file_node[m] * a.N3 + (slot - m * a.N3)) * a.data_dim;
        uint32_t h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = c * 8 + j;
            h[j] = e < n_coeff ? load_half<F32>(a.data, src + e) : 0u;
        }
        reinterpret_cast<uint4*>(a.leaves + slot * a.stride_h)[c] =
            make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        if (c == 0) put_sigma(a.nodes + slot, load_half<F32>(a.data, src + n_coeff));
    }
}

// one work item per element of the file's array
template <bool F32>
__global__ void read_values_generic_kernel(UpdateArgs a) {
    const int n_coeff = a.data_dim - 1;
    const int64_t total = a.capacity * a.N3 * a.data_dim;
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = gid / a.data_dim;
        const int e = (int)(gid - slot * a.data_dim);
        const int64_t m = slot / a.N3;
        const int64_t dst = ((int64_t)a.file_node[m] * a.N3 + (slot - m * a.N3)) * a.data_dim + e;
        const uint32_t h = e < n_coeff ? (uint32_t)a.leaves[slot * a.stride_h + e] : get_sigma(a.nodes[slot]);
        if (F32) static_cast<float*>(a.data)[dst] = half_value(h);
        else static_cast<uint16_t*>(a.data)[dst] = (uint16_t)h;
    }
}

// Lookup refresh (N == 2 trees with a lookup structure, vr_dev_layout.h): the sigma field of every leaf
// entry, from the node word the entry names.  Nothing else of an entry changes, and entries that name an
// internal node stay as they are.  A brick entry names its slot itself (child `slot` of node root + delta),
// so the entry order of the bricks (x-major or blocked) does not matter here.
__global__ void refresh_top_kernel(const uint32_t* nodes, uint2* top, uint32_t n_cells) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_cells) return;
    const uint2 e = top[cell];
    if (e.x & kLeafBit) top[cell].x = (e.x & 0xFFFF0000u) | (nodes[e.y] & 0xFFFFu);
}

__global__ void refresh_bricks_kernel(const uint32_t* nodes, const int32_t* brick_root, uint32_t* bricks,
                                      uint64_t n_entries, int BL) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_entries) return;
    const uint32_t e = bricks[gid];
    if (!(e & kLeafBit)) return;
    const uint32_t node = (uint32_t)brick_root[gid >> (3 * BL)] + ((e >> 19) & 1023u);
    const uint32_t slot = (e >> 16) & 7u;
    bricks[gid] = (e & 0xFFFF0000u) | (nodes[(uint64_t)node * 8u + slot] & 0xFFFFu);
}

// the staged kernels take this run of this array
bool staged(const UpdateArgs& a) {
    const int64_t run = (int64_t)a.N3 * a.data_dim;
    return run <= kRunHalfs && run % 8 == 0 && reinterpret_cast<uintptr_t>(a.data) % 16 == 0;
}

// memory-bound passes: enough workgroups to fill the chip, the rest by stride
unsigned stream_grid(int64_t blocks, int n_cus) {
    const int64_t cap = (int64_t)n_cus * 16;
    return (unsigned)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

}  // namespace

hipError_t launch_update_values(const UpdateArgs& a, int n_cus, hipStream_t stream) {
    if (staged(a)) {
        const dim3 grid(stream_grid((a.capacity + kValueWaves - 1) / kValueWaves, n_cus)), block(kValueWaves * kWave);
        if (a.f32) hipLaunchKernelGGL(update_values_kernel<true>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(update_values_kernel<false>, grid, block, 0, stream, a);
    } else {
        const int64_t total = a.capacity * a.N3 * (a.stride_h >> 3);
        const dim3 grid(stream_grid((total + 255) / 256, n_cus)), block(256);
        if (a.f32) hipLaunchKernelGGL(update_values_generic_kernel<true>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(update_values_generic_kernel<false>, grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_read_values(const UpdateArgs& a, int n_cus, hipStream_t stream) {
    if (staged(a)) {
        const dim3 grid(stream_grid((a.capacity + kValueWaves - 1) / kValueWaves, n_cus)), block(kValueWaves * kWave);
        if (a.f32) hipLaunchKernelGGL(read_values_kernel<true>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(read_values_kernel<false>, grid, block, 0, stream, a);
    } else {
        const int64_t total = a.capacity * a.N3 * a.data_dim;
        const dim3 grid(stream_grid((total + 255) / 256, n_cus)), block(256);
        if (a.f32) hipLaunchKernelGGL(read_values_generic_kernel<true>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(read_values_generic_kernel<false>, grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_refresh_lookup(const uint32_t* nodes, const int32_t* brick_root, int n_bricks, uint2* top,
                                 uint32_t* bricks, int top_levels, int brick_levels, hipStream_t stream) {
    const uint32_t n_cells = 1u << (3 * top_levels);
    hipLaunchKernelGGL(refresh_top_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, stream, nodes, top, n_cells);
    if (n_bricks > 0 && brick_levels > 0) {
        const uint64_t n = (uint64_t)n_bricks << (3 * brick_levels);
        hipLaunchKernelGGL(refresh_bricks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, nodes,
                           brick_root, bricks, n, brick_levels);
    }
    return hipGetLastError();
}

}  // namespace vr
