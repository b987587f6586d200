// vr_update.hip -- gfx950 kernels of vr_tree_update_data / vr_tree_read_data / vr_tree_step: the values of an uploaded tree
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

// Sparse step (vr_tree_step): ONE streaming pass over the bitmap of touched slots, no scratch in global memory, no
// atomics.  A wave takes kWave consecutive words, one per lane, and skips them on an all-zero ballot (the common
// case where rays are few).  Otherwise the lanes write the positions of their set bits, in order, into a per-wave
// LDS table (a prefix sum of the popcounts places them), and the wave walks the table with its lanes ACROSS the
// data_dim elements of a slot: the file-side run is contiguous (SH16: 196 bytes of master, grad and the moments
// each).  Records shorter than half a wave pack kWave / data_dim slots into one instruction, each lane group a run
// of its own (as GradTraits::kPack, vr_dev_backward.h).  A slot costs two dependent trips to memory (its device node, then its node
// word), and the slots of a batch cluster -- a wave may own two thousand of them -- so kStepFlight slots are in
// flight per lane at a time: all their loads are issued before the first value is formed (one slot at a time ran
// at 0.5 TB/s on the bench tree, latency bound).  The wave that owns a word clears it.  The arithmetic is the
// header's, one rounding per operator (-ffp-contract=off, IEEE divide and square root); the tree takes half_bits()
// of the new value as update_values_kernel<true> stores it: coefficients into the padded record of the DEVICE slot
// (the padding is never written), sigma through the leaf-bit rule of put_sigma.
constexpr int kStepWaves = 4;
constexpr int kStepSlots = kWave * 32;  // the slots of a wave's kWave words
constexpr int kStepFlight = 8;          // slots in flight per lane

__global__ __launch_bounds__(kStepWaves * kWave) void step_values_kernel(StepArgs a) {
    __shared__ uint16_t s_list[kStepWaves][kStepSlots];  // positions of the set bits of the wave's words, ascending
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    uint16_t* list = s_list[wave];
    const int dd = a.data_dim;
    const int pack = dd * 2 <= kWave ? kWave / dd : 1;  // slots per wave instruction
    const int chunks = (dd + kWave - 1) / kWave;        // wave instructions per slot
    const int my_sub = pack > 1 ? lane / dd : 0;
    const int my_elem = pack > 1 ? lane - my_sub * dd : lane;
    const uint32_t N3 = (uint32_t)a.N3;
    const bool pow2 = (N3 & (N3 - 1u)) == 0u;
    const int shift = __builtin_ctz(N3);
    const int64_t n_groups = (a.n_words + kWave - 1) / kWave;
    for (int64_t grp = (int64_t)blockIdx.x * kStepWaves + wave; grp < n_groups;
         grp += (int64_t)gridDim.x * kStepWaves) {
        const int64_t wi = grp * kWave + lane;
        const uint32_t word = wi < a.n_words ? a.touched[wi] : 0u;
        if (__builtin_amdgcn_ballot_w64(word != 0u) == 0ull) continue;
        if (word != 0u) a.touched[wi] = 0u;
        // where this lane's bits go: the number of set bits in the lanes below
        const int count = __builtin_popcount(word);
        int below = count;
        for (int d = 1; d < kWave; d <<= 1) {
            const int up = __shfl_up(below, d, kWave);
            if (lane >= d) below += up;
        }
        const int total = __shfl(below, kWave - 1, kWave);
        below -= count;
        for (uint32_t b = word; b != 0u; b &= b - 1u) list[below++] = (uint16_t)(lane * 32 + __builtin_ctz(b));
        // (one wave: its LDS operations execute in order; the compiler must not reorder them)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t base = (uint64_t)grp * kStepSlots;
        for (int ck = 0; ck < chunks; ++ck) {
            const int e = my_elem + ck * kWave;
            const bool lane_on = my_sub < pack && e < dd;
            const bool is_sigma = e == dd - 1;
            const float lr = is_sigma ? a.lr_sigma : a.lr;
            for (int k0 = 0; k0 < total; k0 += kStepFlight * pack) {
                bool on[kStepFlight];
                uint64_t i[kStepFlight], dslot[kStepFlight];
                uint32_t in_node[kStepFlight], old_word[kStepFlight];
                int32_t dnode[kStepFlight];
                float g[kStepFlight], w[kStepFlight], m[kStepFlight], v[kStepFlight];
                // every load of the kStepFlight slots first: the device nodes in front, the node words need them
#pragma unroll
                for (int u = 0; u < kStepFlight; ++u) {
                    const int k = k0 + u * pack + my_sub;
                    on[u] = lane_on && k < total;
                    const uint64_t slot = base + (on[u] ? (uint32_t)list[k] : 0u);
                    on[u] = on[u] && slot < (uint64_t)a.n_slots;  // bits at or beyond capacity * N3 stand for no slot
                    const uint64_t node = pow2 ? slot >> shift : slot / N3;  // the file's node
                    in_node[u] = (uint32_t)(slot - node * N3);
                    i[u] = slot * (uint32_t)dd + (uint32_t)e;
                    dnode[u] = on[u] ? a.node_of_file[node] : 0;
                }
#pragma unroll
                for (int u = 0; u < kStepFlight; ++u) {
                    g[u] = on[u] ? a.grad[i[u]] : 0.f;
                    w[u] = on[u] ? a.master[i[u]] : 0.f;
                    m[u] = on[u] && a.adam ? a.m[i[u]] : 0.f;
                    v[u] = on[u] && a.adam ? a.v[i[u]] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < kStepFlight; ++u) {
                    dslot[u] = (uint64_t)(uint32_t)dnode[u] * N3 + in_node[u];
                    old_word[u] = on[u] && is_sigma ? a.nodes[dslot[u]] : 0u;
                }
#pragma unroll
                for (int u = 0; u < kStepFlight; ++u) {
                    if (!on[u]) continue;
                    float w1;
                    if (a.adam) {
                        const float m1 = a.beta1 * m[u] + a.omb1 * g[u];
                        const float v1 = a.beta2 * v[u] + (a.omb2 * g[u]) * g[u];
                        w1 = w[u] - lr * (m1 / (__builtin_sqrtf(v1) / a.sbc2 + a.eps));
                        a.m[i[u]] = m1;
                        a.v[i[u]] = v1;
                    } else {
                        w1 = w[u] - lr * g[u];
                    }
                    a.master[i[u]] = w1;
                    a.grad[i[u]] = 0.f;
                    const uint32_t h = half_bits(w1);
                    if (is_sigma) {
                        uint32_t nw = old_word[u];
                        put_sigma(&nw, h);  // (an internal slot keeps its word: its sigma is ignored)
                        if (nw != old_word[u]) a.nodes[dslot[u]] = nw;
                    } else {
                        a.leaves[dslot[u] * (uint32_t)a.stride_h + (uint32_t)e] = (uint16_t)h;
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
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

hipError_t launch_step_values(const StepArgs& a, int n_cus, hipStream_t stream) {
    const int64_t n_groups = (a.n_words + kWave - 1) / kWave;
    const dim3 grid(stream_grid((n_groups + kStepWaves - 1) / kStepWaves, n_cus)), block(kStepWaves * kWave);
    hipLaunchKernelGGL(step_values_kernel, grid, block, 0, stream, a);
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
