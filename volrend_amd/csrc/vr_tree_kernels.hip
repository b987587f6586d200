// vr_tree_kernels.hip -- gfx950 kernels outside a launch: the upload-time re-layout of the reference
// arrays into the device layout (vr_dev_layout.h), the codebook decode, the lookup-structure build,
// the bitmap count of the touch meter, and the tile de-interleave of a gathered frame.  Nothing
// of the render path.
#include "vr_internal.h"
#include "vr_dev_layout.h"

namespace vr {

namespace {

// De-interleave `world` gathered COMPACT buffers into frames.  blockIdx.z = frame of the
// batch; rank r's compact buffer of frame i starts at gathered + r*rank_stride + i*in_stride.
__global__ void assemble_kernel(uint8_t* frame, int64_t pitch, const uint8_t* gathered, int width,
                                int height, int tile_w, int tile_h, int tiles_x, int world,
                                int64_t out_stride, int64_t rank_stride, int64_t in_stride) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= width || y >= height) return;
    frame += (int64_t)blockIdx.z * out_stride;
    gathered += (int64_t)blockIdx.z * in_stride;
    const int tx = x / tile_w, ty = y / tile_h;
    const int tile = ty * tiles_x + tx;
    const int rank = tile % world;
    const int64_t k = tile / world;
    const int lx = x - tx * tile_w, ly = y - ty * tile_h;
    const int64_t src = (k * tile_w * tile_h + (int64_t)ly * tile_w + lx);
    *reinterpret_cast<uint32_t*>(frame + (int64_t)y * pitch + (int64_t)x * 4) =
        reinterpret_cast<const uint32_t*>(gathered + (int64_t)rank * rank_stride)[src];
}

// ---------------------------------------------------------------------------
// Upload-time re-layout (reference layout -> device layout, vr_dev_layout.h)
// ---------------------------------------------------------------------------
__global__ void relayout_nodes_kernel(const int32_t* child, const uint16_t* data,
                                      const int32_t* perm, uint32_t* nodes, int64_t n_slots,
                                      int N3, int data_dim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const int64_t n = i / N3;
    const int s = (int)(i - n * N3);
    const int32_t skip = child[i];
    const int64_t target = n + skip;
    uint32_t w;
    // Links of nodes the root cannot reach are not covered by the host's topology check
    // (file capacity > used nodes): a link that leaves the array becomes a leaf word.
    if (skip == 0 || target <= 0 || target >= n_slots / N3) {
        w = kLeafBit | (uint32_t)data[i * data_dim + (data_dim - 1)];
    } else {
        w = (uint32_t)perm[target];
    }
    nodes[(int64_t)perm[n] * N3 + s] = w;
}

// one thread per 16-byte chunk of the padded record array
__global__ void relayout_leaves_kernel(const uint16_t* data, const int32_t* perm, uint16_t* leaves,
                                       int64_t n_slots, int N3, int data_dim, int stride_h) {
    const int chunks = stride_h / 8;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t slot = gid / chunks;
    if (slot >= n_slots) return;
    const int c = (int)(gid - slot * chunks);
    const uint16_t* src = data + slot * data_dim;
    uint16_t h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = c * 8 + j;
        h[j] = e < data_dim - 1 ? src[e] : (uint16_t)0;
    }
    uint4 q;
    q.x = h[0] | ((uint32_t)h[1] << 16);
    q.y = h[2] | ((uint32_t)h[3] << 16);
    q.z = h[4] | ((uint32_t)h[5] << 16);
    q.w = h[6] | ((uint32_t)h[7] << 16);
    const int64_t n = slot / N3;
    const int64_t dst = (int64_t)perm[n] * N3 + (slot - n * N3);
    reinterpret_cast<uint4*>(leaves + dst * stride_h)[c] = q;
}

// Median-cut codebook decode on the device (reference host loop: src/n3tree.cpp:310-339):
//   data[slot, j + n_ret + c*n_basis] = quant_colors[j, quant_map[j, slot], c]   j < n_quant
//   data[slot, j + c*n_basis]         = data_retained[j, slot, c]                j < n_ret
//   data[slot, data_dim-1]            = sigma[slot]
// One work item per (slot, basis); the basis index is the fast one so that the three
// 2-byte stores of neighbouring lanes land in the same lines.  `data` is zeroed first.
__global__ void decode_quant_kernel(const uint16_t* __restrict__ colors,
                                    const uint16_t* __restrict__ map,
                                    const uint16_t* __restrict__ sigma,
                                    const uint16_t* __restrict__ retained,
                                    uint16_t* __restrict__ data, int64_t n_slots, int n_quant,
                                    int n_ret, int data_dim) {
    const int n_basis = n_quant + n_ret;
    const int64_t total = n_slots * n_basis;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total;
         w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = w / n_basis;
        const int j = (int)(w - slot * n_basis);
        const uint16_t* c;
        if (j < n_ret) {
            c = retained + ((int64_t)j * n_slots + slot) * 3;
        } else {
            const int q = j - n_ret;
            c = colors + ((int64_t)q * 65536 + map[(int64_t)q * n_slots + slot]) * 3;
        }
        uint16_t* o = data + slot * data_dim + j;
        o[0] = c[0];
        o[n_basis] = c[1];
        o[2 * n_basis] = c[2];
        if (j == 0) data[slot * data_dim + data_dim - 1] = sigma[slot];
    }
}

__global__ void popcount_kernel(const uint32_t* words, uint64_t n_words, unsigned long long* out) {
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words;
         i += (uint64_t)gridDim.x * blockDim.x)
        acc += (unsigned long long)__builtin_popcount(words[i]);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

// Lookup structure, part 1: top[cell] for every cell of the 2^G0-per-axis grid (the device layout,
// vr_dev_layout.h).  brick_root[] = indices of the internal nodes of level G0, ascending.
__global__ void build_top_kernel(const uint32_t* nodes, const int32_t* brick_root, int n_bricks,
                                 uint2* top, int G0, uint32_t* error_flag) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= (1u << (3 * G0))) return;
    const uint32_t mask = (1u << G0) - 1u;
    const uint32_t cx = (cell >> (2 * G0)) & mask, cy = (cell >> G0) & mask, cz = cell & mask;
    uint32_t node = 0;
    for (int l = 0; l < G0; ++l) {
        const int sh = G0 - 1 - l;
        const uint32_t slot = (((cx >> sh) & 1u) << 2) | (((cy >> sh) & 1u) << 1) | ((cz >> sh) & 1u);
        const uint32_t w = nodes[(uint64_t)node * 8u + slot];
        if (w & kLeafBit) {
            top[cell] = make_uint2(kLeafBit | ((uint32_t)(l + 1) << 16) | (w & 0xFFFFu),
                                   node * 8u + slot);
            return;
        }
        node = w;
    }
    // internal node of level G0: find its brick
    int lo = 0, hi = n_bricks - 1, found = -1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t r = (uint32_t)brick_root[mid];
        if (r == node) {
            found = mid;
            break;
        }
        if (r < node) lo = mid + 1; else hi = mid - 1;
    }
    if (found < 0) {
        atomicOr(error_flag, 1u);  // host and device disagree on the level-G0 nodes
        found = 0;
    }
    top[cell] = make_uint2((uint32_t)found, node);
}

// Lookup structure, part 2: one thread per brick entry.
__global__ void build_bricks_kernel(const uint32_t* nodes, const int32_t* brick_root, int n_bricks,
                                    uint32_t* bricks, int BL, int blocked, uint32_t* error_flag) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per = 1u << (3 * BL);
    if (gid >= (uint64_t)n_bricks * per) return;
    const uint32_t b = (uint32_t)(gid >> (3 * BL)), e = (uint32_t)gid & (per - 1u);
    const uint32_t mask = (1u << BL) - 1u;
    uint32_t ex = (e >> (2 * BL)) & mask, ey = (e >> BL) & mask, ez = e & mask;
    if (blocked) {  // BL == 3: e = [x2 y2 z2 z1 | x1 x0 y1 y0 z0] (query_n2)
        ex = (((e >> 8) & 1u) << 2) | ((e >> 3) & 3u);
        ey = (((e >> 7) & 1u) << 2) | ((e >> 1) & 3u);
        ez = (((e >> 5) & 3u) << 1) | (e & 1u);
    }
    const uint32_t root = (uint32_t)brick_root[b];
    uint32_t node = root;
    for (int k = 0; k < BL; ++k) {
        const int sh = BL - 1 - k;
        const uint32_t slot = (((ex >> sh) & 1u) << 2) | (((ey >> sh) & 1u) << 1) | ((ez >> sh) & 1u);
        const uint32_t w = nodes[(uint64_t)node * 8u + slot];
        if (w & kLeafBit) {
            const uint32_t delta = node - root;
            if (delta > 1023u) atomicOr(error_flag, 2u);  // numbering contract broken
            bricks[gid] = kLeafBit | ((uint32_t)k << 29) | ((delta & 1023u) << 19) | (slot << 16) |
                          (w & 0xFFFFu);
            return;
        }
        node = w;
    }
    bricks[gid] = node;  // internal node of level G0 + BL
}

// ---------------------------------------------------------------------------
// Occupancy of the block cull (vr_internal.h "Block cull"): bitmap and boundary list, from the node words.
// ---------------------------------------------------------------------------
// sigma of a leaf word as the march reads it: a float compare, so NaN, -0 and negative values do not count
__device__ __forceinline__ bool leaf_occupied(uint32_t w) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu)) > 0.f;
}

// Does the subtree of `node` hold a leaf with sigma > 0?  Depth first with an explicit stack of (node, next
// child); a leaf sits at most 24 levels deep (lookup_applies), deeper is answered "yes".
__device__ bool subtree_occupied(const uint32_t* nodes, uint32_t node) {
    constexpr int kStack = 24;
    uint32_t st_node[kStack];
    uint32_t st_next[kStack];
    int sp = 0;
    st_node[0] = node;
    st_next[0] = 0;
    while (sp >= 0) {
        if (st_next[sp] == 8u) {
            --sp;
            continue;
        }
        const uint32_t w = nodes[(uint64_t)st_node[sp] * 8u + st_next[sp]];
        st_next[sp]++;
        if (w & kLeafBit) {
            if (leaf_occupied(w)) return true;
        } else {
            if (sp + 1 >= kStack) return true;
            ++sp;
            st_node[sp] = w;
            st_next[sp] = 0;
        }
    }
    return false;
}

// One thread per cell of the 2^g-per-axis grid, 32 consecutive cells per bitmap word.  Thread 0 clears the
// length of the list, which occupancy_list_kernel appends to behind this kernel.
__global__ void occupancy_cells_kernel(const uint32_t* nodes, int g, uint32_t* occ) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_cells = 1u << (3 * g);
    if (cell == 0) occ[0] = 0u;
    bool set = false;
    if (cell < n_cells) {
        const uint32_t mask = (1u << g) - 1u;
        const uint32_t cx = (cell >> (2 * g)) & mask, cy = (cell >> g) & mask, cz = cell & mask;
        uint32_t node = 0;
        bool leaf = false;
        for (int l = 0; l < g; ++l) {
            const int sh = g - 1 - l;
            const uint32_t slot = (((cx >> sh) & 1u) << 2) | (((cy >> sh) & 1u) << 1) | ((cz >> sh) & 1u);
            const uint32_t w = nodes[(uint64_t)node * 8u + slot];
            if (w & kLeafBit) {
                leaf = true;
                set = leaf_occupied(w);
                break;
            }
            node = w;
        }
        if (!leaf) set = subtree_occupied(nodes, node);  // an internal node of level g (g = 0: the root)
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(set);
    if ((threadIdx.x & 31u) == 0u && cell < (n_cells > 32u ? n_cells : 32u))
        occ[kOccHeaderWords + (cell >> 5)] = (uint32_t)(m >> (threadIdx.x & 32u));
}

// The set cells with an unset or out-of-grid face neighbour, appended with one atomic per wave.
__global__ void occupancy_list_kernel(int g, uint32_t* occ) {
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_cells = 1u << (3 * g);
    const uint32_t* bits = occ + kOccHeaderWords;
    uint32_t* list = occ + kOccHeaderWords + occ_bitmap_words(g);
    bool keep = false;
    if (cell < n_cells) {
        const int n = 1 << g;
        const int c[3] = {(int)((cell >> (2 * g)) & (uint32_t)(n - 1)), (int)((cell >> g) & (uint32_t)(n - 1)),
                          (int)(cell & (uint32_t)(n - 1))};
        auto is_set = [&](int x, int y, int z) -> bool {
            if (x < 0 || y < 0 || z < 0 || x >= n || y >= n || z >= n) return false;
            const uint32_t i = ((uint32_t)x << (2 * g)) | ((uint32_t)y << g) | (uint32_t)z;
            return (bits[i >> 5] >> (i & 31u)) & 1u;
        };
        if (is_set(c[0], c[1], c[2]))
            keep = !(is_set(c[0] - 1, c[1], c[2]) && is_set(c[0] + 1, c[1], c[2]) && is_set(c[0], c[1] - 1, c[2]) &&
                     is_set(c[0], c[1] + 1, c[2]) && is_set(c[0], c[1], c[2] - 1) && is_set(c[0], c[1], c[2] + 1));
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == (uint32_t)__builtin_ctzll(m)) base = atomicAdd(&occ[0], (uint32_t)__builtin_popcountll(m));
    base = (uint32_t)__builtin_amdgcn_readlane((int)base, __builtin_ctzll(m));
    if (keep)
        list[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = cell;
}

}  // namespace

hipError_t launch_build_occupancy(const uint32_t* nodes, int levels, uint32_t* occ, hipStream_t stream) {
    const uint32_t n_cells = 1u << (3 * levels);
    const dim3 grid((n_cells + 255u) / 256u), block(256);
    hipLaunchKernelGGL(occupancy_cells_kernel, grid, block, 0, stream, nodes, levels, occ);
    hipLaunchKernelGGL(occupancy_list_kernel, grid, block, 0, stream, levels, occ);
    return hipGetLastError();
}

hipError_t launch_assemble(uint8_t* frame, int64_t pitch, const uint8_t* gathered, int width,
                           int height, int tile_w, int tile_h, int world, int n_frames,
                           int64_t out_stride, int64_t rank_stride, int64_t in_stride,
                           hipStream_t stream) {
    const int tiles_x = (width + tile_w - 1) / tile_w;
    const dim3 block(64, 4);
    const dim3 grid((width + 63) / 64, (height + 3) / 4, n_frames);
    hipLaunchKernelGGL(assemble_kernel, grid, block, 0, stream, frame, pitch, gathered, width,
                       height, tile_w, tile_h, tiles_x, world, out_stride, rank_stride, in_stride);
    return hipGetLastError();
}

int leaf_stride_halfs(int data_dim) {
    const int bytes = 2 * (data_dim - 1);
    int stride = 16;
    while (stride < bytes && stride < 128) stride *= 2;  // 16, 32, 64, 128: never straddles a line
    if (stride < bytes) stride = (bytes + 31) / 32 * 32;
    return stride / 2;
}

hipError_t launch_relayout(const int32_t* child, const uint16_t* data, const int32_t* perm,
                           uint32_t* nodes, uint16_t* leaves, int64_t n_slots, int N3,
                           int data_dim, int stride_h, hipStream_t stream) {
    const int tpb = 256;
    hipLaunchKernelGGL(relayout_nodes_kernel, dim3((unsigned)((n_slots + tpb - 1) / tpb)), dim3(tpb),
                       0, stream, child, data, perm, nodes, n_slots, N3, data_dim);
    const int64_t n_chunks = n_slots * (stride_h / 8);
    hipLaunchKernelGGL(relayout_leaves_kernel, dim3((unsigned)((n_chunks + tpb - 1) / tpb)),
                       dim3(tpb), 0, stream, data, perm, leaves, n_slots, N3, data_dim, stride_h);
    return hipGetLastError();
}

hipError_t launch_build_lookup(const uint32_t* nodes, const int32_t* brick_root, int n_bricks,
                               uint2* top, uint32_t* bricks, int top_levels, int brick_levels,
                               int brick_blocked, uint32_t* error_flag, hipStream_t stream) {
    const uint32_t n_cells = 1u << (3 * top_levels);
    hipLaunchKernelGGL(build_top_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, stream, nodes,
                       brick_root, n_bricks, top, top_levels, error_flag);
    if (n_bricks > 0 && brick_levels > 0) {
        const uint64_t n = (uint64_t)n_bricks << (3 * brick_levels);
        hipLaunchKernelGGL(build_bricks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                           stream, nodes, brick_root, n_bricks, bricks, brick_levels,
                           (brick_blocked && brick_levels == 3) ? 1 : 0, error_flag);
    }
    return hipGetLastError();
}

hipError_t launch_popcount(const uint32_t* words, uint64_t n_words, unsigned long long* out,
                           hipStream_t stream) {
    if (n_words == 0) return hipSuccess;
    uint64_t blocks = (n_words + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(popcount_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, words, n_words,
                       out);
    return hipGetLastError();
}

hipError_t launch_decode_quant(const uint16_t* colors, const uint16_t* map, const uint16_t* sigma,
                               const uint16_t* retained, uint16_t* data, int64_t n_slots,
                               int n_quant, int n_ret, int data_dim, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(data, 0, (size_t)n_slots * data_dim * sizeof(uint16_t), stream);
    if (e != hipSuccess) return e;
    const int64_t total = n_slots * (int64_t)(n_quant + n_ret);
    const int tpb = 256;
    int64_t blocks = (total + tpb - 1) / tpb;
    if (blocks > (1 << 20)) blocks = 1 << 20;  // grid-stride beyond that
    hipLaunchKernelGGL(decode_quant_kernel, dim3((unsigned)blocks), dim3(tpb), 0, stream, colors,
                       map, sigma, retained, data, n_slots, n_quant, n_ret, data_dim);
    return hipGetLastError();
}

}  // namespace vr
