// vr_dev_layout.h -- the device layout of a tree (node words, leaf records, top grid, bricks) and the
// constants both the render path (vr_render.hip) and the upload-time build kernels
// (vr_tree_kernels.hip) read it with.  Device code only.
#pragma once
#include "vr_internal.h"

namespace vr {

namespace {

constexpr int kWave = 64;

// Kernel flavours (the basis flavours BASIS_*: vr_internal.h).  FAST is the production path: N == 2 integer descent, SH/RGBA
// only, no instrumentation, zero scratch.  FULL adds the SG/ASG lobe code and
// the optional access counters (VrFrame.counters); GENERIC additionally swaps in
// the literal float descent for N != 2 (or trees deeper than 24 levels).
enum { MODE_FAST = 0, MODE_FULL = 1, MODE_GENERIC = 2 };

// ---------------------------------------------------------------------------
// Device layout (built once at upload by the kernels of vr_tree_kernels.hip; the
// tree.npz format and the reference's flat child_/data_ arrays are the INPUT):
//
//   Nodes are RENUMBERED depth-first (pre-order) at upload: a subtree is one contiguous
//   run of the arrays, so the rays of a screen tile -- which walk through one compact
//   region of space -- touch few cache lines / DRAM pages (the file's numbering is
//   whatever the exporter produced, typically breadth-first).
//   nodes[capacity*N3]   one 32-bit word per child slot
//        bit31 = 0 : internal -- ABSOLUTE index of the child node (> 0)
//        bit31 = 1 : leaf     -- low 16 bits = sigma as IEEE fp16
//     so the descent's last load already delivers sigma: an empty-space
//     sample never touches the (GB-sized) coefficient array.
//   leaves[capacity*N3*stride] the data_dim-1 colour coefficients of each slot,
//     fp16, zero padded to `stride` bytes (16-byte aligned; 128 B = one cache
//     line for SH16) so a record is read with a few aligned 16-byte loads.
//   Lookup structure (N == 2), built from nodes[] at upload.  A sample resolves its leaf with
//   ONE load when it stays inside the top cell of the previous sample, and without a loop for
//   trees of up to G0 + BL levels (lego-class trees: 9):
//   top[8^G0]  uint2     one entry per cell of the 2^G0-per-axis grid (default G0 = 6: 2 MB)
//        .x bit31 = 1 : the cell lies inside ONE leaf of depth d <= G0 (extent 2^-d):
//                       .x = leaf | d << 16 | sigma(fp16),  .y = leaf id (slot index)
//        .x bit31 = 0 : the cell is an internal node of level G0 with a brick:
//                       .x = brick index,  .y = that node's index
//   bricks[n_bricks * 8^BL]  u32   (default BL = 3: 512 entries = 2 KB per brick) entry per
//        cell of the 2^BL-per-axis subdivision of a top cell:
//        bit31 = 1 : inside one leaf of depth d = G0 + 1 + drel:
//                    leaf | drel << 29 | delta << 19 | slot << 16 | sigma(fp16), where the leaf
//                    is child `slot` of node root + delta (the brick root's descendants of the
//                    next BL - 1 levels are numbered right behind it: delta <= 8 + 64 + 512)
//        bit31 = 0 : an internal node of level G0 + BL: its index; the walk continues there
//                    with one child-word load per level.
//        Entry order inside a brick: x-major (index = x << 2 BL | y << BL | z: a 128-byte line is a
//        1 x 4 x 8 slab of an 8^3 brick), or -- KParams.brick_blocked, BL == 3 only, chosen per tree
//        at upload -- [x2 y2 z2 z1 | x1 x0 y1 y0 z0]: a line is a 4 x 4 x 2 block, which a ray
//        crosses 3.5 instead of 4.8 of per brick.  The blocked order costs six more vector
//        instructions per brick lookup, so it is for trees whose lookups are fabric traffic: C3
//        (286 MB of lookup structure) -15 % L2<->fabric bytes, -3 % frame time; C1 / C2 (92 MB)
//        +1 % / +4 % (profiles/r05_experiments.jsonl, r05d).
// ---------------------------------------------------------------------------
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr int kMaxBrickLevels = 4;   // delta field (10 bits): 8 + 64 + 512 nodes below a brick root

// Distinct-line meter of the instrumented flavours (SURVEY.md 8(d) "B_unique"): marks the 128-byte
// line(s) an access of `bytes` bytes at byte offset `off` of array `which` touches.
enum { TOUCH_LEAVES = 0, TOUCH_NODES = 1, TOUCH_TOP = 2, TOUCH_BRICKS = 3 };
__device__ __forceinline__ void touch(const KParams& p, int which, uint64_t off, uint32_t bytes) {
    uint32_t* bm = p.touch[which];
    if (!bm) return;
    const int sh = which == TOUCH_LEAVES ? kTouchLeafShift : 7;
    const uint64_t l0 = off >> sh, l1 = (off + bytes - 1) >> sh;
    atomicOr(&bm[l0 >> 5], 1u << (l0 & 31u));
    if (l1 != l0) atomicOr(&bm[l1 >> 5], 1u << (l1 & 31u));
}

}  // namespace

}  // namespace vr
