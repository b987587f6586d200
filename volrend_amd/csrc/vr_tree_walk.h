// vr_tree_walk.h -- what an upload works out on the host from the child array alone: the topology
// check, the new node numbering, the shape of the lookup structure.  Standard C++ only (no HIP header,
// no vr_host.h): tests/cpp/walk_check.cpp builds vr_tree_walk.cpp with a plain host compiler.
// Errors leave through a `why` buffer.  Nothing here is exported from the library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#pragma GCC visibility push(hidden)

// Walks the child links from the root: every link must land on a node that has
// not been reached before (a tree, not a DAG / cycle), inside [1, capacity).
// Returns the deepest node level or -1 (and says `why`).  A malformed file would otherwise make
// the device descent loop forever.
// level[n] = depth of node n (root 0), 255 = not reachable from the root.
int validate_topology(const int32_t* child, int64_t cap, int N3, std::vector<uint8_t>& level,
                      char* why, size_t why_len);

// New node numbering: pre-order depth-first from the root (children in slot order), so a
// subtree is one contiguous run of the arrays.  Exception for the lookup structure (N == 2,
// G0 > 0): behind an internal node of level G0 (a brick root) come first ALL its descendants of
// the next BL - 1 levels, breadth-first (<= 8 + 64 nodes: a brick entry names the parent of its
// leaf as root + delta), and only then the subtrees hanging below level G0 + BL - 1, each
// depth-first.  Unreachable nodes keep their relative order behind the reachable ones.
// brick_roots receives the new indices of the level-G0 internal nodes (ascending).
std::vector<int32_t> node_permutation(const int32_t* child, int64_t cap, int N3, int G0, int BL,
                                      const std::vector<uint8_t>& level,
                                      std::vector<int32_t>& brick_roots);

// The renumbering read the other way: result[new index] = old index.  vr_accumulate_weights reports per
// leaf slot in the file's numbering, so an upload keeps this (unreachable nodes included: perm is a
// permutation of [0, cap)).
std::vector<int32_t> inverse_permutation(const std::vector<int32_t>& perm);

// Which trees take the integer lookup (vr_query_mode_for, include/volrend_hip.h): N == 2, leaves
// within 24 levels (exact integer digits of a binary32 coordinate), node * 8 + slot byte offsets
// that fit 32 bits.  max_depth as validate_topology returns it.
bool lookup_applies(int N, int max_depth, int64_t capacity);

// The shape of the lookup structure (vr_dev_layout.h): a top grid of 2^G0 cells per axis and bricks of
// BL levels below it.  (0, 0): no lookup structure (the tree takes the descent); BL = 0: the top grid
// resolves every leaf.
struct LookupPlan {
    int G0 = 0, BL = 0;
};
// top_levels / brick_levels: the tuning keys (0 = auto / clamped to [1, 4]).  nodes_at_level(l) = how
// many nodes have level l; it is asked once, for the brick roots at level G0.
LookupPlan plan_lookup(int N, int max_depth, int64_t capacity, int top_levels, int brick_levels,
                       const std::function<uint64_t(int)>& nodes_at_level);

#pragma GCC visibility pop
