// vr_tree_walk.cpp -- the host walks of an upload (vr_tree_walk.h).  Standard C++ only.
#include "vr_tree_walk.h"

#include <cstdio>

int validate_topology(const int32_t* child, int64_t cap, int N3, std::vector<uint8_t>& level,
                      char* why, size_t why_len) {
    if (cap <= 0) {
        snprintf(why, why_len, "capacity must be positive");
        return -1;
    }
    // The link check of both walks: slot `s` of node `n` (level `ln`) links to node `m`.  A sound link
    // gives `m` its level; anything else says why.
    const auto link = [&](int64_t n, int s, int64_t m, int ln) {
        if (m <= 0 || m >= cap) {
            snprintf(why, why_len, "node %lld slot %d links outside the tree (%lld)", (long long)n, s,
                     (long long)m);
            return false;
        }
        if (level[(size_t)m] != 255) {
            snprintf(why, why_len, "node %lld is linked twice (cycle or DAG)", (long long)m);
            return false;
        }
        if (ln + 1 > 60) {
            snprintf(why, why_len, "tree deeper than 60 levels");
            return false;
        }
        level[(size_t)m] = (uint8_t)(ln + 1);
        return true;
    };
    // Fast path: files written breadth- or depth-first link every child FORWARD (to a higher
    // index), and then one sweep in index order sees every parent before its children -- no
    // queue, sequential reads (a 2 M-node tree: ~20 ms instead of ~50).  The first backward link
    // abandons the sweep for the general walk below.
    {
        level.assign((size_t)cap, 255);
        level[0] = 0;
        int depth = 0;
        bool forward_only = true;
        for (int64_t n = 0; n < cap && forward_only; ++n) {
            const int ln = level[(size_t)n];
            if (ln == 255) continue;  // not reachable (so far: decided for good if all links go forward)
            const int32_t* c = child + n * N3;
            for (int s = 0; s < N3; ++s) {
                if (c[s] == 0) continue;
                const int64_t m = n + c[s];
                if (m <= n) {
                    forward_only = false;
                    break;
                }
                if (!link(n, s, m, ln)) return -1;
                if (ln + 1 > depth) depth = ln + 1;
            }
        }
        if (forward_only) return depth;
    }
    // General walk: level by level from the root, whatever the order of the nodes.
    level.assign((size_t)cap, 255);
    level[0] = 0;
    std::vector<int64_t> cur{0}, next;
    int depth = 0;
    for (;; ++depth) {
        next.clear();
        for (int64_t n : cur) {
            const int32_t* c = child + n * N3;
            for (int s = 0; s < N3; ++s) {
                if (c[s] == 0) continue;
                const int64_t m = n + c[s];
                if (!link(n, s, m, depth)) return -1;
                next.push_back(m);
            }
        }
        if (next.empty()) return depth;
        cur.swap(next);
    }
}

std::vector<int32_t> node_permutation(const int32_t* child, int64_t cap, int N3, int G0, int BL,
                                      const std::vector<uint8_t>& level,
                                      std::vector<int32_t>& brick_roots) {
    std::vector<int32_t> perm((size_t)cap, -1);
    brick_roots.clear();
    int32_t next = 0;
    std::vector<int64_t> stack{0}, ring, ring_next;
    while (!stack.empty()) {
        const int64_t n = stack.back();
        stack.pop_back();
        perm[(size_t)n] = next++;
        const int32_t* c = child + n * N3;
        if (G0 > 0 && level[(size_t)n] == G0) {
            brick_roots.push_back(perm[(size_t)n]);
            // levels G0+1 .. G0+BL-1 breadth-first right behind the root
            ring.assign(1, n);
            for (int k = 1; k < BL; ++k) {
                ring_next.clear();
                for (int64_t m : ring)
                    for (int s = 0; s < N3; ++s)
                        if (child[m * N3 + s] != 0) {
                            const int64_t ch = m + child[m * N3 + s];
                            perm[(size_t)ch] = next++;
                            ring_next.push_back(ch);
                        }
                ring.swap(ring_next);
            }
            // `ring` = the nodes of level G0+BL-1: their children start ordinary subtrees
            for (size_t i = ring.size(); i-- > 0;) {
                const int64_t m = ring[i];
                for (int s = N3 - 1; s >= 0; --s)
                    if (child[m * N3 + s] != 0) stack.push_back(m + child[m * N3 + s]);
            }
            continue;
        }
        for (int s = N3 - 1; s >= 0; --s)  // reversed: slot 0 is visited first
            if (c[s] != 0) stack.push_back(n + c[s]);
    }
    for (int64_t i = 0; i < cap; ++i)
        if (perm[(size_t)i] < 0) perm[(size_t)i] = next++;
    return perm;
}

std::vector<int32_t> inverse_permutation(const std::vector<int32_t>& perm) {
    std::vector<int32_t> inv(perm.size());
    for (size_t i = 0; i < perm.size(); ++i) inv[(size_t)perm[i]] = (int32_t)i;
    return inv;
}

bool lookup_applies(int N, int max_depth, int64_t capacity) {
    return N == 2 && max_depth <= 23 && capacity < (1ll << 27);
}

LookupPlan plan_lookup(int N, int max_depth, int64_t capacity, int top_levels, int brick_levels,
                       const std::function<uint64_t(int)>& nodes_at_level) {
    LookupPlan p;
    if (!lookup_applies(N, max_depth, capacity)) return p;
    // auto: top grid + brick reach the deepest leaf (depth max_depth + 1) without a child-word
    // walk where a top grid of <= 256^3 cells allows it -- 64^3 (2 MB) for lego-class trees of
    // 9 levels, 128^3 for 10 (measured: C1 0.269 ms at (6,3) against 0.301 at (5,3); C3 0.790
    // at (7,3) against 0.847 at (6,3))
    p.G0 = top_levels > 0 ? top_levels : (max_depth + 1 - 3 < 6 ? 6 : max_depth + 1 - 3);
    if (p.G0 > 8) p.G0 = 8;
    if (p.G0 > max_depth + 1) p.G0 = max_depth + 1;  // deepest leaf depth
    p.BL = brick_levels < 1 ? 1 : (brick_levels > 4 ? 4 : brick_levels);
    if (p.BL > max_depth + 1 - p.G0) p.BL = max_depth + 1 - p.G0;  // 0: the top grid resolves every leaf
    // the kernel addresses brick entries with 32-bit byte offsets: keep the brick array < 4 GB
    const uint64_t n_roots = nodes_at_level(p.G0);
    while (p.BL > 1 && ((n_roots << (3 * p.BL)) * sizeof(uint32_t)) >= (1ull << 32)) --p.BL;
    return p;
}
