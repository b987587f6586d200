"""Helpers of the slot-geometry tests (tests/test_geometry_host.py, tests/test_gpu_geometry.py,
tests/test_gpu_cpp_geometry.py): the numpy restatement of vr_tree_geometry / vr_slot_points as include/volrend_hip.h
states them in plain integers and binary64 operators, an independent top-down walk to hold the restatement against,
the reference's point descent (n3tree_query.hpp:13-48) in numpy float32, and the trees of the tests."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import common
from tests import collapse_util as cu
from tests import refine_util as ru

MAX_DEPTH = 64
CENTER, JITTER = 0, 1


def branching(child) -> int:
    N = round(child.shape[1] ** (1 / 3))
    assert N ** 3 == child.shape[1]
    return N


def digits(j, N):
    """Slot-in-node index j -> (ix, iy, iz)."""
    j = np.asarray(j)
    return np.stack([j // (N * N), j // N % N, j % N], axis=-1)


def restate(child):
    """child int [capacity, N^3] -> (parent_slot int32 [capacity], node_depth int32 [capacity], node_origin uint32
    [capacity, 3]); node_origin is left 0 where node_depth is -1 (unspecified: compare under ``depth >= 0``)."""
    child = np.asarray(child).astype(np.int64)
    cap, N3 = child.shape
    N = branching(child)
    s = np.flatnonzero(child.reshape(-1))
    m = s // N3 + child.reshape(-1)[s]
    ok = (m >= 1) & (m < cap)
    parent = np.full(cap, -1, np.int64)
    parent[m[ok]] = s[ok]
    cur = np.arange(cap)
    depth = np.zeros(cap, np.int64)
    origin = np.zeros((cap, 3), np.uint64)
    w = np.ones(cap, np.uint64)
    for _ in range(MAX_DEPTH):                      # the counted loop
        step = (cur != 0) & (parent[cur] >= 0)
        slot = np.where(step, parent[cur], 0)
        origin += np.where(step[:, None], digits(slot % N3, N).astype(np.uint64) * w[:, None], np.uint64(0))
        w = np.where(step, w * np.uint64(N), w)     # (uint64 arithmetic wraps)
        depth += step
        cur = np.where(step, slot // N3, cur)
    depth[cur != 0] = -1
    origin[cur != 0] = 0
    return parent.astype(np.int32), depth.astype(np.int32), (origin & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def walk_down(child):
    """The independent statement: a top-down descent from node 0 in Python integers -> {node: (parent slot, depth,
    origin modulo 2^32)} of every node it reaches, however deep."""
    child = np.asarray(child)
    cap, N3 = child.shape
    N = branching(child)
    seen = {0: (-1, 0, (0, 0, 0))}
    todo = [0]
    while todo:
        n = todo.pop()
        _, d, o = seen[n]
        for j in np.flatnonzero(child[n]):
            m = n + int(child[n, j])
            if not 1 <= m < cap:
                continue
            assert m not in seen, "not a tree"
            dg = (int(j) // (N * N), int(j) // N % N, int(j) % N)
            seen[m] = (n * N3 + int(j), d + 1, tuple((o[a] * N + dg[a]) % 2 ** 32 for a in range(3)))
            todo.append(m)
    return seen


def _mix(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def points(node_depth, node_origin, N, slots, k=1, mode=CENTER, seed=0):
    """-> (points float32 [n, k, 3], depth int32 [n], side float32 [n]) of vr_slot_points."""
    node_depth, node_origin = np.asarray(node_depth), np.asarray(node_origin).view(np.uint32)
    slots = np.asarray(slots, np.int64)
    cap, N3, n = node_depth.size, N ** 3, slots.size
    ok = (slots >= 0) & (slots < cap * N3)
    s = np.where(ok, slots, 0)
    m, j = s // N3, s % N3
    d = node_depth[m].astype(np.int64)
    ok &= (d >= 0) & (d <= MAX_DEPTH)
    d = np.where(ok, d, 0)
    table = np.cumprod(np.full(MAX_DEPTH + 2, float(N)))      # table[L - 1] = N^L, one binary64 rounding per step
    D = table[d]
    I = node_origin[m].astype(np.uint64) * np.uint64(N) + digits(j, N).astype(np.uint64)          # [n, 3]
    if mode == JITTER:
        with np.errstate(over="ignore"):
            h = _mix(np.uint32(seed) + np.uint32(0x9e3779b9) * s.astype(np.uint32))
            h = _mix(h[:, None] + np.arange(k, dtype=np.uint32)[None, :])
            h = _mix(h[:, :, None] + np.arange(3, dtype=np.uint32)[None, None, :])
        u = (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    else:
        u = np.full((n, k, 3), 0.5)
    x = (I.astype(np.float64)[:, None, :] + u) / D[:, None, None]
    f = x.astype(np.float32)
    up = f.astype(np.float64) > x
    f[up] = np.nextafter(f[up], np.float32(0))                  # toward zero
    f[~ok] = np.nan
    side = (1.0 / D).astype(np.float32)
    side[~ok] = np.nan
    return f, np.where(ok, d, -1).astype(np.int32), side


def descend(child, pts):
    """query_single_from_root in float32, operator by operator -> (slot, depth) of every point [n, 3]."""
    child = np.asarray(child)
    N3, N = child.shape[1], branching(child)
    fN = np.float32(N)
    x = np.maximum(np.minimum(np.asarray(pts, np.float32), np.float32(1.0) - np.float32(1e-6)), np.float32(0)).copy()
    node = np.zeros(x.shape[0], np.int64)
    slot = np.full(x.shape[0], -1, np.int64)
    depth = np.zeros(x.shape[0], np.int64)
    live = np.ones(x.shape[0], bool)
    for level in range(MAX_DEPTH + 2):
        if not live.any():
            break
        x = x * fN
        idx = np.floor(x)
        x = x - idx
        sub = node * N3 + ((idx[:, 0] * fN + idx[:, 1]) * fN + idx[:, 2]).astype(np.int64)
        skip = child.reshape(-1)[np.where(live, sub, 0)]
        done = live & (skip == 0)
        slot[done], depth[done] = sub[done], level
        live &= skip != 0
        node = np.where(live, node + skip, node)
    assert not live.any()
    return slot, depth


# ---- the trees ----
def chain(N, levels, seed=0):
    """child [levels, N^3]: node i links to node i + 1 from a seeded slot -- one node per depth 0..levels - 1."""
    child = np.zeros((levels, N ** 3), np.int32)
    slots = np.random.default_rng(seed).integers(0, N ** 3, levels - 1)
    child[np.arange(levels - 1), slots] = 1
    return child


def random_child(N, seed, depth=3, p_refine=0.3):
    return common.rows_of(common.random_tree_general_n(N=N, depth=depth, seed=seed, p_refine=p_refine)).astype(np.int32)


def refined_collapsed(N=2, seed=4):
    """A random tree after a refine and a collapse (their restatements): appended nodes, then compacted -- the
    numbering is not breadth-first."""
    child = random_child(N, seed, depth=5, p_refine=0.5)
    child = ru.restate(child, ru.selections(child, seed=seed + 100)["random30"])[0]   # (not the tree's own stream)
    sel = cu.selections(child, seed=seed + 101)["random50"]
    return np.asarray(cu.restate(child, sel)["child_out"], np.int32)


def with_orphans(child):
    """Two nodes behind the tree that no slot links to and that link to nothing."""
    return np.concatenate([child, np.zeros((2, child.shape[1]), child.dtype)])


def distinct_records(tree):
    """``tree`` (a SynthTree) with records that identify their slot: seeded values, the slot index s in the first two
    coefficients (s % 2048 and s // 2048, both exact in binary16), a positive sigma; internal slots zero."""
    dd, n_slots = tree.data_dim, tree.child.size
    assert dd >= 3 and n_slots <= 2048 * 2048
    data = (np.random.default_rng(n_slots).standard_normal((n_slots, dd)) * 0.6).astype(np.float16)
    data[:, 0], data[:, 1] = np.arange(n_slots) % 2048, np.arange(n_slots) // 2048
    data[:, -1] = np.abs(data[:, -1]) + np.float16(0.5)
    data[tree.child.reshape(-1) != 0] = 0
    return dataclasses.replace(tree, data=data.reshape(tree.data.shape))


def one_bad_link(child):
    """``child`` with one more link that points outside [1, capacity): never followed."""
    child = child.copy()
    leaf = np.flatnonzero(child.reshape(-1) == 0)[5]
    child.reshape(-1)[leaf] = child.shape[0] + 3
    return child


# name -> child array [capacity, N^3] of every tree the geometry tests run
TREES = {
    "full_n2_73": lambda: ru.full_tree_n2(2),
    "random_n2": lambda: random_child(2, 1, depth=6, p_refine=0.5),
    "random_n3": lambda: random_child(3, 2, depth=3, p_refine=0.45),
    "random_n4": lambda: random_child(4, 3, depth=3, p_refine=0.25),
    "refined_collapsed_n2": refined_collapsed,
    "root_only": lambda: np.zeros((1, 8), np.int32),
    "chain_n2_30": lambda: chain(2, 30, 1),
    "chain_n2_40": lambda: chain(2, 40, 2),          # N^depth > 2^32: the origin modulo 2^32
    "chain_n16_9": lambda: chain(16, 9, 3),          # 16^8 = 2^32
    "chain_n2_70": lambda: chain(2, 70, 4),          # nodes beyond 64 links: depth -1
    "orphans_n2": lambda: with_orphans(random_child(2, 5, depth=5, p_refine=0.5)),
    "bad_link_n2": lambda: one_bad_link(random_child(2, 6, depth=5, p_refine=0.5)),
}
POWER_OF_TWO = ("full_n2_73", "random_n2", "random_n4", "refined_collapsed_n2", "root_only", "orphans_n2")


def reachable_leaves(child, node_depth):
    return np.flatnonzero((child.reshape(-1) == 0) & np.repeat(node_depth >= 0, child.shape[1])).astype(np.int32)
