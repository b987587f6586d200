"""Helpers of the collapse tests (tests/test_collapse_host.py, tests/test_gpu_collapse.py,
tests/test_gpu_cpp_collapse.py): the numpy restatement of vr_collapse_plan / vr_collapse_apply as
include/volrend_hip.h states them in plain integers, the node-bitmap packer, seeded selections and companion sets,
the comparison of an array with its restatement, and the guarded device buffer of the GPU tests."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import common

KEEP, ZERO, MEAN = 0, 1, 2
POISON, GUARD = 0xA5, 512


def pack_bits(flags, extra_words=0, junk=0) -> np.ndarray:
    """bool [capacity] over NODES -> uint32 bitmap, bit m & 31 of word m >> 5.  junk: ORed into every bit at or beyond
    capacity (the tail of the last word and ``extra_words`` further words), which the calls must ignore."""
    flags = np.asarray(flags, bool).reshape(-1)
    n = flags.size
    words = (n + 31) // 32
    bits = np.zeros((words + extra_words) * 32, bool)
    bits[:n] = flags
    if junk:
        bits[n:] = True
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)


def frontier(child) -> np.ndarray:
    """bool [capacity]: the nodes all of whose slots are leaves."""
    return ~(np.asarray(child) != 0).any(axis=1)


def _floats(a):
    """An array of 2- or 4-byte elements as binary16 / binary32."""
    return a.view(np.float16 if a.itemsize == 2 else np.float32)


def mean_records(a, nodes, N3):
    """MEAN of the header: the [N3, dim] records of each node of ``nodes`` in ``a`` [n_slots, dim], summed in binary32
    in ascending slot order starting from slot 0, divided by (float)N3, rounded to the element type -> [len, dim] in
    a's dtype."""
    f = _floats(a).reshape(-1, N3, a.shape[1])[nodes].astype(np.float32)
    with np.errstate(all="ignore"):
        total = f[:, 0].copy()
        for k in range(1, N3):
            total = total + f[:, k]
        mean = (total / np.float32(N3)).astype(np.float32)
        return mean.astype(_floats(a).dtype).view(a.dtype)


def restate(child, sel, arrays=()) -> dict:
    """child int32 [capacity, N^3]; sel bool over nodes (at least capacity flags); arrays: (array [capacity * N^3,
    dim] of 2- or 4-byte elements, rule) pairs.  -> dict(n_keep, child_out [n_keep, N^3], node_map [capacity],
    src_node [n_keep], into_slot [capacity] (all int32), collapsed bool [capacity], dsts: list of [n_keep * N^3,
    dim] in each array's dtype)."""
    child = np.asarray(child)
    cap, N3 = child.shape
    col = np.asarray(sel, bool).reshape(-1)[:cap] & frontier(child)
    col[0] = False
    src_node = np.flatnonzero(~col)
    n_keep = src_node.size
    node_map = np.full(cap, -1, np.int64)
    node_map[src_node] = np.arange(n_keep)
    child_out = np.zeros((n_keep, N3), np.int32)
    into_slot = np.full(cap, -1, np.int64)
    n, j = np.nonzero(child)
    m = n + child[n, j].astype(np.int64)
    ok = (m >= 1) & (m < cap) & ~col[n]           # (a link outside [1, capacity) is not followed: the word stays 0)
    n, j, m = n[ok], j[ok], m[ok]
    p = node_map[n]
    gone = col[m]
    child_out[p[~gone], j[~gone]] = node_map[m[~gone]] - p[~gone]
    into_slot[m[gone]] = p[gone] * N3 + j[gone]
    merged = np.flatnonzero(into_slot >= 0)
    dsts = []
    for a, rule in arrays:
        a = np.asarray(a)
        dst = a.reshape(cap, N3, a.shape[1])[src_node].reshape(n_keep * N3, a.shape[1]).copy()
        if rule == ZERO:
            dst[into_slot[merged]] = 0
        elif rule == MEAN:
            dst[into_slot[merged]] = mean_records(a, merged, N3)
        dsts.append(dst)
    return dict(n_keep=n_keep, child_out=child_out, node_map=node_map.astype(np.int32),
                src_node=src_node.astype(np.int32), into_slot=into_slot.astype(np.int32), collapsed=col, dsts=dsts)


def collapsed_synth(tree, sel, rule=MEAN, data=None):
    """The SynthTree with the selected frontier nodes of ``tree`` collapsed, its values (``data``: the tree's own)
    under ``rule`` -> (tree, the restatement)."""
    N, dd = tree.N, tree.data_dim
    data = np.ascontiguousarray(tree.data if data is None else data, np.float16).reshape(-1, dd)
    res = restate(common.rows_of(tree), sel, [(data.view(np.uint16), rule)])
    cap = res["n_keep"]
    new = dataclasses.replace(tree, child=res["child_out"].reshape(cap, N, N, N),
                              data=res["dsts"][0].view(np.float16).reshape(cap, N, N, N, dd))
    return new, res


def selections(child, seed=0) -> dict:
    """name -> bool [capacity] over the nodes of a child array [capacity, N^3]."""
    cap = child.shape[0]
    rng = np.random.default_rng(seed)
    root, last = np.zeros(cap, bool), np.zeros(cap, bool)
    root[0], last[-1] = True, True
    return {"empty": np.zeros(cap, bool), "all": np.ones(cap, bool),
            "random50": rng.random(cap) < 0.5,             # (frontier nodes and others alike)
            "non_frontier_only": ~frontier(child), "root_only": root, "last_node": last}


def bit_companions(n_slots, data_dim, seed=0):
    """Arrays of random BITS (NaN patterns included: elements move as bits) for KEEP and ZERO."""
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 1 << 16, (n_slots, data_dim), dtype=np.uint16), KEEP),
            (rng.integers(0, 1 << 32, (n_slots, data_dim), dtype=np.uint32), KEEP),
            (rng.integers(1, 1 << 32, (n_slots, 1), dtype=np.uint32), ZERO),
            (rng.integers(1, 1 << 16, (n_slots, data_dim), dtype=np.uint16), ZERO)]


def mean_companions(n_slots, data_dim, seed=0):
    """binary16 and binary32 arrays for MEAN: finite values of mixed magnitude (sums that round at every add, binary16
    subnormal means, binary32 sums that overflow), and a sprinkling of +-inf and NaN."""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for dtype, bits, big, tiny in ((np.float16, np.uint16, 6.0e4, 6.0e-8), (np.float32, np.uint32, 3.0e38, 1.0e-44)):
        x = rng.standard_normal((n_slots, data_dim)) * np.exp(rng.uniform(-6, 6, (n_slots, data_dim)))
        kind = rng.random((n_slots, data_dim))
        x = np.where(kind < 0.02, big * np.sign(x), x)
        x = np.where((kind >= 0.02) & (kind < 0.06), tiny * rng.integers(-8, 9, x.shape), x)
        with np.errstate(all="ignore"):
            x = x.astype(dtype)
        x[(kind >= 0.06) & (kind < 0.07)] = np.inf
        x[(kind >= 0.07) & (kind < 0.08)] = -np.inf
        x[(kind >= 0.08) & (kind < 0.09)] = np.nan
        out.append((np.ascontiguousarray(x).view(bits), MEAN))
    return out


def companions(n_slots, data_dim, seed=0):
    """The arrays of one call: the bit sets, then the MEAN sets (six arrays)."""
    return bit_companions(n_slots, data_dim, seed) + mean_companions(n_slots, data_dim, seed)


def assert_array(got, want, rule, into_slot, what=""):
    """``got`` is ``want`` bit for bit; in the merged slots of a MEAN array an expected NaN must meet a NaN (any
    payload)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    diff = got != want
    if rule == MEAN:
        merged = np.zeros(want.shape[0], bool)
        merged[into_slot[into_slot >= 0]] = True
        nan = np.isnan(_floats(want)) & merged[:, None]
        assert np.isnan(_floats(got))[nan].all(), f"{what}: a NaN mean is missing"
        diff &= ~nan
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ (first at {np.argwhere(diff)[0].tolist()})"


class Guarded:
    """A device buffer of exactly ``nbytes`` bytes, poisoned, with a poisoned guard band behind it -- and, with
    ``offset`` (a multiple of the element size), that many poisoned bytes in front of it, so that the buffer does not
    start on a 16-byte boundary."""

    def __init__(self, torch, nbytes, offset=0):
        self.nbytes, self.offset = int(nbytes), int(offset)
        self.raw = torch.full((self.offset + self.nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.raw.data_ptr() + self.offset

    def bits(self, dtype):
        host = self.raw.cpu().numpy()
        assert (host[self.offset + self.nbytes:] == POISON).all(), "a store went beyond the end of an output"
        assert (host[:self.offset] == POISON).all(), "a store went in front of an output"
        return host[self.offset:self.offset + self.nbytes].copy().view(dtype)

    def untouched(self):
        return bool((self.bits(np.uint8) == POISON).all())
