"""Helpers of the refinement tests (tests/test_refine_host.py, tests/test_gpu_refine.py, tests/test_gpu_cpp_refine.py):
the numpy restatement of vr_refine_plan / vr_refine_apply as include/volrend_hip.h states them in plain integers, the
bitmap packer, and seeded trees and selections."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import common

COPY, ZERO = 0, 1


def pack_bits(flags, extra_words=0, junk=0) -> np.ndarray:
    """bool [n] -> uint32 bitmap, bit s & 31 of word s >> 5.  junk: ORed into every bit at or beyond n (the tail of
    the last word and ``extra_words`` further words), which the calls must ignore."""
    flags = np.asarray(flags, bool).reshape(-1)
    n = flags.size
    words = (n + 31) // 32
    bits = np.zeros((words + extra_words) * 32, bool)
    bits[:n] = flags
    if junk:
        bits[n:] = True
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)


def restate(child, sel, arrays=()):
    """child int32 [capacity, N^3]; sel bool [capacity * N^3]; arrays: (array [capacity * N^3, dim], fill) pairs.
    -> (child_out [capacity + n_new, N^3], src_slot int32 [n_new], list of dst [(capacity + n_new) * N^3, dim])."""
    child = np.asarray(child)
    cap, N3 = child.shape
    src_slot = np.flatnonzero(np.asarray(sel, bool).reshape(-1)[:cap * N3] & (child.reshape(-1) == 0))
    n_new = src_slot.size
    child_out = np.zeros((cap + n_new, N3), np.int32)
    child_out[:cap] = child
    child_out.reshape(-1)[src_slot] = cap + np.arange(n_new) - src_slot // N3
    dsts = []
    for a, fill in arrays:
        new = np.repeat(a[src_slot], N3, axis=0) if fill == COPY else np.zeros((n_new * N3, a.shape[1]), a.dtype)
        dsts.append(np.concatenate([a, new]))
    return child_out, src_slot.astype(np.int32), dsts


def refined_synth(tree, sel):
    """The SynthTree with the selected leaves of ``tree`` subdivided -> (tree, src_slot)."""
    N, dd = tree.N, tree.data_dim
    child_out, src_slot, (data,) = restate(common.rows_of(tree), sel, [(tree.data.reshape(-1, dd), COPY)])
    cap = child_out.shape[0]
    return dataclasses.replace(tree, child=child_out.reshape(cap, N, N, N),
                               data=data.reshape(cap, N, N, N, dd)), src_slot


def full_tree_n2(depth):
    """child [capacity, 8] of the complete N = 2 tree with leaves at ``depth`` (breadth-first numbering)."""
    cap = (8 ** (depth + 1) - 1) // 7
    inner = (8 ** depth - 1) // 7
    child = np.zeros((cap, 8), np.int32)
    node = np.arange(inner)[:, None]
    child[:inner] = 8 * node + 1 + np.arange(8)[None, :] - node
    return child


def selections(child, seed=0) -> dict:
    """name -> bool [capacity * N^3] over a child array [capacity, N^3]."""
    leaf = child.reshape(-1) == 0
    rng = np.random.default_rng(seed)
    last = np.zeros(leaf.size, bool)
    last[-1] = True
    return {"empty": np.zeros(leaf.size, bool), "all_leaves": leaf.copy(),
            "random30": rng.random(leaf.size) < 0.3,      # (leaves and internal slots alike)
            "internal_only": ~leaf, "last_bit": last}


def companions(n_slots, data_dim, seed=0):
    """The arrays of one call: binary16 records COPY, a float32 master COPY, a float32 moment ZERO -- random bits
    (NaN patterns included: elements move as bits)."""
    rng = np.random.default_rng(seed)
    f16 = rng.integers(0, 1 << 16, (n_slots, data_dim), dtype=np.uint16)
    f32 = rng.integers(0, 1 << 32, (n_slots, data_dim), dtype=np.uint32)
    mom = rng.integers(1, 1 << 32, (n_slots, 1), dtype=np.uint32)
    return [(f16, COPY), (f32, COPY), (mom, ZERO)]
