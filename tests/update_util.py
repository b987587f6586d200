"""Helpers of the vr_tree_update_data / vr_tree_read_data tests: the scenes, two data sets per scene that differ in
every value, and what a leaf is to the lookup structure (needs no GPU)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests import common
from tests import grad_util as gu

SIGMA_THRESH = 1e-2   # RenderOptions' default

# Depth-4 SG / ASG scenes at the record lengths where vr_tree_step changes its lane layout (3 * basis_dim + 1 = 22, 31,
# 34, 64, 67: two slots per wave instruction with 20 and with 2 idle lanes, one slot with 30 and with no idle lane,
# two chunks with three lanes in the second).  Their lobe table (tree.extra) is not part of `data`.
SHAPE_SCENES = {"asg7": ("ASG", 7), "sg10": ("SG", 10), "sg11": ("SG", 11), "sg21": ("SG", 21), "sg22": ("SG", 22)}

@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(tree, ndc, trs (two poses), w, h, f, tuning): the grad tests' small scenes, the 28-level chain (float
    descent), `mixed` -- depth 5 under top_levels = 2, brick_levels = 1, so that most leaves lie below top grid and
    bricks and their sigma exists in node words only -- and `n3`, whose file-side runs (27 * 13 elements) are not
    whole 16-byte pieces.  `edge_<case>`: the full-catalogue tree of grad_util.EDGE_CASES[case].  `sh9`, `n4_sh9`
    and SHAPE_SCENES: the record lengths and runs at which the step and the value passes take another path."""
    tuning = None
    if name == "chain":
        tree, target = common.deep_chain_tree_n2()
        trs = [common.camera_at(target)[0], common.camera_at(target, look_at=(0.4, 0.6, 0.5))[0]]
        _, w, h, f = common.camera_at(target)
        return dict(tree=tree, ndc=None, trs=trs, w=w, h=h, f=f, tuning=None)
    if name == "mixed":
        tree, ndc, tuning = common.small_scene(depth=5, basis_dim=4, seed=77), None, dict(top_levels=2, brick_levels=1)
    elif name == "n3":
        tree, ndc = common.random_tree_general_n(N=3, depth=3, basis_dim=4, seed=5), None
    elif name == "n4_sh9":   # a run of 64 * 28 halfs: longer than the staged value kernels take, on an aligned array
        tree, ndc = common.random_tree_general_n(N=4, depth=3, basis_dim=9, seed=22), None
    elif name == "sh9":      # 17,224 slots: nine 2048-slot groups of the step, the last partial
        tree, ndc = common.small_scene(depth=5, basis_dim=9, seed=609), None
    elif name in SHAPE_SCENES:
        fmt, basis_dim = SHAPE_SCENES[name]
        tree, ndc = common.small_scene(depth=4, basis_dim=basis_dim, fmt=fmt, seed=600 + basis_dim), None
    elif name.startswith("edge_"):   # the full-catalogue value-domain trees of tests/grad_util.py: NaN, +-inf
        tree, ndc = gu.edge_tree(name[5:], "full"), None
    else:
        tree, _, ndc = gu.tree_of(name)
        if name == "blocked":
            tuning = dict(top_levels=2, brick_levels=3, brick_blocked=1)
    if ndc is not None:
        trs, w, h, f = gu.views(name, 0, 2)
    else:
        radius = 2.5 if name == "sh9_near" else 4.0
        trs, w, h, f = gu.poses(2, size=48, radius=radius), 48, 48, common.camera_for(size=48)[3]
    return dict(tree=tree, ndc=ndc, trs=trs, w=w, h=h, f=f, tuning=tuning)


CASES = ["sh16", "sh9_near", "sh25", "rgba", "basis1", "n4", "blocked", "ndc", "chain", "mixed", "n3",
         "asg7", "sg10", "sg11", "sg21", "sg22", "n4_sh9", "sh9"]


def edge_values():
    """float32: what the binary32 -> binary16 rounding has to get right -- ties (to even), values around the binary16
    subnormals and below them, around the largest binary16 and beyond, both signs, +-0, +-inf, NaN."""
    h = np.float32
    ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20, 0.1, 1 / 3,
            2049.0, 2051.0, 2050.5, 1023.75]
    sub = [2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -14 * (1 - 2.0 ** -12),
           2.0 ** -14 - 2.0 ** -25, 2.0 ** -15, 1e-7, 5.5e-8, 1e-40, 2.0 ** -149]
    big = [65504.0, 65519.0, 65520.0, 65536.0, 70000.0, 1e38, 3.4e38]
    vals = ties + sub + big
    vals = vals + [-v for v in vals] + [0.0, -0.0, np.inf, -np.inf, np.nan]
    return np.array(vals, h)


def slot_depths(tree):
    """int [capacity, N^3]: the depth of each slot as VrTreeInfo.max_depth counts it + 1 (a slot of the root has
    depth 1: its cell has extent N^-1); -1 for the slots of nodes the root does not reach."""
    n3 = tree.N ** 3
    child = np.asarray(tree.child).reshape(tree.capacity, n3).astype(np.int64)
    level = np.full(tree.capacity, -1, np.int64)
    level[0] = 0
    frontier = np.array([0])
    while frontier.size:
        kids = (frontier[:, None] + child[frontier])[child[frontier] != 0]
        level[kids] = level[np.repeat(frontier, (child[frontier] != 0).sum(1))] + 1
        frontier = kids
    return np.where(level[:, None] >= 0, level[:, None] + 1, -1) * np.ones((1, n3), np.int64)


TOP, BRICK, WORD = 0, 1, 2


def leaf_kinds(tree, top_levels, brick_levels):
    """int [capacity, N^3]: where the sigma of each LEAF slot lives besides its node word -- TOP: in entries of the
    top grid (depth <= top_levels), BRICK: in brick entries (the next brick_levels levels), WORD: in the node word
    only (deeper leaves, and every leaf of a tree without lookup structure); -1 for internal and unreachable slots."""
    d = slot_depths(tree)
    leaf = (np.asarray(tree.child).reshape(d.shape) == 0) & (d > 0)
    kind = np.full(d.shape, WORD)
    if top_levels > 0:
        kind[d <= top_levels + brick_levels] = BRICK
        kind[d <= top_levels] = TOP
    return np.where(leaf, kind, -1)


def n_bricks(tree, top_levels, brick_levels):
    """Bricks of the lookup structure: the internal nodes of level top_levels."""
    if top_levels <= 0 or brick_levels <= 0:
        return 0
    d = slot_depths(tree)
    return int(((d[:, 0] - 1) == top_levels).sum())


@functools.lru_cache(maxsize=None)
def variant(name, which):
    """Data set `which` (1 or 2) of a scene (variant_of with the scene's seed), computed once."""
    return variant_of(case(name)["tree"], which, 1000 * which + sum(map(ord, name)), chain=name == "chain")


def variant_of(tree, which, seed, chain=False):
    """Data set `which` (1 or 2) of a tree, float16 in the file's shape, read-only: every coefficient seeded
    random (those of internal slots too: upload stores them), and sigma by the rank r of a leaf among all leaves
    ordered by depth -- set 1 occupies r % 2 == 0, set 2 occupies (r // 2) % 2 == 0, so that between the two sets
    any four leaves of consecutive rank (so every range of depths that holds four leaves: every kind of
    leaf_kinds) have one that turns on, one that turns off, one that stays on and one that stays off.  Unoccupied
    leaves alternate between 0 and 0.004 (below sigma_thresh, not zero).  Internal slots get a non-zero sigma,
    which the library must ignore; so do the slots of nodes the root does not reach, leaves or not."""
    rng = np.random.default_rng(seed)
    shape = tree.data.shape
    n3 = tree.N ** 3
    data = (rng.standard_normal(shape) * 0.6).astype(np.float32)
    if tree.format_name == "RGBA":
        data[..., :3] = rng.uniform(0.05, 0.95, size=shape[:-1] + (3,))
    d = slot_depths(tree)
    leaf = (np.asarray(tree.child).reshape(d.shape) == 0) & (d > 0)
    rank = np.zeros(d.shape, np.int64)
    idx = np.flatnonzero(leaf.reshape(-1))
    rank.reshape(-1)[idx[np.argsort(d.reshape(-1)[idx], kind="stable")]] = np.arange(idx.size)
    occupied = leaf & ((rank % 2 == 0) if which == 1 else ((rank // 2) % 2 == 0))
    dense = np.exp(rng.uniform(np.log(2.0), np.log(60.0), size=d.shape))
    if chain:   # steps near the target are ~1e-8 long (common.deep_chain_tree_n2)
        dense = np.where(d > 14, dense * 1e3, dense)
    sigma = np.where(occupied, dense, np.where(rank % 3 == 0, 0.0, 0.004))
    sigma = np.where(leaf, sigma, 7.0 + which)
    data[..., -1] = sigma.reshape(shape[:-1])
    out = data.astype(np.float16)
    out.setflags(write=False)
    assert d.shape == (tree.capacity, n3)
    return out


def with_data(tree, data):
    return dataclasses.replace(tree, data=np.ascontiguousarray(data, np.float16))


def stored(tree, data):
    """What the device holds of `data` (float16, the file's shape): the bits, the sigma of internal slots +0.  A slot
    is internal where its link points inside [1, capacity).  The root reaches no other link; a node it does not reach
    may hold one that leaves the array, and the upload makes a leaf of that slot: it reads back its sigma."""
    out = np.array(data, np.float16, copy=True)
    child = np.asarray(tree.child).astype(np.int64)
    target = np.arange(child.shape[0]).reshape((-1,) + (1,) * (child.ndim - 1)) + child
    out[..., -1][(child != 0) & (target >= 1) & (target < child.shape[0])] = 0
    return out


def flips(tree, top_levels, brick_levels, d_from, d_to):
    """-> {kind: (leaves that rise above sigma_thresh, leaves that fall to or below it)} for the kinds of which the
    tree has four leaves or more."""
    kinds = leaf_kinds(tree, top_levels, brick_levels)
    s0 = (np.asarray(d_from)[..., -1].astype(np.float32) > SIGMA_THRESH).reshape(kinds.shape)
    s1 = (np.asarray(d_to)[..., -1].astype(np.float32) > SIGMA_THRESH).reshape(kinds.shape)
    return {k: (int((~s0 & s1 & (kinds == k)).sum()), int((s0 & ~s1 & (kinds == k)).sum()))
            for k in (TOP, BRICK, WORD) if (kinds == k).sum() >= 4}


# ---- shared by the GPU tests (torch is handed in: the module imports without it) -----------------------------------
def upload(name, data=None):
    """The scene with `data` (None: its own), under the scene's upload-time tuning."""
    from volrend_amd import api
    c = case(name)
    tree = c["tree"] if data is None else with_data(c["tree"], data)
    if c["tuning"]:
        api.set_tuning(**c["tuning"])
    try:
        t = api.N3Tree.from_synth(tree, ndc=c["ndc"])
    finally:
        if c["tuning"]:
            api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    if c["tuning"]:
        info = t.info()
        assert all(info[k] == v for k, v in c["tuning"].items()), info
    return t


def dev(torch, a, dtype=None):
    x = torch.from_numpy(np.array(a, copy=True)).cuda()
    return x if dtype is None else x.to(dtype)
