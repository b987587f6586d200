"""Helpers of the renumbered-tree tests (tests/test_renumbered_host.py, tests/test_gpu_renumbered.py): the scenes,
each under the kinds of common.renumbered, and how a per-node array of the original follows its nodes (needs no GPU)."""
from __future__ import annotations

import functools

import numpy as np

from tests import common

# name -> (tree, upload-time tuning, the slot depth `pruned` cuts at).  n3 has three node levels, so a slot of
# depth 2 has a single node below it: there the cut is a slot of the root, whose subtree has the 8 nodes.
SCENES = {
    "sh9": (lambda: common.small_scene(depth=5, basis_dim=9, seed=609), None, 2),
    "mixed": (lambda: common.small_scene(depth=5, basis_dim=4, seed=77), dict(top_levels=2, brick_levels=1), 2),
    "blocked": (lambda: common.small_scene(depth=5, basis_dim=4, seed=78),
                dict(top_levels=2, brick_levels=3, brick_blocked=1), 2),
    "rgba": (lambda: common.small_scene(depth=4, basis_dim=-1, fmt="RGBA", seed=8), None, 2),
    "n3": (lambda: common.random_tree_general_n(N=3, depth=3, basis_dim=4, seed=5), None, 1),
}
LOOKUP_SCENES = ("mixed", "blocked")
POWER_OF_TWO = ("sh9", "mixed", "blocked", "rgba")
COMBINED = ("random", "pruned", "slack_linked")          # calls that take a tree handle
RAW = ("random", "pruned", "slack_zero")                 # raw child arrays: inside vr_tree_geometry's contract
SIZE = 48


def views():
    """-> (two orbit poses, w, h, focal): the frames of update_util.case."""
    trs = [common.camera_for(pose_idx=i, size=SIZE)[0] for i in range(2)]
    return trs, SIZE, SIZE, common.camera_for(size=SIZE)[3]


@functools.lru_cache(maxsize=None)
def base(scene):
    return SCENES[scene][0]()


@functools.lru_cache(maxsize=None)
def case(scene, kinds):
    """-> dict(tree (the renumbered tree), new_of, orig (the tree it restates: the scene, pruned where `kinds` prunes,
    in the scene's own numbering), orphan (bool [capacity of tree]), tuning).  `kinds`: a tuple."""
    tree0, tuning, prune_depth = SCENES[scene]
    kinds = tuple(kinds)
    orig = base(scene)
    if "pruned" in kinds:
        orig = common.renumbered(orig, ["pruned"], prune_depth=prune_depth)[0]
    tree, new_of = common.renumbered(base(scene), kinds, seed=7, prune_depth=prune_depth)
    return dict(tree=tree, new_of=new_of, orig=orig, orphan=common.orphan_nodes(tree), tuning=tuning)


def carry(a, new_of, capacity, fill=0):
    """A per-node array of the original (first axis: node) in the numbering of the renumbered tree; rows of nodes
    without an old index hold `fill`."""
    a = np.asarray(a)
    out = np.full((capacity,) + a.shape[1:], fill, a.dtype)
    out[new_of] = a
    return out


def carry_slots(flat, new_of, capacity, N3, fill=0):
    """carry() for an array indexed by slot (flat [old capacity * N3, ...])."""
    flat = np.asarray(flat)
    a = flat.reshape((new_of.size, N3) + flat.shape[1:])
    return carry(a, new_of, capacity, fill).reshape((capacity * N3,) + flat.shape[1:])


def upload(c, tree=None):
    """The case's tree (or `tree`, another data set on the same child array) under the scene's upload-time tuning."""
    from volrend_amd import api
    tuning = c["tuning"]
    if tuning:
        api.set_tuning(**tuning)
    try:
        t = api.N3Tree.from_synth(c["tree"] if tree is None else tree)
    finally:
        if tuning:
            api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    if tuning:
        info = t.info()
        assert all(info[k] == v for k, v in tuning.items()), info
    return t
