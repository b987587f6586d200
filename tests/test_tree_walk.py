"""The host walks of an upload (volrend_amd/csrc/vr_tree_walk.cpp) on their own: topology check, node
numbering, the shape of the lookup structure.  tests/cpp/walk_check.cpp is built with plain g++ against
that one source -- no HIP, no library -- and its output is checked against walks written here in
numpy / Python."""
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from tests.common import rows_of, scrambled, with_unreachable


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.csrc_program("walk_check", "vr_tree_walk", tmp_path_factory.mktemp("bin"))


def run_walk(exe, tmp_path, child, G0=0, BL=0, cap=None):
    """-> dict(depth, level, perm, roots), or the `why` text of a bad tree."""
    child = np.ascontiguousarray(child, np.int32)
    cap = child.shape[0] if cap is None else cap
    p = str(tmp_path / "child.bin")
    child.tofile(p)
    out = subprocess.check_output([exe, "walk", p, str(cap), str(child.shape[1]), str(G0), str(BL)], text=True)
    if out.startswith("why "):
        return out[4:].rstrip("\n")
    rows = {l.split()[0]: np.array(l.split()[1:], np.int64) for l in out.splitlines()}
    return dict(depth=int(rows["depth"][0]), level=rows["level"], perm=rows["perm"], roots=rows["roots"])


def plan(exe, N, max_depth, capacity, top_levels=0, brick_levels=3, n_roots=1000):
    out = subprocess.check_output([exe, "plan", *map(str, (N, max_depth, capacity, top_levels, brick_levels,
                                                           n_roots))], text=True)
    return tuple(int(x) for x in out.split())


# ---- trees ---------------------------------------------------------------------------------------

def chain(levels, backward=False):
    """N = 2 nodes in a row: node levels 0 .. `levels`.  backward: root, then the chain from its far end."""
    cap = levels + 1
    order = np.arange(cap) if not backward else np.concatenate([[0], np.arange(cap - 1, 0, -1)])
    child = np.zeros((cap, 8), np.int64)
    child[order[:-1], 5] = order[1:] - order[:-1]
    return child


TREES = {
    "scene4": lambda: rows_of(common.small_scene(depth=4)),
    "general_n3": lambda: rows_of(common.random_tree_general_n(N=3)),
    "general_n4": lambda: rows_of(common.random_tree_general_n(N=4)),
    "scrambled": lambda: scrambled(rows_of(common.small_scene(depth=5, basis_dim=9, seed=391)))[0],
    "unreachable": lambda: with_unreachable(rows_of(common.small_scene(depth=4))),
    "unreachable_scrambled": lambda: with_unreachable(scrambled(rows_of(common.small_scene(depth=4)))[0]),
    "deep_chain": lambda: rows_of(common.deep_chain_tree_n2(28)[0]),
    # common.renumbered: every link backward; a subtree cut off in the middle of the array; both, and slack behind
    "reversed": lambda: rows_of(common.renumbered(common.small_scene(depth=4), ["reversed"])[0]),
    "pruned": lambda: rows_of(common.renumbered(common.small_scene(depth=5, basis_dim=9, seed=391), ["pruned"])[0]),
    "pruned_reversed_slack": lambda: rows_of(common.renumbered(common.small_scene(depth=5, basis_dim=9, seed=391),
                                                               ["pruned", "reversed", "slack_linked"])[0]),
}


@pytest.fixture(scope="module", params=sorted(TREES))
def tree(request):
    return TREES[request.param]()


# ---- the walks again, in numpy / Python ----------------------------------------------------------

def kids(child, n):
    return [n + int(c) for c in child[n] if c != 0]


def np_levels(child):
    """Level of every node, breadth-first from the root; 255 = not reachable."""
    level = np.full(child.shape[0], 255, np.int64)
    level[0] = 0
    front, d = np.array([0]), 0
    while True:
        links = child[front]
        front = (front[:, None] + links)[links != 0]
        if front.size == 0:
            return d, level
        d += 1
        level[front] = d


def subtree(child, n):
    """Old indices of the subtree of n, pre-order, children in slot order."""
    out = [n]
    for c in kids(child, n):
        out += subtree(child, c)
    return out


def numbering(child, level, G0, BL):
    """The rule of node_permutation, recursively: -> old indices in their new order, brick roots (old indices)."""
    order, roots = [], []

    def visit(n):
        order.append(n)
        ring = [n]
        if G0 > 0 and level[n] == G0:
            roots.append(n)
            for _ in range(1, BL):
                ring = [c for m in ring for c in kids(child, m)]
                order.extend(ring)
        for m in ring:
            for c in kids(child, m):
                visit(c)

    visit(0)
    return order, roots


# ---- validate_topology ---------------------------------------------------------------------------

def test_depth_and_levels_are_the_numpy_walks(exe, tmp_path, tree):
    got = run_walk(exe, tmp_path, tree)
    depth, level = np_levels(tree)
    assert got["depth"] == depth
    assert np.array_equal(got["level"], level)
    assert ((level == 255) == (got["level"] == 255)).all()


@pytest.mark.parametrize("name", ["scene4", "general_n3", "unreachable", "deep_chain"])
def test_forward_sweep_and_general_walk_agree(exe, tmp_path, name):
    fwd = TREES[name]()
    reach = np_levels(fwd)[1] != 255
    assert not (fwd[reach] < 0).any()                       # the sweep in index order decides this one
    scr, new_of = scrambled(fwd)
    assert (scr[new_of[reach]] < 0).any()                   # ... and gives this one up
    a, b = run_walk(exe, tmp_path, fwd), run_walk(exe, tmp_path, scr)
    assert a["depth"] == b["depth"]
    assert np.array_equal(b["level"][new_of], a["level"])


def prefixed(fault):
    """A tree the general walk decides: 0 -> 2 -> 1 (a backward link), and `fault` as the links of node 1."""
    child = np.zeros((5, 8), np.int64)
    child[0, 0], child[2, 0] = 2, -1
    child[1] = fault
    return child


def slots(**kw):
    row = np.zeros(8, np.int64)
    for k, v in kw.items():
        row[int(k[1:])] = v
    return row


BAD = {
    "cycle": (np.stack([slots(s0=1), slots(s0=1), slots(s4=-1)]), "node 1 is linked twice (cycle or DAG)"),
    "cycle_through_root": (np.stack([slots(s0=1), slots(s0=-1)]), "node 1 slot 0 links outside the tree (0)"),
    "dag": (np.stack([slots(s0=1, s1=1), slots()]), "node 1 is linked twice (cycle or DAG)"),
    "dag_two_parents": (np.stack([slots(s0=1, s1=2), slots(s7=2), slots(s0=1), slots()]),
                        "node 3 is linked twice (cycle or DAG)"),
    "beyond_cap": (np.stack([slots(s3=5), slots()]), "node 0 slot 3 links outside the tree (5)"),
    "at_cap": (np.stack([slots(s3=1), slots(s6=1)]), "node 1 slot 6 links outside the tree (2)"),
    "chain_61": (chain(61), "tree deeper than 60 levels"),
    # the same faults behind a backward link: the general walk meets them
    "general_cycle": (prefixed(slots(s0=1)), "node 2 is linked twice (cycle or DAG)"),
    "general_dag": (prefixed(slots(s0=2, s1=2)), "node 3 is linked twice (cycle or DAG)"),
    "general_beyond_cap": (prefixed(slots(s3=100)), "node 1 slot 3 links outside the tree (101)"),
    "general_at_cap": (prefixed(slots(s3=4)), "node 1 slot 3 links outside the tree (5)"),
    "general_below_zero": (prefixed(slots(s3=-5)), "node 1 slot 3 links outside the tree (-4)"),
    "general_to_root": (prefixed(slots(s3=-1)), "node 1 slot 3 links outside the tree (0)"),
    "general_chain_61": (chain(61, backward=True), "tree deeper than 60 levels"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_trees_and_their_messages(exe, tmp_path, name):
    child, why = BAD[name]
    assert run_walk(exe, tmp_path, child) == why


@pytest.mark.parametrize("backward", [False, True], ids=["sweep", "general"])
def test_sixty_levels_are_accepted(exe, tmp_path, backward):
    got = run_walk(exe, tmp_path, chain(60, backward))
    assert got["depth"] == 60 and sorted(got["level"]) == list(range(61))


def test_empty_capacity(exe, tmp_path):
    assert run_walk(exe, tmp_path, np.zeros((0, 8)), cap=0) == "capacity must be positive"


# ---- node_permutation ----------------------------------------------------------------------------

def check_runs(child, perm, nodes, preorder=True):
    """The subtree of each of `nodes` is one contiguous run that starts with the node (in pre-order)."""
    for n in nodes:
        got = perm[subtree(child, n)]
        assert np.array_equal(got if preorder else np.sort(got), perm[n] + np.arange(got.size)), f"subtree of node {n}"


def check_unreachable_last(level, perm):
    cap = level.size
    assert np.array_equal(np.sort(perm), np.arange(cap))
    reach, lost = np.flatnonzero(level != 255), np.flatnonzero(level == 255)
    assert np.array_equal(np.sort(perm[reach]), np.arange(reach.size))
    assert np.array_equal(perm[lost], reach.size + np.arange(lost.size))    # old relative order


def test_plain_numbering_is_preorder(exe, tmp_path, tree):
    got = run_walk(exe, tmp_path, tree)
    level, perm = got["level"], got["perm"]
    check_unreachable_last(level, perm)
    assert perm[0] == 0 and got["roots"].size == 0
    order = subtree(tree, 0)                                 # pre-order, slot order
    assert np.array_equal(perm[order], np.arange(len(order)))
    check_runs(tree, perm, np.flatnonzero(level != 255))


BRICK_TREES = ["scene4", "scrambled", "unreachable_scrambled", "reversed", "pruned", "pruned_reversed_slack"]
# scene4 has node levels 0..3: (3, 2) puts the roots at the deepest level and (1, 4) asks for a level that
# does not exist, so roots have none or only some of their BL - 1 levels below them; BL = 1: no front
SHAPES = [(1, 2), (2, 2), (1, 3), (3, 2), (2, 1), (1, 1), (1, 4)]


@pytest.mark.parametrize("G0,BL", SHAPES)
@pytest.mark.parametrize("name", BRICK_TREES)
def test_brick_numbering(exe, tmp_path, name, G0, BL):
    child = TREES[name]()
    got = run_walk(exe, tmp_path, child, G0, BL)
    level, perm, roots = got["level"], got["perm"], got["roots"]
    check_unreachable_last(level, perm)
    assert perm[0] == 0
    old_roots = np.flatnonzero(level == G0)
    assert old_roots.size > 1
    assert np.array_equal(roots, np.sort(perm[old_roots])) and (np.diff(roots) > 0).all()
    short = 0
    for r in old_roots:
        # levels G0+1 .. G0+BL-1 below r, breadth-first in slot order: one run right behind r
        ring, front = [r], []
        for _ in range(1, BL):
            ring = [c for m in ring for c in kids(child, m)]
            front += ring
        short += len(front) == 0 or level[front[-1]] < G0 + BL - 1
        assert np.array_equal(perm[front], perm[r] + 1 + np.arange(len(front))), f"front of root {r}"
        # then the deeper subtrees, one after the other, each contiguous and depth-first
        at = perm[r] + 1 + len(front)
        deeper = [c for m in ring for c in kids(child, m)]
        for c in deeper:
            assert perm[c] == at, f"subtree {c} below root {r}"
            at += len(subtree(child, c))
        check_runs(child, perm, deeper)
        assert at == perm[r] + len(subtree(child, r))        # the whole brick subtree is one run
    if G0 + BL - 1 > got["depth"]:
        assert short == old_roots.size                       # no root has BL - 1 levels below it
    check_runs(child, perm, np.flatnonzero(level <= G0), preorder=False)
    # ... and all of it at once: the rule, written recursively
    order, rule_roots = numbering(child, level, G0, BL)
    assert np.array_equal(perm[order], np.arange(len(order)))
    assert np.array_equal(roots, np.sort(perm[rule_roots]))


# ---- plan_lookup ---------------------------------------------------------------------------------

def test_lookup_shape_rule(exe):
    assert plan(exe, 2, 8, 300_000) == (6, 3)
    assert plan(exe, 2, 9, 2_000_000) == (7, 3)
    assert plan(exe, 2, 12, 2_000_000)[0] == 8
    assert plan(exe, 2, 3, 100) == (4, 0)                    # the top grid resolves every leaf
    assert plan(exe, 2, 0, 1) == (1, 0)
    # overrides and their clamps
    assert plan(exe, 2, 8, 300_000, top_levels=5) == (5, 3)
    assert plan(exe, 2, 8, 300_000, top_levels=7) == (7, 2)
    assert plan(exe, 2, 8, 300_000, top_levels=12) == (8, 1)
    assert plan(exe, 2, 3, 100, top_levels=8) == (4, 0)
    assert plan(exe, 2, 3, 100, top_levels=2) == (2, 2)
    assert plan(exe, 2, 8, 300_000, brick_levels=0) == (6, 1)
    assert plan(exe, 2, 8, 300_000, brick_levels=-3) == (6, 1)
    assert plan(exe, 2, 12, 300_000, brick_levels=9) == (8, 4)
    assert plan(exe, 2, 12, 300_000, brick_levels=2) == (8, 2)
    # brick entries are addressed with 32-bit byte offsets: n_roots << 3 BL entries of 4 bytes stay below 2^32
    assert plan(exe, 2, 9, 2_000_000, n_roots=(1 << 21) - 1) == (7, 3)
    assert plan(exe, 2, 9, 2_000_000, n_roots=1 << 21) == (7, 2)
    assert plan(exe, 2, 12, 2_000_000, brick_levels=4, n_roots=(1 << 18) - 1) == (8, 4)
    assert plan(exe, 2, 12, 2_000_000, brick_levels=4, n_roots=1 << 18) == (8, 3)
    assert plan(exe, 2, 9, 2_000_000, n_roots=(1 << 24) - 1) == (7, 2)
    assert plan(exe, 2, 9, 2_000_000, n_roots=1 << 24) == (7, 1)
    assert plan(exe, 2, 9, 2_000_000, n_roots=1 << 40) == (7, 1)         # BL never drops below 1
    # no lookup structure: not N = 2, or a tree that vr_query_mode_for sends to the descent
    assert plan(exe, 3, 3, 100) == (0, 0) and plan(exe, 4, 2, 10) == (0, 0)
    assert plan(exe, 2, 23, 100) == (8, 3) and plan(exe, 2, 24, 100) == (0, 0)
    assert plan(exe, 2, 9, (1 << 27) - 1) == (7, 3) and plan(exe, 2, 9, 1 << 27) == (0, 0)
