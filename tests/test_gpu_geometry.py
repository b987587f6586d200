"""-m gpu: vr_tree_geometry / vr_slot_points against the numpy restatement of tests/geometry_util.py, bit for bit: the
raw C calls over the trees of geometry_util.TREES (every output sized exactly, poisoned beforehand, with a guard band
behind it that must keep its bits), the points over slot lists of every shape, and through the library -- the points
of every leaf of an uploaded tree, fed to vr_query_points, find the leaf they were made for.  No cyclic child array
goes to the device: the walk's counted loop is checked by reading it."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from tests import common
from tests import geometry_util as gu
from tests import refine_util as ru
from tests import collapse_util as cu
from volrend_amd import _abi, api, synth

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512
OUTPUTS = ("parent_slot", "node_depth", "node_origin")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


@functools.lru_cache(maxsize=None)
def tree_of(name):
    """-> (child, N, (parent_slot, node_depth, node_origin) of the restatement): computed once, never written."""
    child = np.ascontiguousarray(gu.TREES[name](), np.int32)
    want = gu.restate(child)
    for a in (child, *want):
        a.setflags(write=False)
    return child, gu.branching(child), want


class Guarded:
    """A device buffer of exactly ``nbytes`` bytes, poisoned, with a poisoned guard band behind it."""

    def __init__(self, torch, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.raw.data_ptr()

    def bits(self, dtype):
        host = self.raw.cpu().numpy()
        assert (host[self.nbytes:] == POISON).all(), "a store went beyond the end of an output"
        return host[:self.nbytes].view(dtype)


def run_geometry(torch, child, N, outputs=OUTPUTS):
    """vr_tree_geometry on the null stream -> dict name -> host array; an output not asked for is None."""
    cap = child.shape[0]
    child_dev = torch.from_numpy(child.copy()).cuda()
    bufs = {"parent_slot": Guarded(torch, cap * 4), "node_depth": Guarded(torch, cap * 4),
            "node_origin": Guarded(torch, cap * 12)}
    g = _abi.VrGeometry()
    g.child, g.capacity, g.N = child_dev.data_ptr(), cap, N
    for name in outputs:
        setattr(g, name, bufs[name].ptr)
    _abi.check(_abi.lib().vr_tree_geometry(C.byref(g), None))
    torch.cuda.synchronize()
    got = {"parent_slot": bufs["parent_slot"].bits(np.int32), "node_depth": bufs["node_depth"].bits(np.int32),
           "node_origin": bufs["node_origin"].bits(np.uint32).reshape(cap, 3)}
    for name in OUTPUTS:
        if name not in outputs:
            assert (got[name].view(np.uint8) == POISON).all(), f"{name} was not asked for"
            got[name] = None
    return got


@pytest.mark.parametrize("outputs", [OUTPUTS, ("parent_slot",), ("node_depth",), ("node_origin",)], ids="+".join)
@pytest.mark.parametrize("name", sorted(gu.TREES))
def test_geometry_matches_the_restatement(torch_cuda, name, outputs):
    child, N, (parent, depth, origin) = tree_of(name)
    got = run_geometry(torch_cuda, child, N, outputs)
    if "parent_slot" in outputs:
        assert np.array_equal(got["parent_slot"], parent)
    if "node_depth" in outputs:
        assert np.array_equal(got["node_depth"], depth)
    if "node_origin" in outputs:
        assert np.array_equal(got["node_origin"][depth >= 0], origin[depth >= 0])


def test_the_trees_are_what_their_names_say():
    assert tree_of("full_n2_73")[0].shape[0] == 73 and all(tree_of(n)[0].shape[0] % 64 for n in gu.TREES)
    assert tree_of("chain_n2_40")[2][2].max() >= 2 ** 31 and tree_of("chain_n2_40")[2][1].max() == 39
    assert tree_of("chain_n16_9")[2][1].max() == 8
    d70 = tree_of("chain_n2_70")[2][1]
    assert d70.max() == 64 and (d70 == -1).sum() == 5
    p, d, _ = tree_of("orphans_n2")[2]
    assert (p[-2:] == -1).all() and (d[-2:] == -1).all() and (d[:-2] >= 0).all()
    child = tree_of("bad_link_n2")[0]
    m = np.arange(child.shape[0])[:, None] + child
    assert ((child != 0) & ((m < 1) | (m >= child.shape[0]))).sum() == 1
    rc = tree_of("refined_collapsed_n2")[2][1]
    assert (np.diff(rc) < 0).any()                                 # not breadth-first


# ---- points ----
def run_points(torch, N, depth, origin, slots, k, mode, seed, outputs=("points", "depth", "side")):
    n = len(slots)
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda() for a in (depth, origin, slots)]
    bufs = {"points": Guarded(torch, n * k * 12), "depth": Guarded(torch, n * 4), "side": Guarded(torch, n * 4)}
    p = _abi.VrSlotPoints()
    p.node_depth, p.node_origin, p.slots = (t.data_ptr() for t in dev)
    for name in outputs:
        setattr(p, name, bufs[name].ptr)
    p.capacity, p.n, p.N, p.k, p.mode, p.seed = depth.size, n, N, k, mode, seed
    _abi.check(_abi.lib().vr_slot_points(C.byref(p), None))
    torch.cuda.synchronize()
    return (bufs["points"].bits(np.float32).reshape(n, k, 3), bufs["depth"].bits(np.int32),
            bufs["side"].bits(np.float32))


def assert_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def slot_lists(child, depth, seed=0):
    """name -> int32 slot list: all reachable leaves, a shuffled subset, repeats, internal slots, indices out of
    range and slots of nodes without a depth, and lists of 1, 63, 64, 65 and 1000 entries."""
    rng = np.random.default_rng(seed)
    cap, N3 = child.shape
    leaves = gu.reachable_leaves(child, depth)
    internal = np.flatnonzero(child.reshape(-1) != 0).astype(np.int32)
    lists = {"all_leaves": leaves, "shuffled": rng.permutation(leaves)[:max(1, leaves.size // 3)],
             "repeats": rng.choice(leaves, 150), "bad": np.array([-1, cap * N3, 2 ** 31 - 1, -2 ** 31, leaves[0]], np.int32)}
    if internal.size:
        lists["internal"] = np.concatenate([internal[:40], leaves[:3]])
    if (depth < 0).any():
        lists["unreachable"] = np.concatenate([np.flatnonzero(np.repeat(depth < 0, N3))[:20], leaves[:2]])
    for n in (1, 63, 64, 65, 1000):
        lists[f"n{n}"] = rng.choice(np.arange(cap * N3), n)
    return {k: np.ascontiguousarray(v, np.int32) for k, v in lists.items()}


POINT_TREES = ("random_n2", "random_n3", "random_n4", "orphans_n2", "chain_n2_40", "chain_n16_9", "chain_n2_70")


@pytest.mark.parametrize("mode,k", [(gu.CENTER, 1), (gu.JITTER, 1), (gu.JITTER, 3), (gu.JITTER, 64), (gu.CENTER, 3),
                                    (gu.CENTER, 64)])
@pytest.mark.parametrize("name", POINT_TREES)
def test_points_match_the_restatement(torch_cuda, name, mode, k):
    child, N, (_, depth, origin) = tree_of(name)
    seed = 0x9E3779B9 if k == 3 else 5
    for what, slots in slot_lists(child, depth).items():
        if k == 64 and slots.size > 1000:
            slots = slots[:1000]
        want = gu.points(depth, origin, N, slots, k, mode, seed)
        got = run_points(torch_cuda, N, depth, origin, slots, k, mode, seed)
        for g, w, field in zip(got, want, ("points", "depth", "side")):
            assert g.dtype == w.dtype and g.shape == w.shape
            assert_bits(g, w, (name, what, field)) if w.dtype == np.float32 else np.testing.assert_array_equal(g, w)
        if what in ("bad", "unreachable"):
            assert np.isnan(got[0]).any() and (got[1] == -1).any() and not np.isnan(got[0][-1]).any()


def test_points_outputs_alone_and_split_lists(torch_cuda):
    child, N, (_, depth, origin) = tree_of("random_n2")
    slots = slot_lists(child, depth)["n1000"]
    whole = run_points(torch_cuda, N, depth, origin, slots, 3, gu.JITTER, 77)
    for i, name in enumerate(("points", "depth", "side")):
        got = run_points(torch_cuda, N, depth, origin, slots, 3, gu.JITTER, 77, outputs=(name,))
        for j, (g, w) in enumerate(zip(got, whole)):
            if i == j:
                assert g.tobytes() == w.tobytes(), name
            else:
                assert (g.view(np.uint8) == POISON).all(), name
    for cut in (1, 333, 640):
        parts = [run_points(torch_cuda, N, depth, origin, s, 3, gu.JITTER, 77) for s in (slots[:cut], slots[cut:])]
        for w, a, b in zip(whole, *parts):
            assert np.concatenate([a, b]).tobytes() == w.tobytes(), cut
    order = np.random.default_rng(1).permutation(slots.size)
    shuffled = run_points(torch_cuda, N, depth, origin, slots[order], 3, gu.JITTER, 77)
    assert all(s.tobytes() == w[order].tobytes() for s, w in zip(shuffled, whole))


# ---- through the library ----
@functools.lru_cache(maxsize=None)
def scene(name):
    """A tree whose every leaf holds a record of its own, so that the record a query returns names the slot."""
    if name == "n2_depth6":
        return gu.distinct_records(common.small_scene(depth=6, basis_dim=4, seed=31))
    return gu.distinct_records(common.random_tree_general_n(N=4, depth=3, seed=8))


@pytest.mark.parametrize("mode,k", [("center", 1), ("jitter", 5)])
@pytest.mark.parametrize("name", ["n2_depth6", "general_n4"])
def test_query_points_finds_the_leaf_the_points_were_made_for(torch_cuda, name, mode, k):
    """Every leaf, none left out: tests/test_geometry_host.py shows from the restatement that all of them qualify."""
    torch = torch_cuda
    synth_tree = scene(name)
    child, dd = common.rows_of(synth_tree), synth_tree.data_dim
    records = synth_tree.data.reshape(-1, dd)
    leaf_records = records[child.reshape(-1) == 0].view(np.uint16)
    assert np.unique(leaf_records, axis=0).shape[0] == leaf_records.shape[0]      # equal record <=> same slot
    tree = api.N3Tree.from_synth(synth_tree)
    try:
        geo = tree.geometry()
        _, depth, origin = gu.restate(child)
        assert np.array_equal(geo["node_depth"].cpu().numpy(), depth)
        assert np.array_equal(geo["node_origin"].cpu().numpy().view(np.uint32), origin)
        leaves = torch.nonzero(torch.from_numpy(child.reshape(-1) == 0).cuda()).reshape(-1).to(torch.int32)
        res = tree.slot_points(leaves, k=k, mode=mode, seed=3, geometry=geo)
        alone = tree.slot_points(leaves, k=k, mode=mode, seed=3)             # (computes the geometry itself)
        assert all(torch.equal(res[w], alone[w]) for w in res)
        q = tree.query(res["points"].reshape(-1, 3), want=("depth", "sigma", "coeffs"), space="tree")
        torch.cuda.synchronize()
        s = np.repeat(leaves.cpu().numpy(), k)
        assert s.size == (child == 0).sum() * k
        assert np.array_equal(q["depth"].cpu().numpy(), depth[s // child.shape[1]])
        assert np.array_equal(res["depth"].cpu().numpy(), depth[leaves.cpu().numpy() // child.shape[1]])
        assert q["sigma"].cpu().numpy().tobytes() == records[s, -1].astype(np.float32).tobytes()
        assert q["coeffs"].cpu().numpy().tobytes() == records[s, :-1].astype(np.float32).tobytes()
        world = tree.slot_points(leaves[:100], k=k, mode=mode, seed=3, space="world", geometry=geo)["points"]
        back = world.cpu().numpy() * tree.scale + tree.offset
        np.testing.assert_allclose(back, res["points"][:100].cpu().numpy(), rtol=0, atol=1e-5)
        empty = tree.slot_points(leaves[:0], k=k)
        assert empty["points"].shape == (0, k, 3) and empty["depth"].shape == (0,)
    finally:
        tree.free_device()


def test_parent_depth_of_a_refined_then_collapsed_tree(torch_cuda, tmp_path):
    torch = torch_cuda
    synth_tree = common.random_tree_general_n(N=2, depth=5, seed=4, p_refine=0.5)      # as gu.refined_collapsed
    tree = api.N3Tree.from_synth(synth_tree)
    child = common.rows_of(synth_tree).astype(np.int32)
    sel = ru.selections(child, seed=104)["random30"]
    refined = tree.refine(torch.from_numpy(sel).cuda())["tree"]
    child_r = refined.child_.reshape(refined.capacity, -1)
    collapsed = refined.collapse(torch.from_numpy(cu.selections(child_r, seed=105)["random50"]).cuda())["tree"]
    try:
        child_c = collapsed.child_.reshape(collapsed.capacity, -1)
        assert np.array_equal(child_c, tree_of("refined_collapsed_n2")[0])
        parent, depth, _ = gu.restate(child_c)
        assert (np.diff(depth) < 0).any()                           # not breadth-first
        want = np.stack([parent, depth], axis=1)
        want[0, 0] = 0
        got = collapsed.parent_depth().cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want)
        N = collapsed.N
        st = dataclasses.replace(synth_tree, child=collapsed.child_,
                                 data=collapsed.read_data().cpu().numpy().reshape(-1, N, N, N, collapsed.data_dim))
        plain, filled = str(tmp_path / "plain.npz"), str(tmp_path / "filled.npz")
        synth.save_npz(st, plain)
        synth.save_npz(st, filled, parent_depth=got)
        za, zb = np.load(plain), np.load(filled)
        assert sorted(za.files) == sorted(zb.files) and np.array_equal(zb["parent_depth"], want)
        assert all(za[key].tobytes() == zb[key].tobytes() for key in za.files if key != "parent_depth")
        loaded = api.N3Tree(filled, upload=False)
        assert np.array_equal(loaded.child_, collapsed.child_) and loaded.data_.tobytes() == st.data.tobytes()
    finally:
        for t in (tree, refined, collapsed):
            t.free_device()
