"""vr_collapse_plan / vr_collapse_apply without a GPU: the symbols, prototypes and struct layouts, every refusal of
the header (with pointers that are never followed) through C and through Python, and the semantics as
tests/collapse_util.py restates them: refine then collapse of the new nodes is the identity, collapsing everything
walks a full tree up level by level, a restated tree passes the upload's host walk, and the oracle's point query finds
the points of collapsed nodes one level higher, in the merged slot, with the MEAN record."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from tests import build_util, common, query_util
from tests import collapse_util as cu
from tests import refine_util as ru
from tests.test_tree_walk import run_walk
from volrend_amd import _abi, api

FUNCS = ("vr_collapse_workspace", "vr_collapse_plan", "vr_collapse_apply")
INVALID, UNSUPPORTED = 1, 5


def test_symbols_are_exported_and_prototyped():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for f in FUNCS:
        assert f in exported and f in _abi.PROTOTYPES, f
    assert _abi.lib().vr_abi_version() == 3                       # additive: the version stands
    assert _abi.COLLAPSE_MAX_ARRAYS == 8
    assert (_abi.COLLAPSE_KEEP, _abi.COLLAPSE_ZERO, _abi.COLLAPSE_MEAN) == (0, 1, 2) == (cu.KEEP, cu.ZERO, cu.MEAN)


def test_struct_layouts_match_the_c_compiler():
    for name, st in (("VrCollapse", _abi.VrCollapse), ("VrCollapseArray", _abi.VrCollapseArray)):
        got = build_util.c_struct_layout(name, st, [("max", "VR_COLLAPSE_MAX_ARRAYS"), ("keep", "VR_COLLAPSE_KEEP"),
                                                    ("zero", "VR_COLLAPSE_ZERO"), ("mean", "VR_COLLAPSE_MEAN")])
        assert got["size"] == C.sizeof(st), name
        for fname, _ in st._fields_:
            assert got[fname] == getattr(st, fname).offset, f"{name}.{fname}"
        assert (got["max"], got["keep"], got["zero"], got["mean"]) == (8, 0, 1, 2)


def test_workspace_rule():
    L = _abi.lib()
    assert L.vr_collapse_workspace(2, 1) > 0
    sizes = [L.vr_collapse_workspace(2, c) for c in (1, 10, 1000, 10 ** 6, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # per 32 nodes: a collapse word, two 64-bit words and a byte of the scan's storage; per node: apply's own into_slot
    assert 4 * 10 ** 6 + 20 * (10 ** 6 // 32) <= sizes[3] <= 4 * 10 ** 6 + 22 * (10 ** 6 // 32) + (1 << 17)
    assert L.vr_collapse_workspace(16, 1000) == L.vr_collapse_workspace(2, 1000)      # (the bitmap is over nodes)
    for N, cap in ((1, 10), (17, 10), (2, 0), (2, -4), (2, 2 ** 31)):
        assert L.vr_collapse_workspace(N, cap) == -1


# ---- refusals through C: every pointer is junk and must never be followed ----
def _valid(n_arrays=3):
    L = _abi.lib()
    arrays = (_abi.VrCollapseArray * 8)()
    for i in range(8):
        arrays[i].src, arrays[i].dst = 0x10000 + 0x2000 * i, 0x11000 + 0x2000 * i
        arrays[i].elem_bytes, arrays[i].dim, arrays[i].rule = (2, 4)[i % 2], 1 + 7 * i, i % 3
    r = _abi.VrCollapse()
    r.child, r.sel, r.child_out, r.workspace = 0x1000, 0x2000, 0x3000, 0x5000
    r.node_map, r.src_node, r.into_slot = 0x6000, 0x7000, 0x8000
    r.arrays, r.n_arrays = arrays, n_arrays
    r.capacity, r.N, r.n_keep = 10, 2, 7
    r.workspace_bytes = L.vr_collapse_workspace(2, 10)
    return r, arrays


def _refused(call, r, code=INVALID, match=None):
    L = _abi.lib()
    n_keep = C.c_int64(-7)
    rc = (L.vr_collapse_plan(C.byref(r), C.byref(n_keep), None) if call == "plan" else
          L.vr_collapse_apply(C.byref(r), None))
    msg = L.vr_last_error().decode()
    assert rc == code and f"vr_collapse_{call}" in msg, (rc, msg)
    assert match is None or match in msg, msg
    assert n_keep.value == -7


@pytest.mark.parametrize("call", ["plan", "apply"])
def test_c_refusals_common_to_both_calls(call):
    L = _abi.lib()
    n_keep = C.c_int64(0)
    assert (L.vr_collapse_plan(None, C.byref(n_keep), None) if call == "plan" else
            L.vr_collapse_apply(None, None)) == INVALID
    for field in ("child", "sel", "workspace"):
        r, _ = _valid()
        setattr(r, field, None)
        _refused(call, r, match="NULL")
    for N in (-1, 0, 1, 17):
        r, _ = _valid()
        r.N = N
        _refused(call, r, match="N=")
    for cap in (0, -1, 2 ** 31):
        r, _ = _valid()
        r.capacity = cap
        _refused(call, r, match="capacity")
    r, _ = _valid()
    r.workspace_bytes -= 1
    _refused(call, r, match="workspace")
    r, _ = _valid()
    r.workspace_bytes = -1
    _refused(call, r, match="workspace")
    r, _ = _valid()
    r.workspace += 128
    _refused(call, r, match="aligned")


def test_c_refusals_of_plan():
    r, _ = _valid()
    assert _abi.lib().vr_collapse_plan(C.byref(r), None, None) == INVALID
    assert "vr_collapse_plan" in _abi.lib().vr_last_error().decode()


def test_c_refusals_of_apply():
    r, _ = _valid()
    r.child_out = None
    _refused("apply", r, match="child_out")
    r, _ = _valid()
    r.child_out = r.child
    _refused("apply", r, match="child_out")
    for n in (0, -1, 11):                                   # outside [1, capacity = 10]
        r, _ = _valid()
        r.n_keep = n
        _refused("apply", r, match="n_keep")
    for n in (-1, 9):
        r, _ = _valid()
        r.n_arrays = n
        _refused("apply", r, match="n_arrays")
    r, _ = _valid()
    r.arrays = None
    _refused("apply", r, match="n_arrays")
    for field, bad in (("elem_bytes", 1), ("elem_bytes", 8), ("elem_bytes", 0), ("dim", 0), ("dim", -2), ("rule", 3),
                       ("rule", -1), ("src", None), ("dst", None)):
        r, arrays = _valid()
        setattr(arrays[1], field, bad)
        _refused("apply", r, match="arrays[1]")
    r, arrays = _valid()
    arrays[0].dst = arrays[0].src
    _refused("apply", r, match="arrays[0]")
    # more than 2^31 slots: into_slot cannot name them -- the caller's, or the one ZERO / MEAN arrays go by
    for into, n_arrays in ((0x8000, 0), (None, 2), (None, 3)):
        r, _ = _valid(n_arrays)                             # (arrays[0] is KEEP, arrays[1] ZERO, arrays[2] MEAN)
        r.capacity, r.N, r.into_slot = 2 ** 20, 16, into    # 2^32 slots
        r.n_keep = r.capacity
        r.workspace_bytes = _abi.lib().vr_collapse_workspace(16, r.capacity)
        _refused("apply", r, code=UNSUPPORTED, match="into_slot")


# ---- refusals through Python: _args.check, before any C call ----
def _py_valid(tree):
    n_slots = tree.capacity * tree.N ** 3
    return (common.FakeCudaTensor((tree.capacity,), "bool"),
            [(common.FakeCudaTensor((n_slots, tree.data_dim)), "mean"), (common.FakeCudaTensor((n_slots,), "int32"), "zero")])


def test_python_refusals():
    tree = common.FakeTree(info=0)
    cap, n_slots = tree.capacity, tree.capacity * 8
    sel, comps = _py_valid(tree)

    def refused(match, sel=sel, comps=comps, calls=0, **kw):
        t = common.FakeTree(info=0)
        with pytest.raises(ValueError, match=match):
            api.collapse(t, sel, comps, **kw)
        assert t.info_calls <= calls
    refused("sel", sel=common.FakeCudaTensor((cap + 1,), "bool"))
    refused("sel", sel=common.FakeCudaTensor((n_slots,), "bool"))           # per node, not per slot
    refused("sel", sel=common.FakeCudaTensor((cap,), "int32"))              # a bitmap has ceil(capacity / 32) words
    refused("sel", sel=common.FakeCudaTensor(((cap + 31) // 32,), "float32"))
    refused("sel", sel=np.zeros(cap, bool))
    refused("sel", sel=common.FakeCudaTensor((cap,), "bool", contiguous=False))
    refused("sel", sel=common.FakeCudaTensor((cap,), "bool", is_cuda=False))
    refused("sel", sel=common.FakeCudaTensor((cap,), "bool", index=1), calls=1)
    refused(r"companions\[0\]", comps=[(common.FakeCudaTensor((n_slots + 1,)), "keep")])
    refused(r"companions\[0\]", comps=[(common.FakeCudaTensor((n_slots,), "float64"), "keep")])
    refused(r"companions\[0\]", comps=[(common.FakeCudaTensor((n_slots,)), "copy")])
    refused(r"companions\[0\]", comps=[common.FakeCudaTensor((n_slots,))])
    refused(r"companions\[0\]", comps=[(0x9000, "keep")])                     # a raw pointer has no size
    refused(r"companions\[0\]", comps=[(common.FakeCudaTensor((n_slots,), "int32"), "mean")])   # no mean of integers
    refused(r"companions\[1\]", comps=[comps[0], (common.FakeCudaTensor((n_slots,), contiguous=False), "zero")])
    refused(r"companions\[1\]", comps=[comps[0], (common.FakeCudaTensor((n_slots,), index=1), "zero")], calls=1)
    refused("at most 7", comps=[comps[0]] * 8)
    refused("values", values="max")

    class NoHandle:
        @property
        def handle(self):
            raise RuntimeError("tree is not on the device")
    with pytest.raises(RuntimeError, match="not on the device"):
        api.collapse(NoHandle(), None)
    assert api.N3Tree.collapse is api.collapse


# ---- the semantics ----
def test_restatement_on_a_tree_small_enough_to_read():
    # root -> 1 (slot 0), 3 (slot 7); node 1 -> 2 (slot 5); nodes 2 and 3 are frontier nodes
    child = np.array([[1, 0, 0, 0, 0, 0, 0, 3], [0, 0, 0, 0, 0, 1, 0, 0], [0] * 8, [0] * 8], np.int32)
    data = np.arange(32 * 2, dtype=np.float32).reshape(32, 2)
    res = cu.restate(child, [True, True, True, False], [(data, cu.KEEP), (data, cu.ZERO), (data, cu.MEAN)])
    # bit 0 (the root) and bit 1 (not a frontier node) are ignored; node 2 goes into slot 5 of node 1
    assert res["collapsed"].tolist() == [False, False, True, False] and res["n_keep"] == 3
    assert res["src_node"].tolist() == [0, 1, 3] and res["node_map"].tolist() == [0, 1, -1, 2]
    assert res["into_slot"].tolist() == [-1, -1, 13, -1]
    assert res["child_out"].tolist() == [[1, 0, 0, 0, 0, 0, 0, 2], [0] * 8, [0] * 8]
    k, z, m = res["dsts"]
    kept = np.concatenate([data[:16], data[24:]])
    assert np.array_equal(k, kept)
    for d in (z, m):
        assert np.array_equal(np.delete(d, 13, axis=0), np.delete(kept, 13, axis=0))
    assert z[13].tolist() == [0, 0]
    assert m[13].tolist() == [data[16:24, 0].mean(), data[16:24, 1].mean()] == [39.0, 40.0]
    # the root cannot collapse even when it is a frontier node
    lone = cu.restate(np.zeros((1, 8), np.int32), [True], [(data[:8], cu.MEAN)])
    assert lone["n_keep"] == 1 and np.array_equal(lone["dsts"][0], data[:8]) and lone["into_slot"].tolist() == [-1]
    assert cu.pack_bits([True, False, True]).tolist() == [5]
    assert cu.pack_bits(np.ones(33, bool), junk=1, extra_words=1).tolist() == [0xFFFFFFFF] * 3


def test_mean_is_the_sequential_binary32_sum():
    """The order matters: 2^24 + 1 + 1 ... in binary32 stays 2^24 when added one at a time from slot 0."""
    a = np.zeros((16, 1), np.float32)
    a[8], a[9:] = 2.0 ** 24, 1.0
    child = np.zeros((2, 8), np.int32)
    child[0, 3] = 1
    with np.errstate(over="ignore"):
        half = a.astype(np.float16)
    res = cu.restate(child, [False, True], [(a.view(np.uint32), cu.MEAN), (half.view(np.uint16), cu.MEAN)])
    assert res["dsts"][0].view(np.float32)[3, 0] == np.float32(2.0 ** 21)          # not (2^24 + 7) / 8
    assert np.isinf(half[8, 0])                                                    # binary16: inf in, inf out
    assert np.isinf(res["dsts"][1].view(np.float16)[3, 0])


def test_refine_then_collapse_of_the_new_nodes_is_the_identity():
    tree = common.small_scene(depth=4, basis_dim=4, seed=21)
    child, dd, N3, cap = common.rows_of(tree).astype(np.int32), tree.data_dim, 8, tree.capacity
    data = tree.data.reshape(-1, dd).view(np.uint16)
    sel = ru.selections(child, seed=5)["random30"]
    child_r, src_slot, (data_r,) = ru.restate(child, sel, [(data, ru.COPY)])
    assert src_slot.size > 10
    new_nodes = np.arange(child_r.shape[0]) >= cap
    res = cu.restate(child_r, new_nodes, [(data_r, cu.KEEP)])
    assert res["n_keep"] == cap
    assert np.array_equal(res["child_out"], child) and np.array_equal(res["dsts"][0], data)
    assert np.array_equal(res["into_slot"][cap:], src_slot) and (res["into_slot"][:cap] == -1).all()
    assert np.array_equal(res["src_node"], np.arange(cap)) and (res["node_map"][cap:] == -1).all()


def test_collapsing_everything_walks_a_full_tree_up_level_by_level():
    child = ru.full_tree_n2(3).astype(np.int32)
    sizes = [child.shape[0]]
    while child.shape[0] > 1:
        res = cu.restate(child, np.ones(child.shape[0], bool))
        assert res["n_keep"] < child.shape[0]
        child = res["child_out"]
        sizes.append(child.shape[0])
    assert sizes == [585, 73, 9, 1] and not child.any()


@pytest.fixture(scope="module")
def walk_exe(tmp_path_factory):
    return build_util.csrc_program("walk_check", "vr_tree_walk", tmp_path_factory.mktemp("bin"))


TREES = {"general_n4": lambda: common.random_tree_general_n(N=4, depth=3),
         "scene5": lambda: common.small_scene(depth=5, basis_dim=4)}


@pytest.mark.parametrize("name", sorted(TREES))
def test_restated_tree_passes_the_walk_and_the_point_query(walk_exe, tmp_path, name):
    tree = TREES[name]()
    N3, cap, dd = tree.N ** 3, tree.capacity, tree.data_dim
    child = common.rows_of(tree)
    sel = cu.selections(child, seed=3)["random50"]
    new, res = cu.collapsed_synth(tree, sel, cu.MEAN)
    node_map, into_slot, col = res["node_map"].astype(np.int64), res["into_slot"].astype(np.int64), res["collapsed"]
    assert 0 < col.sum() < cu.frontier(child).sum() and new.capacity == cap - col.sum() == res["n_keep"]

    before, after = run_walk(walk_exe, tmp_path, child), run_walk(walk_exe, tmp_path, common.rows_of(new))
    assert isinstance(after, dict), after                                   # (a bad tree gives its `why` text)
    assert np.array_equal(after["level"], before["level"][res["src_node"]])
    assert after["depth"] <= before["depth"]

    pts = np.random.default_rng(5).random((3000, 3), np.float32)
    old = query_util.oracle_query(ob.TreeHandle(tree), pts)
    got = query_util.oracle_query(ob.TreeHandle(new), pts)
    old_node, old_j = old["leaf"] // N3, old["leaf"] % N3
    hit = col[old_node]
    assert 100 < hit.sum() < pts.shape[0] - 100
    # points of kept nodes: the same slot of the renumbered node, the record unchanged
    assert np.array_equal(got["leaf"][~hit], node_map[old_node[~hit]] * N3 + old_j[~hit])
    assert np.array_equal(got["depth"][~hit], old["depth"][~hit])
    rec_old, rec_new = tree.data.reshape(-1, dd).view(np.uint16), new.data.reshape(-1, dd).view(np.uint16)
    assert np.array_equal(rec_new[got["leaf"][~hit]], rec_old[old["leaf"][~hit]])
    # points of collapsed nodes: one level higher, in the merged slot, with the MEAN record of the node
    assert np.array_equal(got["leaf"][hit], into_slot[old_node[hit]])
    assert np.array_equal(got["depth"][hit], old["depth"][hit] - 1)
    means = cu.mean_records(rec_old, old_node[hit], N3)
    assert np.array_equal(rec_new[got["leaf"][hit]], means)
