"""vr_refine_plan / vr_refine_apply without a GPU: the symbols, prototypes and struct layouts, every refusal of the
header (with pointers that are never followed) through C and through Python, and the semantics as
tests/refine_util.py restates them: a restated tree passes the upload's host walk, and the oracle's point query
finds, inside refined leaves, the old record one level deeper."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from tests import build_util, common, query_util
from tests import refine_util as ru
from tests.test_tree_walk import run_walk
from volrend_amd import _abi, api

FUNCS = ("vr_refine_workspace", "vr_refine_plan", "vr_refine_apply")
INVALID, UNSUPPORTED = 1, 5


def test_symbols_are_exported_and_prototyped():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for f in FUNCS:
        assert f in exported and f in _abi.PROTOTYPES, f
    L = _abi.lib()
    assert L.vr_abi_version() == 3                       # additive: the version stands
    assert _abi.REFINE_MAX_ARRAYS == 8 and (_abi.REFINE_COPY, _abi.REFINE_ZERO) == (0, 1)


def test_struct_layouts_match_the_c_compiler():
    for name, st in (("VrRefine", _abi.VrRefine), ("VrRefineArray", _abi.VrRefineArray)):
        got = build_util.c_struct_layout(name, st, [("max", "VR_REFINE_MAX_ARRAYS"), ("copy", "VR_REFINE_COPY"),
                                                    ("zero", "VR_REFINE_ZERO")])
        assert got["size"] == C.sizeof(st), name
        for fname, _ in st._fields_:
            assert got[fname] == getattr(st, fname).offset, f"{name}.{fname}"
        assert (got["max"], got["copy"], got["zero"]) == (8, 0, 1)


def test_workspace_rule():
    L = _abi.lib()
    assert L.vr_refine_workspace(2, 1) > 0
    sizes = [L.vr_refine_workspace(2, c) for c in (1, 10, 1000, 10 ** 6, 2 ** 31 - 1)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # mask words, two 64-bit words per mask word, the scan's storage: about 21 bytes per 32 slots
    assert 20 * (8 * 10 ** 6 // 32) <= sizes[3] <= 22 * (8 * 10 ** 6 // 32) + (1 << 17)
    for N, cap in ((1, 10), (17, 10), (2, 0), (2, -4), (2, 2 ** 31)):
        assert L.vr_refine_workspace(N, cap) == -1


# ---- refusals through C: every pointer is junk and must never be followed ----
def _valid(n_arrays=2):
    L = _abi.lib()
    arrays = (_abi.VrRefineArray * 8)()
    for i in range(8):
        arrays[i].src, arrays[i].dst = 0x10000 + 0x2000 * i, 0x11000 + 0x2000 * i
        arrays[i].elem_bytes, arrays[i].dim, arrays[i].fill = (2, 4)[i % 2], 1 + 7 * i, i % 2
    r = _abi.VrRefine()
    r.child, r.sel, r.child_out, r.src_slot, r.workspace = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    r.arrays, r.n_arrays = arrays, n_arrays
    r.capacity, r.N, r.n_new = 10, 2, 3
    r.workspace_bytes = L.vr_refine_workspace(2, 10)
    return r, arrays


def _refused(call, r, code=INVALID, match=None):
    L = _abi.lib()
    n_new = C.c_int64(-7)
    rc = L.vr_refine_plan(C.byref(r), C.byref(n_new), None) if call == "plan" else L.vr_refine_apply(C.byref(r), None)
    msg = L.vr_last_error().decode()
    assert rc == code and f"vr_refine_{call}" in msg, (rc, msg)
    assert match is None or match in msg, msg


@pytest.mark.parametrize("call", ["plan", "apply"])
def test_c_refusals_common_to_both_calls(call):
    L = _abi.lib()
    n_new = C.c_int64(0)
    assert (L.vr_refine_plan(None, C.byref(n_new), None) if call == "plan" else L.vr_refine_apply(None, None)) == INVALID
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
    assert _abi.lib().vr_refine_plan(C.byref(r), None, None) == INVALID


def test_c_refusals_of_apply():
    r, _ = _valid()
    r.child_out = None
    _refused("apply", r, match="child_out")
    r, _ = _valid()
    r.child_out = r.child
    _refused("apply", r, match="child_out")
    r, _ = _valid()
    r.n_new = -1
    _refused("apply", r, match="n_new")
    for n in (-1, 9):
        r, _ = _valid()
        r.n_arrays = n
        _refused("apply", r, match="n_arrays")
    r, _ = _valid()
    r.arrays = None
    _refused("apply", r, match="n_arrays")
    for field, bad in (("elem_bytes", 1), ("elem_bytes", 8), ("elem_bytes", 0), ("dim", 0), ("dim", -2), ("fill", 2),
                       ("fill", -1), ("src", None), ("dst", None)):
        r, arrays = _valid()
        setattr(arrays[1], field, bad)
        _refused("apply", r, match="arrays[1]")
    r, arrays = _valid()
    arrays[0].dst = arrays[0].src
    _refused("apply", r, match="arrays[0]")
    r, _ = _valid()
    r.capacity, r.n_new = 2 ** 31 - 10, 10             # capacity + n_new > INT32_MAX
    r.workspace_bytes = _abi.lib().vr_refine_workspace(2, r.capacity)
    _refused("apply", r, code=UNSUPPORTED, match="int32")


# ---- refusals through Python: _args.check, before any C call ----
def _py_valid(tree):
    n_slots = tree.capacity * tree.N ** 3
    return (common.FakeCudaTensor((n_slots,), "bool"),
            [(common.FakeCudaTensor((n_slots, tree.data_dim)), "copy"), (common.FakeCudaTensor((n_slots,), "int32"), "zero")])


def test_python_refusals():
    tree = common.FakeTree(info=0)
    n_slots = tree.capacity * 8
    sel, comps = _py_valid(tree)

    def refused(match, sel=sel, comps=comps, calls=0):
        t = common.FakeTree(info=0)
        with pytest.raises(ValueError, match=match):
            api.refine(t, sel, comps)
        assert t.info_calls <= calls
    refused("sel", sel=common.FakeCudaTensor((n_slots + 1,), "bool"))
    refused("sel", sel=common.FakeCudaTensor((n_slots,), "int32"))          # a bitmap has ceil(n / 32) words
    refused("sel", sel=common.FakeCudaTensor(((n_slots + 31) // 32,), "float32"))
    refused("sel", sel=np.zeros(n_slots, bool))
    refused("sel", sel=common.FakeCudaTensor((n_slots,), "bool", contiguous=False))
    refused("sel", sel=common.FakeCudaTensor((n_slots,), "bool", is_cuda=False))
    refused("sel", sel=common.FakeCudaTensor((n_slots,), "bool", index=1), calls=1)
    refused(r"companions\[0\]", comps=[(common.FakeCudaTensor((n_slots + 1,)), "copy")])
    refused(r"companions\[0\]", comps=[(common.FakeCudaTensor((n_slots,), "float64"), "copy")])
    refused(r"companions\[0\]", comps=[(common.FakeCudaTensor((n_slots,)), "fill")])
    refused(r"companions\[0\]", comps=[common.FakeCudaTensor((n_slots,))])
    refused(r"companions\[0\]", comps=[(0x9000, "copy")])                     # a raw pointer has no size
    refused(r"companions\[1\]", comps=[comps[0], (common.FakeCudaTensor((n_slots,), contiguous=False), "zero")])
    refused(r"companions\[1\]", comps=[comps[0], (common.FakeCudaTensor((n_slots,), index=1), "zero")], calls=1)
    refused("at most 7", comps=[comps[0]] * 8)

    class NoHandle:
        @property
        def handle(self):
            raise RuntimeError("tree is not on the device")
    with pytest.raises(RuntimeError, match="not on the device"):
        api.refine(NoHandle(), None)
    assert api.N3Tree.refine is api.refine


def test_from_device_arrays_refusals():
    f = api.N3Tree.from_device_arrays
    args = (np.zeros(3), np.ones(3), "SH1")
    child, data = common.FakeCudaTensor((5, 2, 2, 2), "int32"), common.FakeCudaTensor((5, 2, 2, 2, 4), "float16")
    with pytest.raises(ValueError, match="child_dev"):
        f(common.FakeCudaTensor((5, 8), "int32"), data, *args)
    with pytest.raises(ValueError, match="data_dev"):
        f(child, common.FakeCudaTensor((5, 8, 4), "float16"), *args)
    with pytest.raises(ValueError, match="data_dev"):
        f(child, common.FakeCudaTensor((6, 2, 2, 2, 4), "float16"), *args)
    with pytest.raises(ValueError, match="child_dev"):
        f(common.FakeCudaTensor((5, 2, 2, 2), "int64"), data, *args)
    with pytest.raises(ValueError, match="data_dev"):
        f(child, common.FakeCudaTensor((5, 2, 2, 2, 4), "float32"), *args)
    with pytest.raises(ValueError, match="data_dev"):
        f(child, common.FakeCudaTensor((5, 2, 2, 2, 4), "float16", is_cuda=False), *args)


# ---- the semantics ----
def test_restatement_on_a_tree_small_enough_to_read():
    child = np.array([[1, 0, 0, 0, 0, 0, 0, 2], [0] * 8, [0] * 8], np.int32)     # root -> 1 (slot 0), 2 (slot 7)
    sel = np.zeros(24, bool)
    sel[[0, 2, 9, 23]] = True                                                   # slot 0 is internal: ignored
    data = np.arange(24 * 2, dtype=np.float32).reshape(24, 2)
    out, src_slot, (d, z) = ru.restate(child, sel, [(data, ru.COPY), (data, ru.ZERO)])
    assert src_slot.tolist() == [2, 9, 23] and out.shape == (6, 8)
    assert out[0].tolist() == [1, 0, 3, 0, 0, 0, 0, 2] and out[1, 1] == 4 - 1 and out[2, 7] == 5 - 2
    assert not out[3:].any() and np.count_nonzero(out) == 5
    assert np.array_equal(d[:24], data) and np.array_equal(z[:24], data) and not z[24:].any()
    assert np.array_equal(d[24:32], np.tile(data[2], (8, 1))) and np.array_equal(d[40:], np.tile(data[23], (8, 1)))
    assert ru.pack_bits(sel).tolist() == [(1 << 0) | (1 << 2) | (1 << 9) | (1 << 23)]
    assert ru.pack_bits(np.ones(33, bool), junk=1).tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    assert ru.pack_bits(np.ones(33, bool)).tolist() == [0xFFFFFFFF, 1]


@pytest.fixture(scope="module")
def walk_exe(tmp_path_factory):
    return build_util.csrc_program("walk_check", "vr_tree_walk", tmp_path_factory.mktemp("bin"))


TREES = {"general_n4": lambda: common.random_tree_general_n(N=4, depth=3),
         "scene5": lambda: common.small_scene(depth=5, basis_dim=4)}


@pytest.mark.parametrize("name", sorted(TREES))
def test_restated_tree_passes_the_walk_and_the_point_query(walk_exe, tmp_path, name):
    tree = TREES[name]()
    N3, cap = tree.N ** 3, tree.capacity
    child = common.rows_of(tree)
    sel = ru.selections(child, seed=3)["random30"]
    new, src_slot = ru.refined_synth(tree, sel)
    n_new = src_slot.size
    assert 0 < n_new < (child == 0).sum() and new.capacity == cap + n_new

    before, after = run_walk(walk_exe, tmp_path, child), run_walk(walk_exe, tmp_path, common.rows_of(new))
    assert isinstance(after, dict), after                                   # (a bad tree gives its `why` text)
    refined_level = before["level"][src_slot // N3]
    assert np.array_equal(after["level"][:cap], before["level"])
    assert np.array_equal(after["level"][cap:], refined_level + 1)
    assert after["depth"] == max(before["depth"], int(refined_level.max()) + 1)

    pts = np.random.default_rng(5).random((3000, 3), np.float32)
    old = query_util.oracle_query(ob.TreeHandle(tree), pts)
    got = query_util.oracle_query(ob.TreeHandle(new), pts)
    hit = np.isin(old["leaf"], src_slot)
    assert 100 < hit.sum() < pts.shape[0] - 100
    assert np.array_equal(got["leaf"][~hit], old["leaf"][~hit]) and np.array_equal(got["depth"][~hit], old["depth"][~hit])
    assert np.array_equal(got["depth"][hit], old["depth"][hit] + 1)
    assert (got["leaf"][hit] >= cap * N3).all()
    rank = np.searchsorted(src_slot, old["leaf"][hit])
    assert np.array_equal((got["leaf"][hit] // N3) - cap, rank)             # the r-th refined slot is node capacity + r
    rec_old, rec_new = tree.data.reshape(-1, tree.data_dim), new.data.reshape(-1, new.data_dim)
    assert np.array_equal(rec_new[got["leaf"][hit]].view(np.uint16), rec_old[old["leaf"][hit]].view(np.uint16))
