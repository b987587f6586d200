"""vr_tree_geometry / vr_slot_points without a GPU: the symbols, prototypes and struct layouts, every refusal of the
header (with pointers that are never followed) through C, C++ and Python, and the semantics as
tests/geometry_util.py restates them: the restatement agrees with an independent top-down walk, and the reference's
point descent finds every restated point of a power-of-two tree in the slot it was made for."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from tests import geometry_util as gu
from volrend_amd import _abi, api, synth

FUNCS = ("vr_tree_geometry", "vr_slot_points")
INVALID, UNSUPPORTED = 1, 5


def test_symbols_are_exported_and_prototyped():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for f in FUNCS:
        assert f in exported and f in _abi.PROTOTYPES, f
    assert _abi.lib().vr_abi_version() == 3                       # additive: the version stands
    assert (_abi.GEOM_MAX_DEPTH, _abi.POINTS_MAX_K, _abi.POINTS_CENTER, _abi.POINTS_JITTER) == (64, 64, 0, 1)
    assert api.N3Tree.geometry is api.geometry and api.N3Tree.slot_points is api.slot_points
    assert api.N3Tree.parent_depth is api.parent_depth


def test_struct_layouts_match_the_c_compiler():
    extra = [("max_depth", "VR_GEOM_MAX_DEPTH"), ("max_k", "VR_POINTS_MAX_K"), ("center", "VR_POINTS_CENTER"),
             ("jitter", "VR_POINTS_JITTER")]
    for name, st in (("VrGeometry", _abi.VrGeometry), ("VrSlotPoints", _abi.VrSlotPoints)):
        got = build_util.c_struct_layout(name, st, extra)
        assert got["size"] == C.sizeof(st), name
        for fname, _ in st._fields_:
            assert got[fname] == getattr(st, fname).offset, f"{name}.{fname}"
        assert [got[k] for k, _ in extra] == [64, 64, 0, 1]


# ---- refusals through C: every pointer is junk and must never be followed ----
def _geometry(**kw):
    g = _abi.VrGeometry()
    g.child, g.parent_slot, g.node_depth, g.node_origin, g.capacity, g.N = 0x1000, 0x2000, 0x3000, 0x4000, 10, 2
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _points(**kw):
    p = _abi.VrSlotPoints()
    p.node_depth, p.node_origin, p.slots, p.points, p.depth, p.side = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    p.capacity, p.n, p.N, p.k, p.mode, p.seed = 10, 100, 2, 3, 1, 7
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _refused(name, arg, code=INVALID, match=None):
    L = _abi.lib()
    rc = getattr(L, name)(None if arg is None else C.byref(arg), None)
    msg = L.vr_last_error().decode()
    assert rc == code and name in msg, (rc, msg)
    assert match is None or match in msg, msg


def test_c_refusals_of_geometry():
    name = "vr_tree_geometry"
    _refused(name, None, match="NULL")
    _refused(name, _geometry(child=None), match="NULL")
    _refused(name, _geometry(parent_slot=None, node_depth=None, node_origin=None), match="output")
    for N in (-1, 0, 1, 17):
        _refused(name, _geometry(N=N), match="N=")
    for cap in (0, -1, 2 ** 31):
        _refused(name, _geometry(capacity=cap), match="capacity")
    _refused(name, _geometry(capacity=2 ** 31 - 1), code=UNSUPPORTED, match="int32")      # 2^34 slots


def test_c_refusals_of_slot_points():
    name = "vr_slot_points"
    _refused(name, None, match="NULL")
    for field in ("node_depth", "node_origin", "slots"):
        _refused(name, _points(**{field: None}), match="NULL")
    _refused(name, _points(points=None, depth=None, side=None), match="output")
    for N in (-1, 0, 1, 17):
        _refused(name, _points(N=N), match="N=")
    for cap in (0, -1, 2 ** 31):
        _refused(name, _points(capacity=cap), match="capacity")
    for n in (-1, 2 ** 31):
        _refused(name, _points(n=n), match="n=")
    for k in (0, -1, 65):
        _refused(name, _points(k=k), match="k=")
    for mode in (-1, 2):
        _refused(name, _points(mode=mode), match="mode")
    _refused(name, _points(capacity=2 ** 31 - 1), code=UNSUPPORTED, match="int32")
    # n == 0 still checks its arguments -- and then reads no array and launches nothing
    _refused(name, _points(n=0, k=0), match="k=")
    _refused(name, _points(n=0, points=None, depth=None, side=None), match="output")
    p = _points(n=0, slots=None, node_depth=None, node_origin=None)
    assert _abi.lib().vr_slot_points(C.byref(p), None) == 0


def test_refusals_through_cpp(tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("geometry_refusals", tmp_path), refusals=True)
    geometry = {"null_child": "NULL", "no_output": "output", "n_small": "N=", "n_large": "N=",
                "capacity_zero": "capacity", "capacity_large": "capacity", "too_many_slots": "int32"}
    points = {"null_slots": "NULL", "null_node_depth": "NULL", "null_node_origin": "NULL", "no_output": "output",
              "n_negative": "n=", "n_large": "n=", "k_zero": "k=", "k_large": "k=", "mode": "mode", "N": "N=",
              "capacity": "capacity"}
    assert got.pop("points.n_zero") == "OK"
    want = {**{"geometry." + k: ("vr_tree_geometry", v) for k, v in geometry.items()},
            **{"points." + k: ("vr_slot_points", v) for k, v in points.items()}}
    assert sorted(got) == sorted(want)
    for case, text in got.items():
        assert text.startswith(f"runtime_error: {want[case][0]}:") and want[case][1] in text, (case, text)


# ---- refusals through Python: _args.check, before any C call ----
def test_python_refusals():
    cap = 10
    slots = common.FakeCudaTensor((100,), "int32")
    geo = {"node_depth": common.FakeCudaTensor((cap,), "int32"), "node_origin": common.FakeCudaTensor((cap, 3), "int32")}

    def refused(match, calls=0, **kw):
        t = common.FakeTree(info=0)
        args = dict(slots=slots, geometry=geo)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            api.slot_points(t, args.pop("slots"), **args)
        assert t.info_calls <= calls
    refused("slots", slots=common.FakeCudaTensor((100,), "int64"))
    refused("slots", slots=common.FakeCudaTensor((100, 1), "int32"))
    refused("slots", slots=np.zeros(100, np.int32))
    refused("slots", slots=common.FakeCudaTensor((100,), "int32", contiguous=False))
    refused("slots", slots=common.FakeCudaTensor((100,), "int32", is_cuda=False))
    refused("slots", slots=common.FakeCudaTensor((100,), "int32", index=1), calls=1)
    refused("slots", slots=0x9000)                                            # a raw pointer has no length
    for k in (0, 65, 2.0, True):
        refused("k must", k=k)
    refused("mode", mode="centre")
    for seed in (-1, 2 ** 32, 1.5):
        refused("seed", seed=seed)
    refused("space", space="local")
    refused("geometry", geometry={"node_depth": geo["node_depth"]})
    refused("geometry", geometry=(geo["node_depth"], geo["node_origin"]))
    refused("node_depth", geometry=dict(geo, node_depth=common.FakeCudaTensor((cap + 1,), "int32")))
    refused("node_origin", geometry=dict(geo, node_origin=common.FakeCudaTensor((cap, 3), "float32")))
    refused("node_origin", geometry=dict(geo, node_origin=common.FakeCudaTensor((cap * 3,), "int32")))
    for want in ((), ("depth",), ("node_depth", "node_depth"), "origin"):
        with pytest.raises(ValueError, match="want"):
            api.geometry(common.FakeTree(), want)

    class NoHandle:
        @property
        def handle(self):
            raise RuntimeError("tree is not on the device")
    for call in (lambda t: api.geometry(t), lambda t: api.slot_points(t, None), lambda t: api.parent_depth(t)):
        with pytest.raises(RuntimeError, match="not on the device"):
            call(NoHandle())


# ---- the semantics ----
def test_restatement_on_a_tree_small_enough_to_read():
    child = np.array([[0, 0, 0, 0, 0, 0, 2, 0], [0] * 8, [0, 0, 0, -1, 0, 0, 0, 0], [0] * 8], np.int32)
    parent, depth, origin = gu.restate(child)                   # root -(slot 6)-> 2 -(slot 3)-> 1; 3 is an orphan
    assert parent.tolist() == [-1, 2 * 8 + 3, 6, -1] and depth.tolist() == [0, 2, 1, -1]
    assert origin.tolist() == [[0, 0, 0], [2, 3, 1], [1, 1, 0], [0, 0, 0]]           # 6 = (1, 1, 0), 3 = (0, 1, 1)
    pts, d, side = gu.points(depth, origin, 2, [1 * 8 + 5, 7, 3 * 8, 32, -1])
    assert d.tolist() == [2, 0, -1, -1, -1] and side[:2].tolist() == [0.125, 0.5] and np.isnan(side[2:]).all()
    assert pts[0, 0].tolist() == [(2 * 2 + 1 + .5) / 8, (3 * 2 + 0 + .5) / 8, (1 * 2 + 1 + .5) / 8]
    assert pts[1, 0].tolist() == [.75, .75, .75] and np.isnan(pts[2:]).all()
    jit = gu.points(depth, origin, 2, [13, 7], k=4, mode=gu.JITTER, seed=9)[0]
    lo = np.array([[5, 6, 3], [1, 1, 1]])[:, None, :] / np.array([8, 2])[:, None, None]
    assert ((jit >= lo) & (jit < lo + np.array([.125, .5])[:, None, None])).all() and np.unique(jit).size == 24
    # toward zero: (2^25 + 2.5) / 2^26 is 0.625 ulp above 0.5; the cast to nearest goes up, the rule goes down
    o = np.array([[2 ** 24 + 1, 0, 0]], np.uint32)
    p = gu.points(np.array([25], np.int32), o, 2, [0])[0][0, 0, 0]
    assert p == np.float32(0.5) and np.float32((2 ** 25 + 2.5) / 2 ** 26) > p


@pytest.mark.parametrize("name", sorted(gu.TREES))
def test_restatement_agrees_with_a_top_down_walk(name):
    child = gu.TREES[name]()
    parent, depth, origin = gu.restate(child)
    seen = gu.walk_down(child)
    for m in range(child.shape[0]):
        if m in seen and seen[m][1] <= gu.MAX_DEPTH:
            assert (int(parent[m]), int(depth[m]), tuple(int(v) for v in origin[m])) == seen[m], m
        elif m in seen:                         # deeper than 64 links: no depth, but the link into it is known
            assert depth[m] == -1 and parent[m] == seen[m][0], m
        else:                                   # what the walk from the root never reaches: an orphan
            assert depth[m] == -1 and parent[m] == -1, m
    too_deep = sum(d > gu.MAX_DEPTH for _, d, _ in seen.values())
    assert (depth == -1).sum() == too_deep + child.shape[0] - len(seen)
    assert too_deep == (5 if name == "chain_n2_70" else 0) and parent[0] == -1 and depth[0] == 0


def _guarantee_trees():
    for name in gu.POWER_OF_TWO:
        yield name, gu.TREES[name]()
    yield "scene_n2_depth6", common.rows_of(common.small_scene(depth=6, basis_dim=4, seed=31)).astype(np.int32)
    yield "general_n4", common.rows_of(common.random_tree_general_n(N=4, depth=3, seed=8)).astype(np.int32)


def test_the_descent_finds_every_restated_point_in_its_slot():
    """The in-cell guarantee of the header, from the restatement alone, for every tree the GPU test holds against
    vr_query_points: N a power of two, N^L <= 2^24, and no cell so small that the clamp at 1 - 1e-6f leaves it."""
    for name, child in _guarantee_trees():
        N = gu.branching(child)
        _, depth, origin = gu.restate(child)
        assert N in (2, 4) and float(N) ** (depth.max() + 1) <= 2 ** 24, name
        leaves = gu.reachable_leaves(child, depth)
        for mode, k in ((gu.CENTER, 1), (gu.JITTER, 5)):
            pts, d, side = gu.points(depth, origin, N, leaves, k=k, mode=mode, seed=11)
            assert side.min() > 1e-6, name
            slot, found_depth = gu.descend(child, pts.reshape(-1, 3))
            assert np.array_equal(slot.reshape(-1, k), np.repeat(leaves[:, None], k, 1)), (name, mode)
            assert np.array_equal(found_depth.reshape(-1, k), np.repeat(d[:, None], k, 1)), (name, mode)


def test_save_npz_takes_parent_depth(tmp_path):
    tree = common.small_scene(depth=3, basis_dim=1, seed=2)
    parent, depth, _ = gu.restate(common.rows_of(tree))
    pd = np.stack([parent, depth], axis=1)
    pd[0, 0] = 0
    a, b, c = (str(tmp_path / f"{x}.npz") for x in "abc")
    synth.save_npz(tree, a)
    synth.save_npz(tree, b, parent_depth=np.zeros((tree.capacity, 2), np.int32))
    synth.save_npz(tree, c, parent_depth=pd)
    assert open(a, "rb").read() == open(b, "rb").read()
    za, zc = np.load(a), np.load(c)
    assert sorted(za.files) == sorted(zc.files) and not za["parent_depth"].any()
    for key in za.files:
        want = pd if key == "parent_depth" else za[key]
        assert zc[key].dtype == za[key].dtype and np.array_equal(zc[key], want), key
