"""Bulk point queries (vr_query_points / vr_query_grid), the part that needs no GPU:
(a) the C ABI -- symbols, ctypes prototypes, the layout of VrQueryOut, the argument checks that
    come before any device call;
(b) the yardstick of the colour tests: the colour of a sample recomposed from the oracle's own
    pieces (tests/query_util.recompose_rgb) is pinned to or_render on scenes whose first sample is
    opaque, so that or_render's accumulator IS the colour of one sample along the pixel's view
    direction.  (b) validates the yardstick, not the feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import build_util, common, query_util as qu
from tests.common import ob
from volrend_amd import _abi, build


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_query_symbols_and_prototypes(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("vr_query_points", "vr_query_grid"):
        assert name in exported
        assert name in _abi.PROTOTYPES and _abi.PROTOTYPES[name][0] is C.c_int
        assert getattr(L, name).argtypes == _abi.PROTOTYPES[name][1]
    assert len(_abi.PROTOTYPES["vr_query_points"][1]) == 7
    assert len(_abi.PROTOTYPES["vr_query_grid"][1]) == 8
    assert (_abi.SPACE_WORLD, _abi.SPACE_TREE) == (0, 1)
    assert L.vr_abi_version() == 3   # additions only


def test_query_out_layout_matches_the_c_compiler():
    st = _abi.VrQueryOut
    got = build_util.c_struct_layout("VrQueryOut", st, [("world", "VR_SPACE_WORLD"), ("tree", "VR_SPACE_TREE")])
    assert [f for f, _ in st._fields_] == ["sigma", "depth", "local", "coeffs", "rgb"]
    assert got["size"] == C.sizeof(st)
    for fname, _ in st._fields_:
        assert got[fname] == getattr(st, fname).offset, fname
    assert (got["world"], got["tree"]) == (_abi.SPACE_WORLD, _abi.SPACE_TREE)


def test_query_argument_checks_need_no_device(L):
    """A NULL tree is refused first, whatever else is passed, and never dereferenced."""
    out = _abi.VrQueryOut()
    out.sigma = 0x1000   # never written: the calls fail before any device call
    f3, i3 = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4)
    assert L.vr_query_points(None, 8, 0x1000, None, _abi.SPACE_WORLD, C.byref(out), None) == 1
    assert b"tree is NULL" in L.vr_last_error()
    assert L.vr_query_points(None, 0, None, None, 7, None, None) == 1
    assert L.vr_query_points(None, -1, 0x1000, None, _abi.SPACE_TREE, C.byref(out), None) == 1
    assert L.vr_query_grid(None, C.byref(f3), C.byref(f3), C.byref(i3), None, 0, C.byref(out), None) == 1
    assert b"tree is NULL" in L.vr_last_error()
    assert L.vr_query_grid(None, None, None, None, None, 0, None, None) == 1


def test_python_wrappers_refuse_before_any_c_call():
    """N3Tree.query / query_grid on a tree that is not on the device: no C call is made."""
    from volrend_amd import api
    t = api.N3Tree.from_synth(common.small_scene(depth=2, basis_dim=4, seed=1), upload=False)
    with pytest.raises(RuntimeError, match="not on the device"):
        t.query(0x1000, n=4)
    with pytest.raises(RuntimeError, match="not on the device"):
        t.query_grid((0, 0, 0), (1, 1, 1), (2, 2, 2))


# ---- (b) the colour yardstick ------------------------------------------------------------------
@pytest.mark.parametrize("fmt,basis_dim", [("SH", 1), ("SH", 4), ("SH", 9), ("SH", 16), ("SH", 25), ("RGBA", 0)],
                         ids=["SH1", "SH4", "SH9", "SH16", "SH25", "RGBA"])
def test_recomposed_colour_equals_or_render_on_one_sample_scenes(fmt, basis_dim):
    tree = qu.one_sample_tree(basis_dim, fmt, seed=40 + basis_dim)
    tr, w, h, f = common.axis_camera(size=33, focal=40.0, dist=4.0)
    _, acc, cnt = common.oracle_frame(tree, tr, w, h, f, ob.FP_STRICT)
    assert (acc[..., 3] == 1.0).all() and cnt["rays_hit_box"] == w * h, "every pixel must be a hit"
    th = ob.TreeHandle(tree)
    dirs = qu.pixel_dirs(w, h, f, f).reshape(-1, 3)
    rec = qu.records(tree)[0, :-1]
    rgb = qu.recompose_rgb(tree, th, np.broadcast_to(rec, (w * h, rec.size)), dirs)
    want = np.ascontiguousarray(acc[..., :3]).reshape(-1, 3)
    assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32)), \
        f"{int((rgb.view(np.uint32) != want.view(np.uint32)).any(-1).sum())} of {w * h} pixels differ"


def test_point_sets_meet_their_conditions_on_the_oracle():
    """The seeds the GPU tests use, checked where no GPU is needed (tests/query_util.POINT_TREES; tests/test_gpu_query.py
    repeats the check on the oracle's answers before it looks at the kernel)."""
    for name in qu.POINT_TREES:
        tree, pts = qu.make_point_tree(name, n=20000)
        th = ob.TreeHandle(tree)
        ans = qu.oracle_answers(tree, th, pts, "tree")
        qu.check_point_set(tree, ans, name)
