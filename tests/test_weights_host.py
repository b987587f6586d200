"""vr_accumulate_weights, the part that needs no GPU: the C ABI (symbol, prototype, struct layout) and every
refusal -- through C, C++ and Python.  All of them come before the tree handle is followed and before any
device call, so the calls below pass a tree handle that is never followed (and device pointers that are
never written)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from volrend_amd import _abi, build

INVALID = 1
TREE, BUF = 0x1000, 0x3000   # never dereferenced


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbol_prototype_and_abi_version(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "vr_accumulate_weights" in exported
    res, args = _abi.PROTOTYPES["vr_accumulate_weights"]
    assert res is C.c_int and len(args) == 7
    assert L.vr_accumulate_weights.argtypes == args
    assert L.vr_abi_version() == 3   # additions only


def test_vrleafweights_layout_matches_the_c_compiler():
    st = _abi.VrLeafWeights
    got = build_util.c_struct_layout("VrLeafWeights", st, [("abi", "VR_ABI_VERSION"), ("batch", "VR_MAX_BATCH")])
    assert [f for f, _ in st._fields_] == ["max_weight", "hits"]
    assert got["size"] == C.sizeof(st) == 16
    for fname, _ in st._fields_:
        assert got[fname] == getattr(st, fname).offset, fname
    assert (got["abi"], got["batch"]) == (3, _abi.MAX_BATCH)


def _args(n=1, w=64, h=48):
    cams = (_abi.VrCamera * n)()
    opt = _abi.VrRenderOptions()
    _abi.lib().vr_default_options(C.byref(opt))
    for i in range(n):
        cams[i].width, cams[i].height, cams[i].fx, cams[i].fy = w, h, 50.0, 50.0
    out = _abi.VrLeafWeights()
    out.max_weight, out.hits = BUF, BUF
    return cams, opt, out


def _call(L, n, cams, opt, out, fp_mode=0, tree=TREE):
    rc = L.vr_accumulate_weights(tree, n, cams, None if opt is None else C.byref(opt), fp_mode,
                                 None if out is None else C.byref(out), None)
    return rc, (L.vr_last_error() or b"").decode()


def test_invalid_arguments_through_c(L):
    cams, opt, out = _args(2)
    assert _call(L, 2, cams, opt, out, tree=None)[0] == INVALID
    assert _call(L, 2, None, opt, out)[0] == INVALID
    assert _call(L, 2, cams, None, out)[0] == INVALID
    assert _call(L, 2, cams, opt, None)[0] == INVALID
    assert _call(L, 0, None, None, out)[0] == INVALID           # n_frames == 0 still needs opt ...
    assert _call(L, 0, None, opt, None)[0] == INVALID           # ... and out
    none = _abi.VrLeafWeights()
    rc, msg = _call(L, 2, cams, opt, none)
    assert rc == INVALID and "both outputs" in msg
    assert _call(L, 0, None, opt, none)[0] == INVALID
    for fp in (2, -1, 9):
        rc, msg = _call(L, 2, cams, opt, out, fp_mode=fp)
        assert rc == INVALID and "fp_mode" in msg
    for n in (-1, _abi.MAX_BATCH + 1):
        rc, msg = _call(L, n, cams, opt, out)
        assert rc == INVALID and "n_frames" in msg
    for field, value in (("width", 32), ("height", 40), ("fx", 51.0), ("fy", 49.0)):
        cams, opt, out = _args(3)
        setattr(cams[2], field, value)
        rc, msg = _call(L, 3, cams, opt, out)
        assert rc == INVALID and "frame 2" in msg, field
    # the launch contract of vr_render_batch
    for step in (0.0, -1e-3, float("nan")):
        cams, opt, out = _args(1)
        opt.step_size = step
        rc, msg = _call(L, 1, cams, opt, out)
        assert rc == INVALID and "step_size" in msg
    cams, opt, out = _args(1, w=70000)
    assert _call(L, 1, cams, opt, out)[0] == INVALID
    cams, opt, out = _args(1)
    cams[0].fx = 0.0
    assert _call(L, 1, cams, opt, out)[0] == INVALID


def test_refusals_through_python(L):
    from volrend_amd import api
    cam = api.Camera(64, 48, 50.0, 50.0)
    t = common.FakeTree(handle=TREE, data_dim=None, data_format=None)
    tr = np.zeros(12, np.float32)

    def code(transforms=(tr, tr), opts=None, **kw):
        kw.setdefault("max_weight", BUF)
        with pytest.raises(_abi.VolrendError) as e:
            api.accumulate_weights(t, cam, list(transforms), opts or api.RenderOptions(), **kw)
        return e.value.code

    assert code(fp_mode=5) == INVALID
    assert code(opts=api.RenderOptions(step_size=0.0)) == INVALID
    assert code(max_weight=None, hits=None, want=()) == INVALID          # both outputs NULL
    assert code(transforms=[tr] * (_abi.MAX_BATCH + 1), fp_mode=3) == INVALID
    with pytest.raises(ValueError, match="want"):
        api.accumulate_weights(t, cam, [tr], api.RenderOptions(), want=("weights",))
    with pytest.raises(ValueError, match="want"):
        api.accumulate_weights(t, cam, [tr], api.RenderOptions(), want=("hits", "hits"))


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("weights_refusals", tmp_path), refusals=True)
    for case, word in [("both_null", "both outputs"), ("fp_mode", "fp_mode"), ("step_size", "step_size")]:
        assert got[case].startswith("runtime_error: vr_accumulate_weights:") and word in got[case], (case, got[case])
