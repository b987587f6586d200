"""vr_render_backward, the part that needs no GPU: the C ABI (symbol, prototype) and every refusal that comes
before the tree handle is followed -- through C, C++ and Python.  The calls below pass a tree handle that is never
followed and device pointers that are never read or written."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from volrend_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5
TREE, G, D = 0x1000, 0x3000, 0x5000   # never dereferenced


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbol_prototype_and_abi_version(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "vr_render_backward" in exported
    res, args = _abi.PROTOTYPES["vr_render_backward"]
    assert res is C.c_int and len(args) == 8
    assert L.vr_render_backward.argtypes == args
    assert L.vr_abi_version() == 3   # additions only
    header = open(os.path.join(ROOT, "include", "volrend_hip.h")).read()
    assert "int vr_render_backward(vr_tree_t tree, int n_frames, const VrCamera* cams, const VrRenderOptions* opt," in header
    assert _abi.VolrendError(UNSUPPORTED, "").code == UNSUPPORTED and "VR_ERR_UNSUPPORTED" in header


def _args(n=1, w=64, h=48):
    cams = (_abi.VrCamera * n)()
    opt = _abi.VrRenderOptions()
    _abi.lib().vr_default_options(C.byref(opt))
    for i in range(n):
        cams[i].width, cams[i].height, cams[i].fx, cams[i].fy = w, h, 50.0, 50.0
    return cams, opt


def _call(L, n, cams, opt, g=G, d=D, fp_mode=0, tree=TREE):
    rc = L.vr_render_backward(tree, n, cams, None if opt is None else C.byref(opt), fp_mode, g, d, None)
    return rc, (L.vr_last_error() or b"").decode()


def test_invalid_arguments_through_c(L):
    cams, opt = _args(2)
    for kw in (dict(tree=None), dict(g=None), dict(d=None)):
        rc, msg = _call(L, 2, cams, opt, **kw)
        assert rc == INVALID and "NULL" in msg, kw
    assert _call(L, 2, None, opt)[0] == INVALID
    assert _call(L, 2, cams, None)[0] == INVALID
    assert _call(L, 0, None, None)[0] == INVALID            # n_frames == 0 still needs opt ...
    assert _call(L, 0, None, opt, g=None)[0] == INVALID     # ... and both buffers
    assert _call(L, 0, None, opt, d=None)[0] == INVALID
    for fp in (2, -1, 9):
        rc, msg = _call(L, 2, cams, opt, fp_mode=fp)
        assert rc == INVALID and "fp_mode" in msg
    for n in (-1, _abi.MAX_BATCH + 1):
        rc, msg = _call(L, n, cams, opt)
        assert rc == INVALID and "n_frames" in msg
    for field, value in (("width", 32), ("height", 40), ("fx", 51.0), ("fy", 49.0)):
        cams, opt = _args(3)
        setattr(cams[2], field, value)
        rc, msg = _call(L, 3, cams, opt)
        assert rc == INVALID and "frame 2" in msg, field
    for step in (0.0, -1e-3, float("nan")):
        cams, opt = _args(1)
        opt.step_size = step
        rc, msg = _call(L, 1, cams, opt)
        assert rc == INVALID and "step_size" in msg
        assert _call(L, 0, None, opt)[0] == INVALID
    cams, opt = _args(1, w=70000)
    assert _call(L, 1, cams, opt)[0] == INVALID
    cams, opt = _args(1)
    cams[0].fx = 0.0
    assert _call(L, 1, cams, opt)[0] == INVALID


def test_unsupported_options_through_c(L):
    """render_depth, enable_probe and rot_dirs need no tree: refused before the handle is followed."""
    for field, value, word in (("render_depth", 1, "render_depth"), ("enable_probe", 1, "enable_probe")):
        cams, opt = _args(1)
        setattr(opt, field, value)
        rc, msg = _call(L, 1, cams, opt)
        assert rc == UNSUPPORTED and word in msg and "vr_render_backward" in msg
    for axis in range(3):
        cams, opt = _args(1)
        opt.rot_dirs[axis] = 0.5
        rc, msg = _call(L, 1, cams, opt)
        assert rc == UNSUPPORTED and "rot_dirs" in msg


def test_refusals_through_python(L):
    torch = pytest.importorskip("torch")
    from volrend_amd import api
    cam = api.Camera(64, 48, 50.0, 50.0)
    t = common.FakeTree(handle=TREE)
    tr = np.zeros(12, np.float32)
    good_g = torch.zeros((2, 48, 64, 4), dtype=torch.float32)
    good_d = torch.zeros((10, 2, 2, 2, 49), dtype=torch.float32)

    def refused(g=good_g, d=good_d, match="must be"):
        with pytest.raises(ValueError, match=match):
            api.render_backward(t, cam, [tr, tr], api.RenderOptions(), g, grad_data=d)

    refused(g=torch.zeros((2, 48, 64, 3)), match="grad_accum")            # shape
    refused(g=torch.zeros((1, 48, 64, 4)), match="grad_accum")            # one frame short
    refused(g=good_g.double(), match="float32")
    refused(g=torch.zeros((2, 48, 4, 64)).permute(0, 1, 3, 2), match="contiguous")
    refused(d=torch.zeros((10, 2, 2, 2, 48)), match="grad_data")
    refused(d=good_d.half(), match="float32")
    refused(d=torch.zeros((10, 2, 2, 49, 2)).transpose(3, 4), match="contiguous")
    refused(g=None, match="grad_accum")
    refused(g=np.zeros((2, 48, 64, 4), np.float32), match="torch tensor")

    # what the C call refuses comes back as VolrendError (raw pointers: nothing is read, refused first)
    def code(opts=None, transforms=(tr, tr), **kw):
        with pytest.raises(_abi.VolrendError) as e:
            api.render_backward(t, cam, list(transforms), opts or api.RenderOptions(), G, grad_data=D, **kw)
        return e.value.code

    assert code(fp_mode=5) == INVALID
    assert code(opts=api.RenderOptions(step_size=0.0)) == INVALID
    assert code(opts=api.RenderOptions(render_depth=True)) == UNSUPPORTED
    assert code(opts=api.RenderOptions(rot_dirs=(0.0, 0.1, 0.0))) == UNSUPPORTED


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("grad_refusals", tmp_path), refusals=True)
    for case, word in [("null_grad_accum", "NULL"), ("null_grad_data", "NULL"), ("fp_mode", "fp_mode"),
                       ("step_size", "step_size"), ("render_depth", "render_depth"), ("rot_dirs", "rot_dirs")]:
        assert got[case].startswith("runtime_error: vr_render_backward:") and word in got[case], (case, got[case])
