"""vr_render_rays, vr_accumulate_weights_rays, vr_render_backward_rays and vr_reserve_rays, the part that needs no
GPU: the C ABI (symbols, prototypes) and every refusal that comes before the tree handle is followed -- through C,
C++ and Python.  The calls below pass a tree handle that is never followed and device pointers that are never
read or written."""
import ctypes as C
import os
import subprocess

import pytest

from tests import build_util, common
from volrend_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5
TREE, O, D, A, G = 0x1000, 0x3000, 0x5000, 0x7000, 0x9000   # never dereferenced
NAMES = ("vr_render_rays", "vr_accumulate_weights_rays", "vr_render_backward_rays")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbols_prototypes_and_abi_version(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "volrend_hip.h")).read()
    for name, n_args in (("vr_render_rays", 7), ("vr_accumulate_weights_rays", 7), ("vr_render_backward_rays", 8),
                         ("vr_reserve_rays", 3)):
        assert name in exported
        res, args = _abi.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n_args and args[1] is C.c_int64
        assert getattr(L, name).argtypes == args
        assert f"int {name}(vr_tree_t tree, int64_t n, " in header
    assert L.vr_abi_version() == 3 and "#define VR_ABI_VERSION 3" in header   # additions only
    assert "typedef struct VrRays" in header and "typedef struct VrRayOut" in header
    assert C.sizeof(_abi.VrRays) == 16 and C.sizeof(_abi.VrRayOut) == 16


def _opt(**kw):
    opt = _abi.VrRenderOptions()
    _abi.lib().vr_default_options(C.byref(opt))
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _call(L, name, n=100, rays=(O, D), opt="default", out=(None, A), fp_mode=0, tree=TREE, g=A, d=G):
    """One call of `name`; rays / opt / out = None pass a NULL pointer -> (rc, message)."""
    r = None
    if rays is not None:
        r = _abi.VrRays()
        r.origins, r.dirs = rays
    o = _opt() if isinstance(opt, str) else opt
    rp, op = (None if r is None else C.byref(r)), (None if o is None else C.byref(o))
    if name == "vr_render_backward_rays":
        rc = L.vr_render_backward_rays(tree, n, rp, op, fp_mode, g, d, None)
    else:
        w = None
        if out is not None:
            w = _abi.VrRayOut() if name == "vr_render_rays" else _abi.VrLeafWeights()
            if name == "vr_render_rays":
                w.rgba, w.accum = out
            else:
                w.hits, w.max_weight = out
        rc = getattr(L, name)(tree, n, rp, op, fp_mode, None if w is None else C.byref(w), None)
    return rc, (L.vr_last_error() or b"").decode()


@pytest.mark.parametrize("name", NAMES)
def test_invalid_arguments_through_c(L, name):
    for kw in (dict(tree=None), dict(rays=None), dict(rays=(None, D)), dict(rays=(O, None)), dict(opt=None)):
        rc, msg = _call(L, name, **kw)
        assert rc == INVALID and "NULL" in msg and name in msg, kw
    if name == "vr_render_backward_rays":
        for kw in (dict(g=None), dict(d=None)):
            rc, msg = _call(L, name, **kw)
            assert rc == INVALID and "NULL" in msg and name in msg, kw
    else:
        rc, msg = _call(L, name, out=None)
        assert rc == INVALID and "NULL" in msg and name in msg
        rc, msg = _call(L, name, out=(None, None))
        assert rc == INVALID and "both outputs" in msg and name in msg
    for fp in (2, -1, 9):
        rc, msg = _call(L, name, fp_mode=fp)
        assert rc == INVALID and "fp_mode" in msg and name in msg
    for n in (-1, 1 << 30, 1 << 40):
        rc, msg = _call(L, name, n=n)
        assert rc == INVALID and "n=" in msg and name in msg
    for step in (0.0, -1e-3, float("nan")):
        for n in (100, 0):       # n == 0 still checks its arguments
            rc, msg = _call(L, name, n=n, opt=_opt(step_size=step))
            assert rc == INVALID and "step_size" in msg
    # n == 0 still needs every pointer
    assert _call(L, name, n=0, rays=(None, D))[0] == INVALID
    assert _call(L, name, n=0, opt=None)[0] == INVALID


def test_an_empty_colour_list_is_ok_without_a_tree(L):
    """vr_render_rays with n == 0 launches nothing and follows nothing (the other two upload their table)."""
    assert _call(L, "vr_render_rays", n=0) == (0, _call(L, "vr_render_rays", n=0)[1])
    assert _call(L, "vr_render_rays", n=0, out=(A, None))[0] == 0


def test_unsupported_options_through_c(L):
    for name in ("vr_render_rays", "vr_render_backward_rays"):
        for field in ("render_depth", "enable_probe"):
            rc, msg = _call(L, name, opt=_opt(**{field: 1}))
            assert rc == UNSUPPORTED and field in msg and name in msg
            assert _call(L, name, n=0, opt=_opt(**{field: 1}))[0] == UNSUPPORTED
    for axis in range(3):
        opt = _opt()
        opt.rot_dirs[axis] = 0.5
        rc, msg = _call(L, "vr_render_backward_rays", opt=opt)
        assert rc == UNSUPPORTED and "rot_dirs" in msg and "vr_render_backward_rays" in msg


def test_reserve_rays_refusals(L):
    assert L.vr_reserve_rays(None, 100, 2) == INVALID and b"vr_reserve_rays" in L.vr_last_error()
    for slots in (0, 9, -1):
        assert L.vr_reserve_rays(TREE, 100, slots) == INVALID and b"n_slots" in L.vr_last_error()
    for n in (-1, 1 << 30):
        assert L.vr_reserve_rays(TREE, n, 2) == INVALID and b"n=" in L.vr_last_error()


def test_refusals_through_python(L):
    torch = pytest.importorskip("torch")
    from volrend_amd import api
    t = common.FakeTree(handle=TREE)
    good = torch.zeros((100, 3), dtype=torch.float32)
    opts = api.RenderOptions()
    calls = {
        "render": lambda o, d, **kw: api.render_rays(t, o, d, opts, **kw),
        "weights": lambda o, d, **kw: api.accumulate_weights_rays(t, o, d, opts, **kw),
        "backward": lambda o, d, **kw: api.render_backward_rays(t, o, d, opts, torch.zeros((100, 4)), **kw),
    }
    for what, call in calls.items():
        def refused(o=good, d=good, match="must", **kw):
            with pytest.raises(ValueError, match=match):
                call(o, d, **kw)
        refused(o=torch.zeros((100, 4)), match="origins")                   # shape
        refused(d=torch.zeros((99, 3)), match="dirs")                       # one ray short
        refused(d=torch.zeros(300), match="dirs")
        refused(o=good.double(), match="float32")
        refused(d=torch.zeros((3, 100)).t(), match="contiguous")
        refused(o=None, match="origins")
        refused(o=[[0.0, 0.0, 0.0]], match="torch tensor")
        refused(o=good, d=good, match="device")                             # host tensors: not on the tree's device
        refused(o=O, d=D, match="pass n")                                   # raw pointers need n
    # outputs and gradients
    with pytest.raises(ValueError, match="want"):
        api.render_rays(t, O, D, opts, want=("depth",), n=100)
    with pytest.raises(ValueError, match="accum"):
        api.render_rays(t, O, D, opts, accum=torch.zeros((100, 3)), n=100)
    with pytest.raises(ValueError, match="uint8"):
        api.render_rays(t, O, D, opts, want=(), rgba=torch.zeros((100, 4)), n=100)
    with pytest.raises(ValueError, match="no output"):
        api.render_rays(t, O, D, opts, want=(), n=100)
    with pytest.raises(ValueError, match="hits"):
        api.accumulate_weights_rays(t, O, D, opts, hits=torch.zeros((10, 2, 2, 2)), n=100)
    with pytest.raises(ValueError, match="grad_accum"):
        api.render_backward_rays(t, O, D, opts, torch.zeros((100, 3)), grad_data=G, n=100)
    with pytest.raises(ValueError, match="grad_accum"):
        api.render_backward_rays(t, O, D, opts, None, grad_data=G, n=100)
    with pytest.raises(ValueError, match="grad_data"):
        api.render_backward_rays(t, O, D, opts, A, grad_data=torch.zeros((10, 2, 2, 2, 48)), n=100)

    # what the C call refuses comes back as VolrendError (raw pointers: nothing is read, refused first)
    def code(fn, *a, **kw):
        with pytest.raises(_abi.VolrendError) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(api.render_rays, t, O, D, opts, accum=A, n=100, fp_mode=5) == INVALID
    assert code(api.render_rays, t, O, D, api.RenderOptions(step_size=0.0), accum=A, n=100) == INVALID
    assert code(api.render_rays, t, O, D, api.RenderOptions(render_depth=True), accum=A, n=100) == UNSUPPORTED
    assert code(api.render_rays, t, O, D, opts, accum=A, n=1 << 30) == INVALID
    assert code(api.accumulate_weights_rays, t, O, D, opts, max_weight=A, want=(), n=100, fp_mode=3) == INVALID
    assert code(api.render_backward_rays, t, O, D, api.RenderOptions(rot_dirs=(0.0, 0.1, 0.0)), A, grad_data=G,
                n=100) == UNSUPPORTED
    assert code(api.render_backward_rays, t, O, D, api.RenderOptions(enable_probe=True), A, grad_data=G,
                n=100) == UNSUPPORTED


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("rays_refusals", tmp_path), refusals=True)
    fn = {"render": "vr_render_rays", "weights": "vr_accumulate_weights_rays", "backward": "vr_render_backward_rays",
          "reserve": "vr_reserve_rays"}
    words = {"null_origins": "NULL", "null_dirs": "NULL", "no_output": "both outputs", "fp_mode": "fp_mode",
             "n_negative": "n=", "n_large": "n=", "step_size": "step_size", "render_depth": "render_depth",
             "enable_probe": "enable_probe", "null_grad_accum": "NULL", "null_grad_data": "NULL",
             "rot_dirs": "rot_dirs", "n_slots": "n_slots", "null_tree": "NULL"}
    assert len(got) == 26
    for case, text in got.items():
        head, rest = case.split("_", 1)
        assert text.startswith(f"runtime_error: {fn[head]}:") and words[rest] in text, (case, text)
