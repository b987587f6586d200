"""vr_fit_rays, the part that needs no GPU: the C ABI (symbol, prototype, the layout of VrFit) and every refusal that
comes before the tree handle is followed -- through C, C++ and Python.  The calls below pass a tree handle that is
never followed and device pointers that are never read or written."""
import ctypes as C
import os
import subprocess

import pytest

from tests import build_util, common
from volrend_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 5
TREE, O, D, T, G, B, S, A = 0x1000, 0x3000, 0x5000, 0x7000, 0x9000, 0xB000, 0xD000, 0xF000   # never dereferenced
NAME = "vr_fit_rays"


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbol_prototype_and_abi_version(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "volrend_hip.h")).read()
    assert NAME in exported
    res, args = _abi.PROTOTYPES[NAME]
    assert res is C.c_int and len(args) == 7 and args[1] is C.c_int64
    assert args[2] is C.POINTER(_abi.VrRays) and args[5] is C.POINTER(_abi.VrFit)
    assert getattr(L, NAME).argtypes == args
    assert f"int {NAME}(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt,\n" in header
    assert L.vr_abi_version() == 3 and "#define VR_ABI_VERSION 3" in header   # additions only
    assert "typedef struct VrFit" in header


def test_vrfit_layout_is_the_c_compilers():
    got = build_util.c_struct_layout("VrFit", _abi.VrFit)
    assert got.pop("size") == C.sizeof(_abi.VrFit) == 48
    assert got == {f: getattr(_abi.VrFit, f).offset for f, _ in _abi.VrFit._fields_}
    assert [f for f, _ in _abi.VrFit._fields_] == ["target", "grad_scale", "grad_data", "touched", "sq_err", "accum"]


def _opt(**kw):
    opt = _abi.VrRenderOptions()
    _abi.lib().vr_default_options(C.byref(opt))
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _call(L, n=100, rays=(O, D), opt="default", fit="default", fp_mode=0, tree=TREE, **fields):
    """One call; rays / opt / fit = None pass a NULL pointer; ``fields`` overwrite those of VrFit -> (rc, message)."""
    r = None
    if rays is not None:
        r = _abi.VrRays()
        r.origins, r.dirs = rays
    o = _opt() if isinstance(opt, str) else opt
    f = None
    if fit is not None:
        f = _abi.VrFit()
        f.target, f.grad_scale, f.grad_data, f.touched, f.sq_err, f.accum = T, 0.5, G, B, S, A
        for k, v in fields.items():
            setattr(f, k, v)
    ptr = lambda x: None if x is None else C.byref(x)   # noqa: E731
    rc = L.vr_fit_rays(tree, n, ptr(r), ptr(o), fp_mode, ptr(f), None)
    return rc, (L.vr_last_error() or b"").decode()


def test_invalid_arguments_through_c(L):
    for kw in (dict(tree=None), dict(rays=None), dict(rays=(None, D)), dict(rays=(O, None)), dict(opt=None),
               dict(fit=None), dict(target=None), dict(grad_data=None)):
        rc, msg = _call(L, **kw)
        assert rc == INVALID and "NULL" in msg and NAME in msg, kw
    for fp in (2, -1, 9):
        rc, msg = _call(L, fp_mode=fp)
        assert rc == INVALID and "fp_mode" in msg and NAME in msg
    for n in (-1, 1 << 30, 1 << 40):
        rc, msg = _call(L, n=n)
        assert rc == INVALID and "n=" in msg and NAME in msg
    for step in (0.0, -1e-3, float("nan")):
        for n in (100, 0):       # n == 0 still checks its arguments
            rc, msg = _call(L, n=n, opt=_opt(step_size=step))
            assert rc == INVALID and "step_size" in msg
    for scale in (float("inf"), float("-inf"), float("nan")):
        for n in (100, 0):
            rc, msg = _call(L, n=n, grad_scale=scale)
            assert rc == INVALID and "grad_scale" in msg and NAME in msg
    # n == 0 still needs every pointer
    assert _call(L, n=0, rays=(None, D))[0] == INVALID
    assert _call(L, n=0, opt=None)[0] == INVALID
    assert _call(L, n=0, target=None)[0] == INVALID
    assert _call(L, n=0, grad_data=None)[0] == INVALID


def test_optional_outputs_are_not_what_is_refused(L):
    """touched / sq_err / accum = NULL pass the argument checks: the refusal that follows is the option's."""
    opt = _opt(render_depth=1)
    for kw in (dict(touched=None), dict(sq_err=None), dict(accum=None), dict(touched=None, sq_err=None, accum=None)):
        rc, msg = _call(L, opt=opt, **kw)
        assert rc == UNSUPPORTED and "render_depth" in msg, kw


def test_unsupported_options_through_c(L):
    for field in ("render_depth", "enable_probe"):
        rc, msg = _call(L, opt=_opt(**{field: 1}))
        assert rc == UNSUPPORTED and field in msg and NAME in msg
        assert _call(L, n=0, opt=_opt(**{field: 1}))[0] == UNSUPPORTED
    for axis in range(3):
        opt = _opt()
        opt.rot_dirs[axis] = 0.5
        rc, msg = _call(L, opt=opt)
        assert rc == UNSUPPORTED and "rot_dirs" in msg and NAME in msg


def test_refusals_through_python(L):
    torch = pytest.importorskip("torch")
    from volrend_amd import api
    t = common.FakeTree(handle=TREE)
    assert api.N3Tree.fit_rays is api.fit_rays
    good = torch.zeros((100, 3), dtype=torch.float32)
    opts = api.RenderOptions()

    def refused(o=good, d=good, tg=good, match="must", **kw):
        with pytest.raises(ValueError, match=match):
            api.fit_rays(t, o, d, opts, tg, **dict(dict(grad_scale=0.5), **kw))
    refused(o=torch.zeros((100, 4)), match="origins")                   # shape
    refused(d=torch.zeros((99, 3)), match="dirs")                       # one ray short
    refused(tg=torch.zeros((100, 4)), match="target")
    refused(tg=torch.zeros((99, 3)), match="target")
    refused(tg=good.double(), match="float32")
    refused(tg=torch.zeros((3, 100)).t(), match="contiguous")
    refused(tg=None, match="target")
    refused(o=[[0.0, 0.0, 0.0]], match="torch tensor")
    refused(match="device")                                             # host tensors: not on the tree's device
    refused(o=O, d=D, tg=T, match="pass n")                             # raw pointers need n
    refused(o=O, d=D, tg=T, n=100, want=("rgba",), match="want")
    refused(o=O, d=D, tg=T, n=100, want=("sq_err", "sq_err"), match="want")
    refused(o=O, d=D, tg=T, n=100, grad_data=torch.zeros((10, 2, 2, 2, 48)), match="grad_data")
    refused(o=O, d=D, tg=T, n=100, grad_data=G, touched=torch.zeros(2, dtype=torch.int32), match="touched")
    for scale in (float("inf"), float("nan"), 1e39):                    # (1e39 is not a finite float32)
        refused(o=O, d=D, tg=T, n=100, grad_data=G, grad_scale=scale, match="grad_scale")
    with pytest.raises(TypeError):
        api.fit_rays(t, O, D, opts, T, n=100, grad_data=G)              # grad_scale has no default
    assert t.info_calls == 0

    # what the C call refuses comes back as VolrendError (raw pointers: nothing is read, refused first)
    def code(**kw):
        options = kw.pop("options", opts)
        with pytest.raises(_abi.VolrendError) as e:
            api.fit_rays(t, O, D, options, T, **dict(dict(grad_scale=0.5, grad_data=G, want=(), n=100), **kw))
        assert NAME in str(e.value) or "step_size" in str(e.value)   # (the step check does not name its caller)
        return e.value.code

    assert code(fp_mode=5) == INVALID
    assert code(options=api.RenderOptions(step_size=0.0)) == INVALID
    assert code(n=1 << 30) == INVALID
    assert code(options=api.RenderOptions(render_depth=True)) == UNSUPPORTED
    assert code(options=api.RenderOptions(rot_dirs=(0.0, 0.1, 0.0)), touched=B) == UNSUPPORTED
    assert code(options=api.RenderOptions(enable_probe=True)) == UNSUPPORTED
    assert t.info_calls == 0


def test_optimizer_has_fit():
    pytest.importorskip("torch")
    from volrend_amd import optim
    assert callable(optim.SparseTreeOptimizer.fit)


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("fit_refusals", tmp_path), refusals=True)
    words = {"null_origins": "NULL", "null_dirs": "NULL", "null_target": "NULL", "null_grad_data": "NULL",
             "fp_mode": "fp_mode", "n_negative": "n=", "n_large": "n=", "step_size": "step_size",
             "grad_scale_inf": "grad_scale", "grad_scale_nan": "grad_scale", "render_depth": "render_depth",
             "enable_probe": "enable_probe", "rot_dirs": "rot_dirs", "null_tree": "NULL"}
    assert sorted(got) == sorted(words)
    for case, text in got.items():
        assert text.startswith(f"runtime_error: {NAME}:") and words[case] in text, (case, text)
