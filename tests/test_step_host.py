"""vr_tree_step and the marked backward calls (vr_render_backward_touched, vr_render_backward_rays_touched), the part
that needs no GPU: the C ABI (symbols, prototypes, struct layout), every refusal that comes before the tree handle
is followed -- through C, C++ and Python -- and the self-checks of the numpy restatement the GPU tests compare
with (tests/step_util.py).  The calls below pass a tree handle that is never followed and device pointers that
are never read or written."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import build_util, common, step_util as su
from volrend_amd import _abi, build

INVALID = 1
TREE, D, BITS = 0x1000, 0x5000, 0x6000   # never dereferenced
NEW_CALLS = ("vr_tree_step", "vr_render_backward_touched", "vr_render_backward_rays_touched")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbols_prototypes_and_struct_layout(L, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_CALLS:
        assert name in exported and name in _abi.PROTOTYPES
    assert L.vr_abi_version() == 3      # additions only
    assert len(_abi.PROTOTYPES["vr_render_backward_touched"][1]) == len(_abi.PROTOTYPES["vr_render_backward"][1]) + 1
    assert len(_abi.PROTOTYPES["vr_render_backward_rays_touched"][1]) == \
        len(_abi.PROTOTYPES["vr_render_backward_rays"][1]) + 1
    assert (_abi.STEP_SGD, _abi.STEP_ADAM) == (0, 1)
    got = build_util.c_struct_layout("VrStep", _abi.VrStep, [("sgd", "VR_STEP_SGD"), ("adam", "VR_STEP_ADAM")])
    assert got["size"] == C.sizeof(_abi.VrStep) and (got["sgd"], got["adam"]) == (0, 1)
    for n, _ in _abi.VrStep._fields_:
        assert got[n] == getattr(_abi.VrStep, n).offset, n


def make_step(**kw):
    s = _abi.VrStep()
    s.master = s.grad = s.m = s.v = D
    s.touched = BITS
    s.kind, s.lr, s.lr_sigma, s.beta1, s.beta2, s.eps, s.step = _abi.STEP_ADAM, 0.1, 0.2, 0.9, 0.999, 1e-8, 1
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_step_refusals_through_c(L):
    def call(tree=TREE, s=None, **kw):
        s = make_step(**kw) if s is None else s
        return L.vr_tree_step(tree, C.byref(s), None), (L.vr_last_error() or b"").decode()

    rc, msg = call(tree=None)
    assert rc == INVALID and "NULL" in msg
    assert L.vr_tree_step(TREE, None, None) == INVALID and b"NULL" in L.vr_last_error()
    for name in ("master", "grad", "touched"):
        for kind in (_abi.STEP_SGD, _abi.STEP_ADAM):
            rc, msg = call(**{name: None, "kind": kind})
            assert rc == INVALID and "NULL" in msg, (name, kind)
    for kind in (2, -1, 7):
        rc, msg = call(kind=kind)
        assert rc == INVALID and "kind" in msg, kind
    for name in ("m", "v"):
        rc, msg = call(**{name: None})
        assert rc == INVALID and "moments" in msg, name
    for step in (0, -1, -2 ** 31):
        rc, msg = call(step=step)
        assert rc == INVALID and "step" in msg, step
    for name in ("beta1", "beta2"):
        for bad in (1.0, 1.5, -0.1, float("nan"), float("inf")):
            rc, msg = call(**{name: bad})
            assert rc == INVALID and "beta" in msg, (name, bad)
    for name in ("lr", "lr_sigma", "eps"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            for kind in (_abi.STEP_SGD, _abi.STEP_ADAM):
                rc, msg = call(**{name: bad, "kind": kind})
                assert rc == INVALID and "finite" in msg, (name, bad, kind)


def test_marked_backward_refusals_through_c(L):
    """NULL touched, and every refusal of the unmarked siblings that needs no tree, with a garbage handle."""
    o = _abi.VrRenderOptions()
    L.vr_default_options(C.byref(o))
    cams = (_abi.VrCamera * 2)()
    for c in cams:
        c.width, c.height, c.fx, c.fy = 16, 16, 20.0, 20.0
    rays = _abi.VrRays()
    rays.origins = rays.dirs = D

    def frames(tree=TREE, n=2, cams=cams, opt=o, fp=0, ga=D, gd=D, touched=BITS):
        return (L.vr_render_backward_touched(tree, n, cams, C.byref(opt) if opt is not None else None, fp, ga, gd,
                                             touched, None), (L.vr_last_error() or b"").decode())

    def lists(tree=TREE, n=64, rays=rays, opt=o, fp=0, ga=D, gd=D, touched=BITS):
        return (L.vr_render_backward_rays_touched(tree, n, C.byref(rays) if rays is not None else None,
                                                  C.byref(opt) if opt is not None else None, fp, ga, gd, touched, None),
                (L.vr_last_error() or b"").decode())

    for call in (frames, lists):
        rc, msg = call(touched=None)
        assert rc == INVALID and "NULL" in msg and "touched" in msg
        for kw in (dict(tree=None), dict(opt=None), dict(ga=None), dict(gd=None)):
            rc, msg = call(**kw)
            assert rc == INVALID and "NULL" in msg, (call.__name__, kw)
        rc, msg = call(fp=2)
        assert rc == INVALID and "fp_mode" in msg
        bad = _abi.VrRenderOptions()
        L.vr_default_options(C.byref(bad))
        bad.step_size = 0.0
        rc, msg = call(opt=bad)
        assert rc == INVALID and "step_size" in msg
        for field in ("render_depth", "enable_probe"):
            bad = _abi.VrRenderOptions()
            L.vr_default_options(C.byref(bad))
            setattr(bad, field, 1)
            rc, msg = call(opt=bad)
            assert rc == 5 and field in msg and "touched" in msg, field
        bad = _abi.VrRenderOptions()
        L.vr_default_options(C.byref(bad))
        bad.rot_dirs[1] = 0.5
        assert call(opt=bad)[0] == 5
    assert frames(cams=None)[0] == INVALID and frames(n=-1)[0] == INVALID and frames(n=_abi.MAX_BATCH + 1)[0] == INVALID
    cams[1].width = 17
    assert frames()[0] == INVALID and "intrinsics" in frames()[1]
    cams[1].width = 16
    assert lists(rays=None)[0] == INVALID and lists(n=-1)[0] == INVALID and lists(n=1 << 30)[0] == INVALID
    empty = _abi.VrRays()
    assert lists(rays=empty)[0] == INVALID


def test_refusals_through_python(L):
    torch = pytest.importorskip("torch")
    from volrend_amd import api
    t = common.FakeTree(handle=TREE)
    assert api.touched_words(t) == 3    # 80 slots
    shape = (10, 2, 2, 2, 49)
    x = torch.zeros(shape, dtype=torch.float32)
    bits = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="kind"):
        api.tree_step(t, x, x, bits, kind="rmsprop", lr=0.1)
    with pytest.raises(ValueError, match="device"):
        api.tree_step(t, x, x, bits, lr=0.1)                   # host tensors
    with pytest.raises(ValueError, match="float32"):
        api.tree_step(t, x.half(), x, bits, lr=0.1)
    with pytest.raises(ValueError, match="moments"):
        api.tree_step(t, D, D, BITS, kind="adam", lr=0.1)
    with pytest.raises(ValueError, match="int32"):
        api._touched_ptr(t, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="words"):
        api._touched_ptr(t, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="device"):
        api._touched_ptr(t, bits)

    class Cai:   # anything with a device pointer; what the C call refuses comes back as VolrendError
        def __init__(self, ptr):
            self.__cuda_array_interface__ = dict(shape=shape, typestr="<f4", data=(ptr, False), strides=None, version=3)

    with pytest.raises(_abi.VolrendError) as e:
        api.tree_step(t, Cai(D), Cai(D), BITS, lr=float("nan"))
    assert e.value.code == INVALID and "finite" in str(e.value)
    with pytest.raises(_abi.VolrendError) as e:
        api.tree_step(t, Cai(D), Cai(D), BITS, kind="adam", m=Cai(D), v=Cai(D), lr=0.1, step=0)
    assert e.value.code == INVALID and "step" in str(e.value)
    with pytest.raises(_abi.VolrendError) as e:
        api.tree_step(t, Cai(D), Cai(0), BITS, lr=0.1)
    assert e.value.code == INVALID and "NULL" in str(e.value)


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("step_refusals", tmp_path), refusals=True)
    step_cases = [("null_tree", "NULL"), ("null_master", "NULL"), ("null_grad", "NULL"), ("null_touched", "NULL"),
                  ("kind", "kind"), ("lr_nan", "finite"), ("lr_sigma_inf", "finite"), ("eps_nan", "finite"),
                  ("adam_null_m", "moments"), ("adam_null_v", "moments"), ("adam_step0", "step"),
                  ("adam_beta1", "beta"), ("adam_beta2", "beta")]
    for case, word in step_cases:
        line = got[f"step_{case}"]
        assert line.startswith("runtime_error: vr_tree_step:") and word in line, (case, line)
    for call, fn in (("frames", "vr_render_backward_touched"), ("rays", "vr_render_backward_rays_touched")):
        for case in ("null_touched", "null_tree", "null_grad" if call == "frames" else "null_grad_accum"):
            line = got[f"{call}_{case}"]
            assert line.startswith(f"runtime_error: {fn}:") and "NULL" in line, (call, case, line)
    assert len(got) == len(step_cases) + 6


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_bitmap_round_trip():
    rng = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 27 * 5, 1000):
        mask = rng.random(n) < 0.3
        words = su.pack_bits(mask)
        assert words.dtype == np.uint32 and words.size == su.n_words(n)
        assert np.array_equal(su.unpack_bits(words, n), mask)
        for s in np.flatnonzero(mask)[:5]:
            assert (int(words[s >> 5]) >> (s & 31)) & 1
        assert sum(bin(int(w)).count("1") for w in words) == int(mask.sum())


def test_sgd_with_a_zero_gradient_keeps_every_bit():
    rng = np.random.default_rng(1)
    master = rng.standard_normal((40, 13)).astype(np.float32)
    master[::3, 0] = -0.0
    master[1::3, 5] = 0.0
    master[2, 2], master[3, 3], master[4, 4] = np.float32(2.0 ** -140), np.inf, -np.inf
    grad = np.zeros_like(master)
    mask = rng.random(40) < 0.5
    out = su.restate("sgd", master, grad, mask, lr=0.3, lr_sigma=7.0)
    assert np.array_equal(out["master"].view(np.uint32), master.view(np.uint32))
    assert (out["master"].view(np.uint32) == 0x80000000).sum() >= 10, "no -0 in the sample"
    assert np.array_equal(out["grad"].view(np.uint32), np.zeros(master.shape, np.uint32))
    assert out["m"] is None and out["v"] is None


def test_sgd_restatement_rates_and_mask():
    rng = np.random.default_rng(2)
    master = rng.standard_normal((50, 4)).astype(np.float32)
    grad = rng.standard_normal((50, 4)).astype(np.float32)
    mask = np.arange(50) % 3 == 0
    out = su.restate("sgd", master, grad, mask, lr=0.25, lr_sigma=2.0)
    want = master.copy()
    want[mask, :3] = master[mask, :3] - np.float32(0.25) * grad[mask, :3]   # (both rates are exact: one rounding each)
    want[mask, 3] = master[mask, 3] - np.float32(2.0) * grad[mask, 3]
    assert np.array_equal(out["master"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out["grad"][~mask].view(np.uint32), grad[~mask].view(np.uint32))
    assert not out["grad"][mask].any() and not np.signbit(out["grad"][mask]).any()


def test_adam_first_step_is_the_closed_form():
    """step = 1 with zero moments: m' = (1 - b1) g, v' = (1 - b2) g^2, bias corrections 1 - b1 and sqrt(1 - b2), so
    w = master - lr g / (|g| + eps) up to rounding.  Every operator of the restatement rounds once (relative error
    2^-24 each): the update term carries at most 8 roundings (omb1, omb2, two products for v', sqrt (half), divide by
    sbc2, add eps, divide, a_e and its product) and the final subtraction one on the result."""
    rng = np.random.default_rng(3)
    master = rng.standard_normal((64, 49)).astype(np.float32)
    grad = (rng.standard_normal((64, 49)) * 10.0 ** rng.uniform(-3, 1, (64, 49))).astype(np.float32)
    zeros = np.zeros_like(master)
    mask = np.ones(64, bool)
    mask[::5] = False
    lr, lr_sigma, eps = 0.01, 0.5, 1e-8
    out = su.restate("adam", master, grad, mask, lr=lr, lr_sigma=lr_sigma, m=zeros, v=zeros, eps=eps, step=1)
    g = grad.astype(np.float64)
    rate = np.full(49, float(np.float32(lr)))
    rate[-1] = float(np.float32(lr_sigma))
    upd = rate * g / (np.abs(g) + float(np.float32(eps)))
    want = master.astype(np.float64) - upd
    err = np.abs(out["master"].astype(np.float64) - want)[mask]
    bound = (9 * 2.0 ** -24 * np.abs(upd) + 2.0 ** -24 * np.abs(want))[mask]
    assert (err <= bound).all(), float((err / bound).max())
    assert np.array_equal(out["master"][~mask].view(np.uint32), master[~mask].view(np.uint32))
    assert not out["m"][~mask].any() and not out["v"][~mask].any()
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert np.allclose(out["m"][mask], (1 - b1) * g[mask], rtol=2.0 ** -22, atol=0)
    assert np.allclose(out["v"][mask], (1 - b2) * g[mask] ** 2, rtol=2.0 ** -21, atol=1e-44)
    omb1, omb2, sbc2, a, a_sigma = su.host_scalars(lr, lr_sigma, (0.9, 0.999), 1)
    assert all(x.dtype == np.float32 for x in (omb1, omb2, sbc2, a, a_sigma))
    assert omb1 == np.float32(1.0 - b1) and sbc2 == np.float32(np.sqrt(1.0 - b2))
    assert a == np.float32(float(np.float32(lr)) / (1.0 - b1)) and a_sigma != a


def test_mixture_rounds_only_marked_slots():
    old = np.arange(24, dtype=np.float32).reshape(6, 4).astype(np.float16)
    master = (old.astype(np.float32) + np.float32(1 + 2.0 ** -11))   # a tie: rounds to even
    mask = np.array([1, 0, 0, 1, 0, 1], bool)
    got = su.mixture(old, master, mask)
    assert np.array_equal(got[~mask], old[~mask])
    assert np.array_equal(got[mask].view(np.uint16), master[mask].astype(np.float16).view(np.uint16))
