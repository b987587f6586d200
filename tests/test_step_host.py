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


# ---- the value-domain catalogue (step_util.catalogue; the GPU side: tests/test_gpu_step.py) -----------------------
f32, f64 = np.float32, np.float64
TINY = f32(2.0 ** -126)
BETAS = [(0.0, 0.0), (0.9, 0.999), (0.5, su.BELOW_ONE), (su.BELOW_ONE, 0.0)]
STEPS = [1, 2, 1000, 2 ** 31 - 1]


def flushed(x):
    """binary32 subnormals as zero, the sign kept."""
    x = np.asarray(x, f32)
    return np.where(np.abs(x) < TINY, np.copysign(f32(0), x), x).astype(f32)


def fused(a, b, c):
    """a * b + c with the product exact (binary64) and one rounding to binary32."""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def wrong_restate(variant, kind, master, grad, mask, *, lr, lr_sigma, m=None, v=None, betas=(0.9, 0.999), eps=1e-8,
                  step=1):
    """su.restate with one deliberate mistake -> (master, m, v).  variant: "ftz" | "fma" | "eps_in_sqrt" |
    "bias_in_sqrt" | "lr_for_sigma" (anything else: no mistake)."""
    dd = master.shape[-1]
    mask = np.asarray(mask, bool).reshape(-1)
    z = flushed if variant == "ftz" else (lambda x: np.asarray(x, f32))
    op = lambda f, *xs: z(f(*[z(x) for x in xs]))     # noqa: E731  (one operator: inputs and output through z)
    w0, g = master.reshape(-1, dd)[mask], grad.reshape(-1, dd)[mask]
    m1 = v1 = None
    with np.errstate(all="ignore"):
        if kind == "sgd":
            rates, x = (f32(lr), f32(lr_sigma)), g
        else:
            omb1, omb2, sbc2, a, a_sigma = su.host_scalars(lr, lr_sigma, betas, step)
            beta1, beta2, e = f32(betas[0]), f32(betas[1]), f32(eps)
            rates = (a, a_sigma)
            m0, v0 = m.reshape(-1, dd)[mask], v.reshape(-1, dd)[mask]
            if variant == "fma":
                m1, v1 = fused(omb1, g, beta1 * m0), fused(omb2 * g, g, beta2 * v0)
            else:
                m1 = op(np.add, op(np.multiply, beta1, m0), op(np.multiply, omb1, g))
                v1 = op(np.add, op(np.multiply, beta2, v0), op(np.multiply, op(np.multiply, omb2, g), g))
            if variant == "eps_in_sqrt":
                den = np.sqrt(v1 + e) / sbc2
            elif variant == "bias_in_sqrt":
                den = np.sqrt(v1 / (sbc2 * sbc2)) + e
            else:
                den = op(np.add, op(np.divide, op(np.sqrt, v1), sbc2), e)
            x = op(np.divide, m1, den)
        rate = np.full(dd, rates[0], f32)
        rate[-1] = rates[0] if variant == "lr_for_sigma" else rates[1]
        w = fused(-rate, x, w0) if variant == "fma" else op(np.subtract, w0, op(np.multiply, rate, x))
    assert w.dtype == f32
    out = [np.array(a, f32).reshape(-1, dd) if a is not None else None for a in (master, m, v)]
    for a, new in zip(out, (w, m1, v1)):
        if new is not None:
            a[mask] = new
    return [None if a is None else a.reshape(master.shape) for a in out]


def half_truncated(x):
    """binary32 -> binary16 towards zero."""
    with np.errstate(over="ignore"):
        h = np.asarray(x, f32).astype(np.float16)
    away = np.abs(h.astype(f32)) > np.abs(x)
    return np.where(away, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def half_flushed(x):
    """binary32 -> binary16 to nearest even, subnormal halves as zero."""
    with np.errstate(over="ignore"):
        h = np.asarray(x, f32).astype(np.float16)
    sub = (h.view(np.uint16) & 0x7C00) == 0
    return np.where(sub, np.copysign(np.float16(0), h), h).astype(np.float16)


def changed(a, b):
    """Elements in which b is another value than a non-NaN a."""
    bits = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return int(((a.view(bits) != b.view(bits)) & ~np.isnan(a)).sum())


def test_wrong_restate_without_a_mistake_is_the_restatement():
    c = su.catalogue("sh25")
    for call_name, call in su.CALLS.items():
        want, _ = su.catalogue_expected("sh25", call_name)
        got = wrong_restate(None, call["kind"], c["master"], c["grad"], c["mask"], m=c["m"], v=c["v"], **su.call_kw(call))
        for key, a in zip(("master", "m", "v"), got):
            if want[key] is not None:
                assert su.same_or_nan(a, want[key]).all(), (call_name, key)


@pytest.mark.parametrize("variant", ["ftz", "fma", "eps_in_sqrt", "bias_in_sqrt", "lr_for_sigma", "half_truncated",
                                     "half_flushed"])
@pytest.mark.parametrize("name", su.CATALOGUE_SCENES)
def test_the_catalogue_sees_a_wrong_step(name, variant):
    """Each mistake a kernel could make changes a non-NaN bit of master, m, v or the binary16 data on this scene."""
    c = su.catalogue(name)
    seen = {}
    for call_name, call in su.CALLS.items():
        want, expected16 = su.catalogue_expected(name, call_name)
        if variant.startswith("half_"):
            wrong16 = {"half_truncated": half_truncated, "half_flushed": half_flushed}[variant](want["master"])
            marked = c["mask"].reshape(expected16.shape[:-1])
            seen[call_name] = changed(expected16[marked], wrong16[marked])
            continue
        got = wrong_restate(variant, call["kind"], c["master"], c["grad"], c["mask"], m=c["m"], v=c["v"],
                            **su.call_kw(call))
        seen[call_name] = sum(changed(want[key], a) for key, a in zip(("master", "m", "v"), got) if want[key] is not None)
    print(name, variant, "elements changed per call:", seen)
    assert sum(seen.values()) > 0, "the catalogue does not see this mistake"
    if variant in ("ftz", "fma", "lr_for_sigma", "half_truncated", "half_flushed"):   # (the others are Adam's alone)
        assert seen["sgd"] > 0
    if variant in ("ftz", "fma", "eps_in_sqrt", "bias_in_sqrt"):
        assert seen["adam"] > 0


def formula64(call, w0, g, m, v, sigma):
    """The header's Adam formulas in binary64 with the exact binary32 scalars -> (w, the error unit, in scope): in
    scope is an element none of whose binary32 intermediates overflows, is non-finite or underflows (the unit is
    purely relative: it has no term for a result below 2^-126)."""
    omb1, omb2, sbc2, a, a_sigma = (float(x) for x in su.host_scalars(call["lr"], call["lr_sigma"], call["betas"],
                                                                      call["step"]))
    b1, b2, e = float(f32(call["betas"][0])), float(f32(call["betas"][1])), float(f32(call["eps"]))
    w0, g, m, v = (np.asarray(x, f64) for x in (w0, g, m, v))
    rate = np.where(sigma, a_sigma, a)
    with np.errstate(all="ignore"):
        steps = [b1 * m, omb1 * g, b1 * m + omb1 * g, omb2 * g, omb2 * g * g, b2 * v, b2 * v + omb2 * g * g]
        m1, v1 = steps[2], steps[6]
        steps += [np.sqrt(v1), np.sqrt(v1) / sbc2, np.sqrt(v1) / sbc2 + e]
        den = steps[-1]
        steps += [m1 / den, rate * (m1 / den), w0 - rate * (m1 / den), w0, g, m, v]
        unit = 2.0 ** -24 * (np.abs(w0) + np.abs(rate) * (np.abs(b1 * m) + np.abs(omb1 * g)) / den)
        ok = np.ones(w0.shape, bool)
        for s in steps:
            ok &= np.isfinite(s) & (np.abs(s) <= float(np.finfo(f32).max)) & ((s == 0) | (np.abs(s) >= float(TINY)))
    return steps[12], unit, ok


def random_draws(seed, n=20000):
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice([-1.0, 1.0], n)     # noqa: E731
    w0 = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 2, n)).astype(f32)
    g = (sign() * 10.0 ** rng.uniform(-6, 3, n)).astype(f32)
    m = (sign() * 10.0 ** rng.uniform(-6, 1, n)).astype(f32)
    v = (10.0 ** rng.uniform(-12, 2, n)).astype(f32)
    return w0, g, m, v


def test_restatement_against_float64():
    """su.restate("adam") against the formulas in binary64, in units of 2^-24 times the MAGNITUDES that enter an
    element (not the cancelled m'): the finite part of the catalogue, and random draws under every pair of betas, eps
    and step count.  Ties the restatement to the formula; no GPU tolerance comes from it."""
    worst, worst_case = 0.0, None
    cases = []
    for name in su.CATALOGUE_SCENES:
        c = su.catalogue(name)
        dd = c["master"].shape[-1]
        mask = c["mask"]
        pick = lambda a: a.reshape(-1, dd)[mask]      # noqa: E731
        sigma = np.zeros((int(mask.sum()), dd), bool)
        sigma[:, -1] = True
        for call_name, call in su.CALLS.items():
            if call["kind"] == "adam":
                want, _ = su.catalogue_expected(name, call_name)
                cases.append((f"{name} {call_name}", call, pick(c["master"]), pick(c["grad"]), pick(c["m"]), pick(c["v"]),
                              sigma, pick(want["master"])))
    n = 0
    for betas in BETAS:
        for eps in (0.0, 1e-8, 1.0):
            for step in STEPS:
                call = dict(kind="adam", lr=1e-3, lr_sigma=-0.5, betas=betas, eps=eps, step=step)
                w0, g, m, v = (x.reshape(-1, 2) for x in random_draws(900 + n))
                n += 1
                sigma = np.zeros(w0.shape, bool)
                sigma[:, -1] = True
                got = su.restate("adam", w0, g, np.ones(w0.shape[0], bool), m=m, v=v, **su.call_kw(call))["master"]
                cases.append((f"random draws, betas {betas}, eps {eps}, step {step}", call, w0, g, m, v, sigma, got))
    judged = 0
    for what, call, w0, g, m, v, sigma, got in cases:
        w64, unit, ok = formula64(call, w0, g, m, v, sigma)
        assert ok.sum() > 0.25 * ok.size, (what, int(ok.sum()), ok.size)   # (lr = 3e38 overflows in most elements)
        judged += int(ok.sum())
        err = np.abs(got.astype(f64)[ok] - w64[ok])
        zero = unit[ok] == 0
        assert (err[zero] == 0).all(), what
        ratio = float((err[~zero] / unit[ok][~zero]).max()) if (~zero).any() else 0.0
        if ratio > worst:
            worst, worst_case = ratio, what
    print(f"worst |binary32 - binary64| / unit: {worst:.3f} ({worst_case}), {judged} elements judged")
    assert worst <= su.K_STEP32, (worst, worst_case)
    assert worst > 0.5, "the comparison judged nothing"


def test_host_scalars_of_the_catalogue():
    lr, lr_sigma = 1e-3, 0.5
    for betas in BETAS:
        for step in STEPS:
            s = su.host_scalars(lr, lr_sigma, betas, step)
            assert all(x.dtype == f32 and np.isfinite(x) and x > 0 for x in s), (betas, step, s)
            b1, b2 = float(f32(betas[0])), float(f32(betas[1]))
            if 1.0 - b1 ** step == 1.0:        # beta1^step has underflowed against 1
                assert s[3] == f32(lr) and s[4] == f32(lr_sigma), (betas, step)
            else:
                assert s[3] > f32(lr)
            if b2 == 0.0:
                assert s[2] == f32(1.0)
    assert su.host_scalars(lr, lr_sigma, (0.9, 0.999), 1000)[3] == f32(lr)
    assert su.host_scalars(lr, lr_sigma, (su.BELOW_ONE, 0.0), 2 ** 31 - 1)[3] == f32(lr)
    assert su.host_scalars(lr, lr_sigma, (su.BELOW_ONE, 0.0), 1)[3] == f32(float(f32(lr)) * 2.0 ** 24)
    for call in su.CALLS.values():     # the calls themselves: a and a_sigma stay finite
        if call["kind"] == "adam":
            assert all(np.isfinite(x) for x in su.host_scalars(call["lr"], call["lr_sigma"], call["betas"], call["step"]))
    used = [c for c in su.CALLS.values() if c["kind"] == "adam"]
    assert {c["betas"] for c in used} == set(BETAS) and {c["step"] for c in used} == set(STEPS)
    assert {c["eps"] for c in used} == {0.0, 1e-8, 1.0}
    assert {c["lr"] for c in su.CALLS.values()} == {0.0, 1e-3, -0.5, 3e38}
    assert all(c["lr_sigma"] * c["lr"] < 0 or (c["lr"] == 0 and c["lr_sigma"] < 0) for c in su.CALLS.values())


@pytest.mark.parametrize("name", su.CATALOGUE_SCENES)
def test_catalogue_caps(name):
    """Every entry is where it should be, often enough; NaN stays a small share, so that bit-exactness judges the
    rest; sigma goes everywhere a sigma can go."""
    from tests import update_util as uu
    c = su.catalogue(name)
    tree = uu.case(name)["tree"]
    dd = tree.data_dim
    internal = np.asarray(tree.child).reshape(-1) != 0
    mask = c["mask"]
    assert (mask & internal).sum() >= 3 and (mask & ~internal).sum() > 1000
    flat = {k: c[k].reshape(-1) for k in ("master", "grad", "m", "v")}
    sig = {k: c[k].reshape(-1, dd)[:, -1] for k in ("master", "grad", "m", "v")}
    for label, w0, g, m, v in su.entries():
        at, leaves = c["coeff"][label], c["sigma"][label]
        slot = at // dd
        assert at.size >= 8 and (at % dd != dd - 1).all() and mask[slot].all() and not internal[slot].any(), label
        assert leaves.size >= 4 and mask[leaves].all() and not internal[leaves].any(), label
        for key, x in (("master", w0), ("grad", g), ("m", m), ("v", v)):
            x = np.full(1, x, f32)
            assert su.same_or_nan(flat[key][at], np.repeat(x, at.size)).all(), (label, key)
            assert su.same_or_nan(sig[key][leaves], np.repeat(x, leaves.size)).all(), (label, key)
    marked_elems = int(mask.sum()) * dd
    for call_name, call in su.CALLS.items():
        want, expected16 = su.catalogue_expected(name, call_name)
        nan = int(np.isnan(want["master"]).sum())
        assert nan <= 0.15 * marked_elems, (call_name, nan, marked_elems)
        found = su.sigma_outcomes(name, expected16)
        print(name, call_name, "NaN in master:", nan, "of", marked_elems, "sigma:", found)
        need = su.SIGMA_OUTCOMES if su.passes_through(call) else ("rises", "falls", "nan")
        assert all(found[k] > 0 for k in need), (call_name, found)
        if su.passes_through(call):    # g = m = v = 0: the step hands master through, and the tree rounds it
            edges = uu.edge_values()
            for x in edges:
                at = c["coeff"][f"pass {float(x)!r}"]
                assert su.same_or_nan(want["master"].reshape(-1)[at], np.repeat(x, at.size)).all(), (call_name, x)
                with np.errstate(over="ignore"):
                    h = np.repeat(x, at.size).astype(np.float16)
                assert su.same_or_nan(expected16.reshape(-1)[at], h).all(), (call_name, x)


def test_bitmap_patterns_mark_the_groups_they_name():
    from tests import update_util as uu
    for name in ("rgba", "basis1", "sh9", "sh16", "sh25"):
        tree = uu.case(name)["tree"]
        slots = tree.capacity * tree.N ** 3
        patterns = su.bitmap_patterns(slots)
        assert len(patterns) == 1 + 4 + 2 + len(su.COUNTS) + 2
        for label, words, groups in patterns:
            assert words.dtype == np.uint32 and words.size == su.n_words(slots) and groups, (name, label)
            mask = su.unpack_bits(words, slots)
            for g in groups:
                assert mask[g * su.GROUP:(g + 1) * su.GROUP].any(), (name, label, g)
            named = np.zeros(slots, bool)
            for g in groups:
                named[g * su.GROUP:(g + 1) * su.GROUP] = True
            assert not (mask & ~named).any(), (name, label, "a bit outside the groups the pattern names")
        counts = [int(su.unpack_bits(w, slots).sum()) for label, w, _ in patterns if "bits in group 0" in label]
        assert counts == list(su.COUNTS)
        assert slots % su.GROUP != 0, "the last group is not partial"
