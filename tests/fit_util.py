"""Helpers of the vr_fit_rays tests: the numpy restatement of the loss head (include/volrend_hip.h), the rays of a
camera as the FMA model's matrix product forms them, the float64 gradient of a batch for the head's g, and the four
checks the GPU tests hold a fused call to (assert_four)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import grad_util as gu
from tests import rays_util as ru
from tests import step_util as su

BG = 0.625                                   # not 0 and not 1: g_3 = -bg sum g_ch matters


def head(out, target, bg, grad_scale, dtype=np.float32):
    """The loss head over out [n, 4] and target [n, 3], every operator rounded once to ``dtype`` in the header's
    order -> dict(pred [n, 3], r [n, 3], sq_err [n], g [n, 4]).  numpy rounds each binary32 operation once and
    fuses nothing, which is the kernel's "uncontracted binary32"."""
    f = dtype
    out, target = np.asarray(out, f), np.asarray(target, f)
    bg, gs = f(bg), f(grad_scale)
    with np.errstate(all="ignore"):
        na = f(1.0) - out[:, 3]
        pred = out[:, :3] + (bg * na)[:, None]
        r = pred - target
        sq = r * r
        sq_err = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        g3 = gs * r
        g = np.empty((out.shape[0], 4), f)
        g[:, :3] = g3
        g[:, 3] = -(bg * ((g3[:, 0] + g3[:, 1]) + g3[:, 2]))
    assert all(a.dtype == f for a in (pred, r, sq_err, g))
    return dict(pred=pred, r=r, sq_err=sq_err, g=g)


def loss64(out64, target, bg, grad_scale):
    """L = grad_scale / 2 * sum r^2 per ray, float64 [n] (summing it gives the loss)."""
    r = head(out64, target, bg, grad_scale, np.float64)["r"]
    return 0.5 * float(grad_scale) * (r * r).sum(1)


def _fma32(a, b, c):
    """fmaf(a, b, c) over float32 arrays, correctly rounded: the product of two binary32 is exact in binary64; the
    sum p + c is formed with its exact residual, and where the binary64 sum sits exactly on a binary32 tie the
    residual decides (rounding binary64 -> binary32 a second time would not see it)."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)              # TwoSum: s + err == p + c exactly
    tie = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    nudge = tie & (err != 0)
    s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def rays_of_camera(transform, w, h, fx, fp_mode=0, fy=None):
    """rays_util.rays_of_camera in FP model ``fp_mode``: the strict model's order, or the FMA model's
    fmaf(m[6 + i], z, fmaf(m[i], x, m[3 + i] * y)) (the oracle's mv3) -- the frame's bits in either model."""
    if fp_mode == 0:
        return ru.rays_of_camera(transform, w, h, fx, fy)
    f32 = np.float32
    m = np.asarray(transform, f32)
    fy = fx if fy is None else fy
    ix, iy = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    x = ((ix - f32(0.5) * f32(w)) / f32(fx)).astype(f32).reshape(-1)
    y = (-(iy - f32(0.5) * f32(h)) / f32(fy)).astype(f32).reshape(-1)
    z = np.full_like(x, -1.0)
    dirs = np.stack([_fma32(m[6 + i], z, _fma32(m[i], x, (m[3 + i] * y).astype(f32))) for i in range(3)], axis=1)
    origins = np.broadcast_to(m[9:12], dirs.shape).astype(f32).copy()
    return origins, np.ascontiguousarray(dirs, f32)


def camera_rays(trs, w, h, fx, fp_mode=0):
    """The rays of every pixel of every view, frame after frame in scanline order."""
    parts = [rays_of_camera(tr, w, h, fx, fp_mode) for tr in trs]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def targets(n, seed):
    return np.random.default_rng(seed).random((n, 3), np.float32)


def reference_for(ref, g):
    """grad_util.reference's dict for the upstream gradient ``g`` [views * h * w, 4] over the traces of ``ref``: the
    float64 gradient and the magnitudes assert_parity needs.  Rays whose row of g is zero add nothing."""
    d64 = gu.data64_of(ref["tree"])
    grad, mag, under = (np.zeros(d64.shape, np.float64) for _ in range(3))
    g = np.asarray(g, np.float64).reshape(len(ref["traces"]), ref["h"], ref["w"], 4)
    for i, t in enumerate(ref["traces"]):
        t.backward64(d64, g[i], grad, mag, under)
    return dict(ref, g=g, grad=grad, mag=mag, under=under)


# ---- shared by the GPU tests (torch is handed in: the module imports without it) -----------------------------------
def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the references are read-only)


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def zero_bits(torch, tree):
    return torch.zeros(su.n_words(tree.capacity * tree.N ** 3), dtype=torch.int32, device="cuda")


def options(ref, **kw):
    from volrend_amd import api
    return api.RenderOptions(**dict(dict(ref["opt"], background_brightness=BG), **kw))


def fit(torch, t, ref, o, d, target, fp_mode, grad_scale, start=None, grad_data=None, touched="new", want=("sq_err", "accum"),
        opts=None, out=None):
    """One fit_rays call -> (result dict, touched).  ``out``: the caller's own "sq_err" [n] and "accum" [n, 4]
    tensors (the Python call allocates these two itself, so this goes through the C entry point)."""
    if grad_data is None and start is not None:
        grad_data = dev(torch, start)
    if isinstance(touched, str):
        touched = zero_bits(torch, ref["tree"])
    od, dd, td, opts = dev(torch, o), dev(torch, d), dev(torch, target), opts or options(ref)
    if out is None:
        res = t.fit_rays(od, dd, opts, td, grad_scale=grad_scale, grad_data=grad_data, touched=touched, want=want,
                         fp_mode=fp_mode)
        return res, touched
    from volrend_amd import _abi
    assert len(o) > 0 and grad_data is not None and touched is not None
    rays, c_opts, c_fit = _abi.VrRays(), opts.to_c(), _abi.VrFit()
    rays.origins, rays.dirs = od.data_ptr(), dd.data_ptr()
    c_fit.target, c_fit.grad_scale, c_fit.grad_data = td.data_ptr(), float(grad_scale), grad_data.data_ptr()
    c_fit.touched, c_fit.sq_err, c_fit.accum = touched.data_ptr(), out["sq_err"].data_ptr(), out["accum"].data_ptr()
    _abi.check(_abi.lib().vr_fit_rays(t.handle, len(o), C.byref(rays), C.byref(c_opts), int(fp_mode), C.byref(c_fit),
                                      None))
    torch.cuda.synchronize()       # (od, dd, td are this function's: they must outlive the launch)
    return dict(out, grad_data=grad_data), touched


def unfused(torch, t, ref, o, d, target, fp_mode, grad_scale, opts=None):
    """The sequence the call fuses: render_rays -> the numpy head -> the marked render_backward_rays
    -> (accum float32 [n, 4], the head's dict, grad_data, touched words)."""
    opts = opts or options(ref)
    od, dd = dev(torch, o), dev(torch, d)
    accum = t.render_rays(od, dd, opts, want=("accum",), fp_mode=fp_mode)["accum"].cpu().numpy()
    want = head(accum, target, BG, grad_scale)
    touched = zero_bits(torch, ref["tree"])
    grad = t.render_backward_rays(od, dd, opts, dev(torch, want["g"]), fp_mode=fp_mode, touched=touched)
    return accum, want, grad, touched


def assert_four(torch, t, ref, o, d, target, fp_mode, what, idx=None, guarded=None):
    """The four checks of tests/test_gpu_fit.py's docstring for one list (rays ``idx`` of the views of ``ref``; all
    when None).  ``guarded``: a factory (torch, shape, numpy dtype, init) -> an object with .tensor and .host() (the
    Guarded of tests/rays_util.py): the call's four outputs then sit in such buffers, whose guard bands .host()
    checks."""
    n = len(o)
    grad_scale = 2.0 / (3 * n)
    start = gu.sentinel(ref["grad"].shape)
    if guarded is None:
        res, touched = fit(torch, t, ref, o, d, target, fp_mode, grad_scale, start=start)
    else:
        tree = ref["tree"]
        bufs = dict(grad_data=guarded(torch, start.shape, np.float32, start),
                    touched=guarded(torch, (su.n_words(tree.capacity * tree.N ** 3),), np.int32, 0),
                    sq_err=guarded(torch, (n,), np.float32, None), accum=guarded(torch, (n, 4), np.float32, None))
        fit(torch, t, ref, o, d, target, fp_mode, grad_scale, grad_data=bufs["grad_data"].tensor,
            touched=bufs["touched"].tensor, out=dict(sq_err=bufs["sq_err"].tensor, accum=bufs["accum"].tensor))
        res = {k: b.host() for k, b in bufs.items()}
        touched = res.pop("touched")
    accum, want, _, touched_b = unfused(torch, t, ref, o, d, target, fp_mode, grad_scale)
    torch.cuda.synchronize()
    assert t.status() == 0
    assert np.isfinite(accum).all()
    bad = (bits(res["accum"]) != bits(accum)).any(1)
    assert not bad.any(), f"{what}: accum differs from render_rays in {int(bad.sum())} of {n} rays, first {np.flatnonzero(bad)[:4]}"
    bad = bits(res["sq_err"]) != bits(want["sq_err"])
    assert not bad.any(), f"{what}: sq_err differs from the numpy head in {int(bad.sum())} of {n} rays"
    assert np.array_equal(bits(touched), bits(touched_b)), f"{what}: touched differs from the marked backward's"
    assert bits(touched).any()
    g = np.zeros((len(ref["traces"]) * ref["h"] * ref["w"], 4), np.float32)
    g[np.arange(n) if idx is None else idx] = want["g"]
    fref = reference_for(ref, g)
    got = res["grad_data"]
    gu.assert_parity(got.cpu().numpy() if hasattr(got, "cpu") else got, fref, start=start, what=what)
    return res, want, fref
