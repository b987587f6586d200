"""Helpers of the vr_fit_rays tests: the numpy restatement of the loss head (include/volrend_hip.h), the rays of a
camera as the FMA model's matrix product forms them, and the float64 gradient of a batch for the head's g."""
from __future__ import annotations

import numpy as np

from tests import grad_util as gu
from tests import rays_util as ru


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
