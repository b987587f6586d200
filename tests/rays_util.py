"""Helpers of the ray-list tests (vr_render_rays, vr_accumulate_weights_rays, vr_render_backward_rays).

The oracle takes cameras, not rays, and stays as it is.  Pixel (1, 1) of a 2 x 2 camera whose transform is
[0,0,0, 0,0,0, -d, o] has xyz = (0, -0, -1), so the oracle's matrix product yields exactly d in either FP model:
``or_render(region=(1, 1, 1, 1))`` of that camera IS ray (o, d) as the ray-list calls define it (the direction
normalised behind the product, then everything a pixel's ray goes through).  tests/test_rays_restatement.py
pins this against whole frames of the oracle."""
from __future__ import annotations

import numpy as np

from tests.common import ob


def rays_of_camera(transform, w, h, fx, fy=None):
    """The rays of every pixel of a camera in scanline order, float32: origins [h * w, 3] = transform[9:12],
    dirs [h * w, 3] = the 3 x 3 part of ``transform`` times (x, y, -1) with x = (ix - 0.5 w) / fx,
    y = -(iy - 0.5 h) / fy, formed as (m[i] x + m[3 + i] y) + m[6 + i] z -- the strict model's order.  Not
    normalised (the library normalises)."""
    f32 = np.float32
    m = np.asarray(transform, f32)
    fy = fx if fy is None else fy
    ix, iy = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    x = ((ix - f32(0.5) * f32(w)) / f32(fx)).astype(f32).reshape(-1)
    y = (-(iy - f32(0.5) * f32(h)) / f32(fy)).astype(f32).reshape(-1)
    z = f32(-1.0)
    dirs = np.stack([((m[i] * x).astype(f32) + (m[3 + i] * y).astype(f32)).astype(f32) + (m[6 + i] * z)
                     for i in range(3)], axis=1).astype(f32)
    origins = np.broadcast_to(m[9:12], dirs.shape).astype(f32).copy()
    return origins, np.ascontiguousarray(dirs)


def oracle_rays(tree, origins, dirs, fp_mode=0, ndc=None, **opt_kw):
    """Every ray through the oracle as its own 2 x 2 camera -> (rgba uint8 [n, 4], accum float32 [n, 4],
    number of rays that hit the box)."""
    th = ob.TreeHandle(tree, ndc=ndc)
    opt = ob.default_options(**opt_kw)
    origins = np.asarray(origins, np.float32)
    dirs = np.asarray(dirs, np.float32)
    n = origins.shape[0]
    rgba = np.zeros((n, 4), np.uint8)
    accum = np.zeros((n, 4), np.float32)
    hit = 0
    tr = np.zeros(12, np.float32)
    for i in range(n):
        tr[6:9] = -dirs[i]
        tr[9:12] = origins[i]
        r, a, cnt = ob.render(th, ob.make_camera(tr, 2, 2, 1.0), opt, fp_mode, region=(1, 1, 1, 1), nthreads=1)
        rgba[i], accum[i] = r[1, 1], a[1, 1]
        hit += cnt["rays_hit_box"]
    return rgba, accum, hit


def permutation_pose(perm=(1, 2, 0), signs=(1, -1, 1), centre=(3.4, 0.3, -0.2)):
    """A 12-float transform whose columns are +-e_k (column c = signs[c] * e_perm[c]): the matrix product of
    screen2worlddir is then exact, fused or not, so camera-derived rays equal the frame's in both FP models.
    With an odd width and height no component of a direction is zero."""
    tr = np.zeros(12, np.float32)
    for c in range(3):
        tr[3 * c + perm[c]] = signs[c]
    tr[9:12] = centre
    return tr


def world_box(tree):
    """The volume [0, 1]^3 of the tree in world space -> (lo [3], hi [3])."""
    off, sc = np.asarray(tree.offset, np.float64), np.asarray(tree.invradius3, np.float64)
    a, b = (0.0 - off) / sc, (1.0 - off) / sc
    return np.minimum(a, b), np.maximum(a, b)


def arbitrary_rays(tree, n=600, seed=0):
    """n seeded rays, float32: origins outside the volume (a shell around it) and inside it, aimed at points of
    the volume -- one in eight anywhere, so some miss -- with lengths log-uniform in [0.01, 100] and every sign
    combination of the components."""
    rng = np.random.default_rng(seed)
    lo, hi = world_box(tree)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    target = mid + rng.uniform(-0.9, 0.9, (n, 3)) * half
    out = rng.standard_normal((n, 3))
    out = mid + out / np.linalg.norm(out, axis=1, keepdims=True) * np.linalg.norm(half) * rng.uniform(1.2, 2.5, (n, 1))
    inside = mid + rng.uniform(-0.8, 0.8, (n, 3)) * half
    origins = np.where((np.arange(n) % 3 == 0)[:, None], inside, out)
    d = target - origins
    stray = np.arange(n) % 8 == 1
    d[stray] = rng.standard_normal((int(stray.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= 10.0 ** rng.uniform(-2, 2, (n, 1))
    dirs = d.astype(np.float32)
    assert np.isfinite(dirs).all() and (dirs != 0).all()
    combos = {tuple(s) for s in (dirs > 0).astype(int)}
    assert len(combos) == 8, "not every sign combination is present"
    return np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs)


def strip_camera(n, fp_mode=0):
    """A camera of n x 1 pixels whose rays fan through the middle of the volume -> (transform, w, h, focal): a ray
    list of ANY length n that is also a frame, so the oracle, the leaf-weight restatement and the gradient trace
    of that frame judge it.  The strict model takes an orbit pose; the FMA model a signed-permutation pose, whose
    matrix product is exact fused or not.  (The focal length is that of max(n, 8) pixels: the one ray of n = 1
    then looks at the middle of the volume, not past it.)"""
    from tests import common
    if fp_mode == 0:
        return common.camera_for(pose_idx=1, size=96)[0], n, 1, max(n, 8) * 1111.111 / 800.0
    return permutation_pose(), n, 1, max(n, 8) * 112.0 / 95.0


# ---- shared by the GPU tests (torch is handed in: the module imports without it) -----------------------------------
GUARD, POISON = 4096, 0xA5


class Guarded:
    """An output of exactly its own size with a poisoned guard band behind it (the idea of
    tests/test_gpu_refine.py): ``tensor`` is what the call gets, ``host()`` the result once the band has been seen
    intact.  init: None = poisoned like the band, a number or an array = what the buffer starts from."""

    def __init__(self, torch, shape, dtype, init=None):
        self.shape, self.dtype = tuple(int(x) for x in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.raw = torch.full((self.nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        tdtype = {"float32": torch.float32, "int32": torch.int32, "uint8": torch.uint8}[self.dtype.name]
        self.tensor = self.raw[:self.nbytes].view(tdtype).view(self.shape)
        assert self.tensor.data_ptr() == self.raw.data_ptr() and self.tensor.is_contiguous()
        if init is not None:
            self.tensor.copy_(torch.from_numpy(np.broadcast_to(np.asarray(init, self.dtype), self.shape).copy()))

    def host(self):
        raw = self.raw.cpu().numpy()
        assert (raw[self.nbytes:] == POISON).all(), "a store went beyond the end of an output"
        return raw[:self.nbytes].view(self.dtype).reshape(self.shape).copy()
