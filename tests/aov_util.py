"""Helpers of the vr_render_aov tests: the per-pixel planes of the C restatement of the march
(tests/cpp/aov_restatement.c over march_restatement.h), and the scenes the CPU and GPU tests share."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests import build_util, common
from tests.common import ob


@functools.lru_cache(maxsize=None)
def lib():
    L = build_util.c_library("aov_restatement.c")
    L.aov_restate.restype = C.c_int
    L.aov_restate.argtypes = [C.POINTER(ob.OrTree), C.POINTER(ob.OrCamera), C.POINTER(ob.OrOptions), C.c_int,
                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def restate(tree, transform, w, h, focal, fp_mode=0, ndc=None, offscreen=True, depth_init=None, fy=None, **opt_kw):
    """-> (D, T, delta_scale float32 [h,w], stopped bool [h,w]) of every pixel."""
    th = ob.TreeHandle(tree, ndc=ndc)
    cam = ob.make_camera(transform, w, h, focal, fy)
    opt = ob.default_options(**opt_kw)
    D, T, ds = (np.zeros((h, w), np.float32) for _ in range(3))
    stop = np.zeros((h, w), np.uint8)
    dep = None if depth_init is None else np.ascontiguousarray(depth_init, np.float32)
    rc = lib().aov_restate(C.byref(th.struct), C.byref(cam), C.byref(opt), fp_mode, 1 if offscreen else 0,
                           None if dep is None else dep.ctypes.data, D.ctypes.data, T.ctypes.data, ds.ctypes.data,
                           stop.ctypes.data)
    assert rc == 0
    return D, T, ds, stop.astype(bool)


def world_depth(D, ds):
    """VR_DEPTH_WORLD: fl(D * delta_scale), one rounding."""
    with np.errstate(all="ignore"):
        return (D.astype(np.float32) * ds.astype(np.float32)).astype(np.float32)


def same_bits(a, b):
    """Mask of the words that are bit-equal, or NaN in both."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~same_bits(got, want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ, first at {tuple(np.argwhere(bad)[0])}"


# option sets of the tie to the oracle
OPTION_SETS = {
    "default": {},
    "no_early_stop": dict(stop_thresh=0.0),
    "coarse": dict(step_size=1e-2, sigma_thresh=0.5),
}


def scene(name):
    """-> (tree, transform, w, h, focal) of the scenes the issue names."""
    if name == "sh16":
        return (common.small_scene(depth=5, basis_dim=16),) + common.camera_for(size=96)
    if name == "sh9_near":
        return (common.small_scene(basis_dim=9, seed=3),) + common.camera_for(size=96, radius=2.5)
    if name == "fog":
        return (common.fog_tree(),) + common.camera_for(size=64)
    if name == "n4":
        return (common.random_tree_general_n(),) + common.camera_for(size=64)
    if name == "value_edge":
        return (common.value_edge_tree(),) + common.camera_for(size=56)
    raise KeyError(name)


SCENES = ("sh16", "sh9_near", "fog", "n4", "value_edge")
# (the fog tree has no sample above sigma_thresh = 0.5: every D is 0 and the case shows nothing)
TIE_CASES = [(s, o) for s in SCENES for o in OPTION_SETS if (s, o) != ("fog", "coarse")]
NDC = (96.0, 72.0, 80.0)
NDC_TRANSFORM = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.05, -0.02, 0.3], dtype=np.float32)


# ---- shared by the GPU tests (torch is handed in: the module imports without it) -----------------------------------
SENTINEL = 0x7FC12345   # a NaN payload no computation produces: "this word was never written"


def sentinel_planes(torch, n, h, w_words):
    return torch.full((n, h, w_words), SENTINEL, dtype=torch.int32, device="cuda")


def host_f32(t):
    return t.cpu().numpy().view(np.float32)


def render_both(torch, t, w, h, f, trs, fp_mode=0, units="tree", offscreen=True, rgba_init=None,
                depth_init=None, shard=None, stream=None, want=("depth", "transmittance"), pad_words=0, fy=None,
                **opt_kw):
    """One vr_render_batch launch and one vr_render_aov launch of the same arguments.
    -> dict(img0, acc0, img1, acc1, depth, trans) as numpy arrays; planes [n, h, w + pad_words] float32
    (SENTINEL where never written), depth / trans None when not asked for."""
    from volrend_amd import api
    n = len(trs)
    cam = api.Camera(w, h, f, f if fy is None else fy)
    opts = api.RenderOptions(**opt_kw)
    out = {}
    depths = None if depth_init is None else [torch.from_numpy(depth_init).cuda() for _ in range(n)]
    dp = sentinel_planes(torch, n, h, w + pad_words) if "depth" in want else None
    tp = sentinel_planes(torch, n, h, w + pad_words) if "transmittance" in want else None
    aov = [api.AovPlanes(dp[i] if dp is not None else None, tp[i] if tp is not None else None,
                         (w + pad_words) * 4 if pad_words else 0) for i in range(n)]
    for k, kw in (("0", {}), ("1", dict(aov=aov, depth_units=units))):
        shape = (n, h, w, 4)
        if shard is not None and shard.compact:
            shape = (n, api.compact_bytes(w, h, shard))
        if rgba_init is not None:
            img = torch.from_numpy(np.broadcast_to(rgba_init, (n,) + rgba_init.shape).copy()).cuda()
        else:
            img = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        acc = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
        api.launch_renderer_batch(t, cam, trs, opts, list(img), stream, offscreen, accums=list(acc),
                                  depths=depths, shard=shard, fp_mode=fp_mode, **kw)
        torch.cuda.synchronize()
        out["img" + k], out["acc" + k] = img.cpu().numpy(), acc.cpu().numpy()
    assert t.status() == 0
    out["depth"] = None if dp is None else host_f32(dp)
    out["trans"] = None if tp is None else host_f32(tp)
    return out


def assert_colour_unchanged(r, what=""):
    assert np.array_equal(r["img1"], r["img0"]), f"{what}: RGBA8 differs from vr_render_batch"
    assert_same_bits(r["acc1"], r["acc0"], f"{what}: accum vs vr_render_batch")


def check(torch, tree, trs, w, h, f, fp_mode=0, ndc=None, units=("tree", "world"), offscreen=True,
          rgba_init=None, depth_init=None, tree_tuning=None, fy=None, **opt_kw):
    """Upload, launch per depth unit, compare every pixel of every frame with the restatement."""
    from volrend_amd import api
    t = api.N3Tree.from_synth(tree, ndc=ndc)
    if tree_tuning:
        t.set_tuning(**tree_tuning)
    want = [restate(tree, tr, w, h, f, fp_mode, ndc=ndc, offscreen=offscreen, depth_init=depth_init, fy=fy,
                    **opt_kw)
            for tr in trs]
    try:
        for u in units:
            r = render_both(torch, t, w, h, f, trs, fp_mode, u, offscreen, rgba_init, depth_init, fy=fy, **opt_kw)
            assert_colour_unchanged(r, u)
            for i, (D, T, ds, _) in enumerate(want):
                assert_same_bits(r["depth"][i], D if u == "tree" else world_depth(D, ds), f"depth[{u}] frame {i}")
                assert_same_bits(r["trans"][i], T, f"transmittance frame {i}")
    finally:
        t.free_device()
    return want
