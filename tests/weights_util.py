"""Helpers of the vr_accumulate_weights tests: the per-leaf rule over the C restatement of the march
(tests/cpp/weights_restatement.c over march_restatement.h), and the cases the CPU and GPU tests share.
Scenes and option sets are those of tests/aov_util.py."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests import aov_util as au
from tests import build_util, common
from tests.common import ob


@functools.lru_cache(maxsize=None)
def lib():
    L = build_util.c_library("weights_restatement.c")
    L.weights_restate.restype = C.c_int
    L.weights_restate.argtypes = [C.POINTER(ob.OrTree), C.POINTER(ob.OrCamera), C.POINTER(ob.OrOptions), C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_uint64)]
    return L


def slots_shape(tree):
    return (tree.capacity, tree.N, tree.N, tree.N)


def restate_frame(tree, transform, w, h, focal, fp_mode=0, ndc=None, max_weight=None, hits=None, fy=None, **opt_kw):
    """One frame, accumulated INTO max_weight (float32) / hits (uint32), both [capacity, N, N, N] in the
    file's numbering (allocated zeroed when None).
    -> dict(max_weight, hits, D, T, stop [h, w], nonpositive)."""
    th = ob.TreeHandle(tree, ndc=ndc)
    cam = ob.make_camera(transform, w, h, focal, fy)
    opt = ob.default_options(**opt_kw)
    mw = np.zeros(slots_shape(tree), np.float32) if max_weight is None else max_weight
    hc = np.zeros(slots_shape(tree), np.uint32) if hits is None else hits
    assert mw.dtype == np.float32 and hc.dtype == np.uint32 and mw.flags.c_contiguous and hc.flags.c_contiguous
    assert mw.shape == hc.shape == slots_shape(tree)
    D, T = (np.zeros((h, w), np.float32) for _ in range(2))
    stop = np.zeros((h, w), np.uint8)
    bad = C.c_uint64(0)
    rc = lib().weights_restate(C.byref(th.struct), C.byref(cam), C.byref(opt), fp_mode, mw.ctypes.data,
                               hc.ctypes.data, D.ctypes.data, T.ctypes.data, stop.ctypes.data, C.byref(bad))
    assert rc == 0
    return dict(max_weight=mw, hits=hc, D=D, T=T, stop=stop.astype(bool), nonpositive=int(bad.value))


def restate(tree, transforms, w, h, focal, fp_mode=0, ndc=None, max_weight=None, hits=None, fy=None, **opt_kw):
    """All frames into one pair of arrays -> (max_weight, hits, nonpositive over all frames)."""
    mw = np.zeros(slots_shape(tree), np.float32) if max_weight is None else max_weight.copy()
    hc = np.zeros(slots_shape(tree), np.uint32) if hits is None else hits.copy()
    bad = 0
    for tr in transforms:
        bad += restate_frame(tree, tr, w, h, focal, fp_mode, ndc, mw, hc, fy=fy, **opt_kw)["nonpositive"]
    return mw, hc, bad


def poses(n, size=96, radius=4.0):
    """n poses of the 8-pose orbit the other tests use (pose i of camera_for)."""
    return [common.camera_for(pose_idx=i % 8, size=size, radius=radius)[0] for i in range(n)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_slots(got_mw, got_hits, want_mw, want_hits, what=""):
    """Every slot of the tree: max_weight bit for bit, hits exactly."""
    if got_mw is not None:
        bad = bits(got_mw) != bits(want_mw)
        assert not bad.any(), (f"{what}: max_weight differs in {int(bad.sum())} of {bad.size} slots, first at "
                               f"{tuple(np.argwhere(bad)[0])}")
    if got_hits is not None:
        got_hits = np.asarray(got_hits)
        assert got_hits.dtype.itemsize == 4 and got_hits.shape == want_hits.shape, (what, got_hits.dtype, got_hits.shape)
        bad = got_hits.view(np.uint32) != want_hits
        assert not bad.any(), (f"{what}: hits differ in {int(bad.sum())} of {bad.size} slots, first at "
                               f"{tuple(np.argwhere(bad)[0])}")


# the negative-threshold case: negative densities become hits, so some weights are <= 0 (or NaN)
NEGATIVE = dict(sigma_thresh=-1.0)
SCENES = au.SCENES
OPTION_SETS = au.OPTION_SETS
TIE_CASES = au.TIE_CASES


@functools.lru_cache(maxsize=None)
def scene(name):
    return au.scene(name)


RADIUS = {"sh9_near": 2.5}     # (the camera distance au.scene gives the scene)


@functools.lru_cache(maxsize=None)
def reference(scene_name, optset, fp_mode, n_poses, size=None):
    """The restatement of `n_poses` orbit poses (size x size pixels; None = the scene's own size), from
    zeroed arrays; computed once per session and read-only.  optset: a key of OPTION_SETS or "negative".
    -> (tree, transforms, w, h, focal, max_weight, hits, nonpositive)."""
    tree, _, w, _, _ = scene(scene_name)
    size = w if size is None else size
    kw = NEGATIVE if optset == "negative" else OPTION_SETS[optset]
    trs = poses(n_poses, size=size, radius=RADIUS.get(scene_name, 4.0))
    f = common.camera_for(size=size)[3]
    mw, hc, bad = restate(tree, trs, size, size, f, fp_mode, **kw)
    mw.setflags(write=False)
    hc.setflags(write=False)
    return tree, trs, size, size, f, mw, hc, bad


# ---- shared by the GPU tests (torch is handed in: the module imports without it) -----------------------------------
SENT_W = np.float32(2.0 ** -100)          # a known non-negative float: a reached slot holds max(weight, this)
SENT_H = np.uint32(0xFFFFFFF0)            # sixteen short of the wrap: busy slots count through 2^32


def buffers(torch, tree, want=("max_weight", "hits")):
    shape = slots_shape(tree)
    mw = torch.full(shape, float(SENT_W), dtype=torch.float32, device="cuda") if "max_weight" in want else None
    hc = torch.full(shape, -16, dtype=torch.int32, device="cuda") if "hits" in want else None   # SENT_H
    return mw, hc


def expected(want_mw, want_hits):
    """What sentinel-initialised buffers hold after accumulating a reference that started from zero."""
    with np.errstate(over="ignore"):
        return np.maximum(want_mw, SENT_W), (want_hits + SENT_H).astype(np.uint32)


def host(t):
    return None if t is None else t.cpu().numpy()


def accumulate(torch, t, w, h, f, trs, fp_mode=0, want=("max_weight", "hits"), stream=None, mw=None, hc=None,
               tree=None, fy=None, **opt_kw):
    from volrend_amd import api
    if mw is None and hc is None:
        mw, hc = buffers(torch, tree, want)
    cam = api.Camera(w, h, f, f if fy is None else fy)
    t.accumulate_weights(cam, trs, api.RenderOptions(**opt_kw), max_weight=mw, hits=hc,
                         want=(), fp_mode=fp_mode, stream=stream)
    return mw, hc
