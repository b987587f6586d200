"""Helpers of the vr_accumulate_weights tests: the C restatement of trace_ray's loop with the per-leaf
rule (tests/cpp/weights_restatement.c), compiled on first use with the oracle's flags, and the cases the
CPU and GPU tests share.  Scenes and option sets are those of tests/aov_util.py."""
from __future__ import annotations

import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import aov_util as au
from tests import common
from tests.common import ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "weights_restatement.c")
_lib = None


def lib():
    global _lib
    if _lib is None:
        td = tempfile.mkdtemp(prefix="vr_weights_restate_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "libweights_restatement.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-mfma", "-fPIC", "-shared",
                               "-Wno-unused-function", "-I", os.path.join(ROOT, "oracle"), SRC, "-o", so, "-lm"])
        L = C.CDLL(so)
        L.weights_restate.restype = C.c_int
        L.weights_restate.argtypes = [C.POINTER(ob.OrTree), C.POINTER(ob.OrCamera), C.POINTER(ob.OrOptions), C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


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
