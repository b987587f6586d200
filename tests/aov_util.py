"""Helpers of the vr_render_aov tests: the C restatement of trace_ray's loop without the colour
(tests/cpp/aov_restatement.c), compiled on first use with the oracle's flags, and the scenes the
CPU and GPU tests share."""
from __future__ import annotations

import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import common
from tests.common import ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "aov_restatement.c")
_lib = None


def lib():
    global _lib
    if _lib is None:
        td = tempfile.mkdtemp(prefix="vr_aov_restate_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "libaov_restatement.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-mfma", "-fPIC", "-shared",
                               "-Wno-unused-function", "-I", os.path.join(ROOT, "oracle"), SRC, "-o", so, "-lm"])
        L = C.CDLL(so)
        L.aov_restate.restype = C.c_int
        L.aov_restate.argtypes = [C.POINTER(ob.OrTree), C.POINTER(ob.OrCamera), C.POINTER(ob.OrOptions), C.c_int,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


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
