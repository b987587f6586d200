"""Helpers of the vr_render_backward tests: the C restatement of trace_ray's loop with the derivative's formulas
(tests/cpp/grad_restatement.c), compiled on first use with the oracle's flags, and the cases the CPU and GPU
tests share.  Scenes and option sets are those of tests/aov_util.py."""
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
SRC = os.path.join(ROOT, "tests", "cpp", "grad_restatement.c")
_lib = None

EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126
# The summation constant (tests/test_grad_restatement.py::test_summation_constant measures it): the largest
# |binary32 - binary64| / unit() of the restatement's binary32 entry point over the cases of the GPU parity
# test, in scanline and in shuffled ray order: 36.70 (rgba, no_early_stop, strict), rounded up.  The GPU
# tolerance is K = 4 * K32 -- two bits for the device expf and an arrival order nobody controls.  If the GPU
# exceeds K, that is a finding about the kernel: K does not move.
K32 = 37.0
K = 4.0 * K32

OPTION_SETS = au.OPTION_SETS


def lib():
    global _lib
    if _lib is None:
        td = tempfile.mkdtemp(prefix="vr_grad_restate_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "libgrad_restatement.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-mfma", "-fPIC", "-shared",
                               "-Wno-unused-function", "-I", os.path.join(ROOT, "oracle"), SRC, "-o", so, "-lm"])
        L = C.CDLL(so)
        L.grad_trace_frame.restype = C.c_void_p
        L.grad_trace_frame.argtypes = [C.POINTER(ob.OrTree), C.POINTER(ob.OrCamera), C.POINTER(ob.OrOptions), C.c_int]
        L.grad_trace_free.restype = None
        L.grad_trace_free.argtypes = [C.c_void_p]
        L.grad_trace_rays.restype = None
        L.grad_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.grad_trace_slots.restype = None
        L.grad_trace_slots.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.grad_eval64.restype = C.c_int
        L.grad_eval64.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        L.grad_eval32.restype = C.c_int
        L.grad_eval32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


class Trace:
    """The constants of one frame's differentiation: per ray its hits (slot, delta), basis values, stop flag."""

    def __init__(self, tree, transform, w, h, focal, fp_mode=0, ndc=None, fy=None, **opt_kw):
        th = ob.TreeHandle(tree, ndc=ndc)
        cam = ob.make_camera(transform, w, h, focal, fy)
        opt = ob.default_options(**opt_kw)
        self.w, self.h = w, h
        self.shape = tuple(tree.data.shape)
        self.ptr = lib().grad_trace_frame(C.byref(th.struct), C.byref(cam), C.byref(opt), fp_mode)
        assert self.ptr
        self.n_hits = np.zeros(w * h, np.int64)
        stopped = np.zeros(w * h, np.uint8)
        lib().grad_trace_rays(self.ptr, _p(self.n_hits), _p(stopped))
        self.stopped = stopped.astype(bool)

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.grad_trace_free(self.ptr)
            self.ptr = None

    def slots(self, ray):
        out = np.zeros(int(self.n_hits[ray]), np.int64)
        lib().grad_trace_slots(self.ptr, int(ray), _p(out))
        return out

    def forward64(self, data64):
        """-> (out [h, w, 4], wsum [h, w]) in float64."""
        out = np.zeros((self.h, self.w, 4), np.float64)
        wsum = np.zeros((self.h, self.w), np.float64)
        assert data64.dtype == np.float64 and data64.flags.c_contiguous and data64.shape == self.shape
        assert lib().grad_eval64(self.ptr, _p(data64), None, _p(out), _p(wsum), None, None, None) == 0
        return out, wsum

    def backward64(self, data64, g64, grad=None, mag=None, under=None):
        """Adds the frame's contributions into grad / mag / under (float64, the shape of data; allocated when
        None)."""
        grad = np.zeros(self.shape, np.float64) if grad is None else grad
        mag = np.zeros(self.shape, np.float64) if mag is None else mag
        under = np.zeros(self.shape, np.float64) if under is None else under
        g64 = np.ascontiguousarray(g64, np.float64)
        assert g64.shape == (self.h, self.w, 4) and data64.dtype == np.float64 and data64.flags.c_contiguous
        assert lib().grad_eval64(self.ptr, _p(data64), _p(g64), None, None, _p(grad), _p(mag), _p(under)) == 0
        return grad, mag, under

    def loss64(self, data64, g64):
        """sum(g * out): the scalar whose derivative backward64 claims to be."""
        return float((self.forward64(data64)[0] * g64).sum())

    def backward32(self, data32, g32, order, grad32):
        g32 = np.ascontiguousarray(g32, np.float32)
        order = np.ascontiguousarray(order, np.int64)
        assert data32.dtype == np.float32 and grad32.dtype == np.float32 and grad32.shape == self.shape
        assert lib().grad_eval32(self.ptr, _p(data32), _p(g32), _p(order), order.size, _p(grad32)) == 0
        return grad32


def poses(n, size=96, radius=4.0):
    return [common.camera_for(pose_idx=i % 8, size=size, radius=radius)[0] for i in range(n)]


def decoy_pose(transform):
    """`transform` turned round where it stands: right and back negated (still a rotation).  From a camera that
    looked at the scene every ray now leaves it; the tests that use it check that first."""
    d = np.array(transform, np.float32)
    d[0:3], d[6:9] = -d[0:3], -d[6:9]
    return d


def upstream(kind, n, h, w, seed=7):
    """grad_accum of n frames, float32 [n, h, w, 4]."""
    if kind == "normal":
        return np.random.default_rng(seed).standard_normal((n, h, w, 4)).astype(np.float32)
    g = np.zeros((n, h, w, 4), np.float32)
    g[...] = {"colour": (1, 1, 1, 0), "alpha": (0, 0, 0, 1), "zero": (0, 0, 0, 0)}[kind]
    return g


@functools.lru_cache(maxsize=None)
def tree_of(name):
    """-> (tree, camera radius, ndc)."""
    if name == "sh16":
        return common.small_scene(depth=5, basis_dim=16), 4.0, None
    if name == "sh9_near":
        return common.small_scene(basis_dim=9, seed=3), 2.5, None
    if name == "sh4":
        return common.small_scene(depth=4, basis_dim=4, seed=5), 4.0, None
    if name == "sh25":
        return common.small_scene(depth=4, basis_dim=25, seed=6), 4.0, None
    if name == "basis1":
        return common.small_scene(depth=4, basis_dim=3, seed=7), 4.0, None
    if name == "rgba":
        return common.small_scene(depth=4, basis_dim=-1, fmt="RGBA", seed=8), 4.0, None
    if name == "n4":
        return common.random_tree_general_n(), 4.0, None
    if name == "fog":
        return common.fog_tree(), 4.0, None
    if name == "blocked":
        return common.small_scene(depth=7, basis_dim=4, seed=1201), 4.0, None
    if name == "ndc":
        return common.small_scene(depth=5, basis_dim=4, seed=51), 4.0, au.NDC
    raise KeyError(name)


def views(name, size, n_poses):
    """-> (transforms, w, h, focal)."""
    tree, radius, ndc = tree_of(name)
    if ndc is not None:
        tr2 = au.NDC_TRANSFORM.copy()
        tr2[9:12] += np.float32(0.05)
        return [au.NDC_TRANSFORM, tr2][:n_poses], 48, 36, 40.0
    return poses(n_poses, size=size, radius=radius), size, size, common.camera_for(size=size)[3]


def data64_of(tree):
    return np.ascontiguousarray(tree.data, np.float16).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, optset, fp_mode, n_poses, size, gkind="normal"):
    """The float64 gradient and magnitude of `n_poses` views, once per session and read-only.
    -> dict(tree, ndc, trs, w, h, f, g [n, h, w, 4] float32, grad, mag, traces)."""
    tree, _, ndc = tree_of(name)
    trs, w, h, f = views(name, size, n_poses)
    kw = OPTION_SETS[optset] if isinstance(optset, str) else dict(optset)
    g = upstream(gkind, len(trs), h, w)
    d64 = data64_of(tree)
    grad = np.zeros(d64.shape, np.float64)
    mag = np.zeros(d64.shape, np.float64)
    under = np.zeros(d64.shape, np.float64)
    traces = []
    for i, tr in enumerate(trs):
        t = Trace(tree, tr, w, h, f, fp_mode, ndc=ndc, **kw)
        t.backward64(d64, g[i].astype(np.float64), grad, mag, under)
        traces.append(t)
    for a in (g, grad, mag, under):
        a.setflags(write=False)
    return dict(tree=tree, ndc=ndc, trs=trs, w=w, h=h, f=f, g=g, grad=grad, mag=mag, under=under, traces=traces, opt=kw)


# The cases of the GPU parity test (and of the summation constant): (tree, size, poses)
PARITY_TREES = [("sh16", 96, 2), ("sh9_near", 96, 1), ("sh4", 40, 1), ("sh25", 40, 1), ("basis1", 40, 1),
                ("rgba", 40, 1), ("n4", 40, 1), ("blocked", 40, 1), ("ndc", 0, 1)]
PARITY_CASES = [(n, s, p, o, "normal") for n, s, p in PARITY_TREES for o in OPTION_SETS] + \
               [("sh16", 96, 2, "default", "colour"), ("sh16", 96, 2, "default", "alpha")]


def unit(ref):
    """The error unit per element: 2^-24 M, plus 2^-126 U where binary32 underflows (TINY32 = the smallest normal
    binary32; U = M with every transmittance factor replaced by 1, tests/cpp/grad_restatement.c).  For an
    element whose gradient is not itself of subnormal size the second term is 1e-30 of the first."""
    return EPS32 * ref["mag"] + TINY32 * ref["under"]


def worst_ratio(got, ref):
    """max |got - grad| / unit over the elements with M > 0, and whether got == grad where M == 0."""
    grad, mag = ref["grad"], ref["mag"]
    diff = np.abs(np.asarray(got, np.float64) - grad)
    pos = mag > 0
    ratio = float((diff[pos] / unit(ref)[pos]).max()) if pos.any() else 0.0
    return ratio, bool((diff[~pos] == 0).all())
