"""Helpers of the vr_order_rays tests: the key of a ray from the C restatement over the oracle's functions
(tests/cpp/order_restatement.c), the result rule, and the cases the CPU and GPU tests share."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np

from tests import build_util, common
from tests import rays_util as ru
from tests.common import ob

MISS = np.uint32(0xFFFFFFFF)
DEFAULT_BITS = 2            # what VrRayOrder.bits == 0 selects (include/volrend_hip.h states it)
KEY_WAVES = 4               # waves per workgroup of the key kernel (vr_order.h kOrderKeyWaves)
NDC = (120.0, 60.0, 95.0)   # an NDC tree's (width, height, focal): tests/common.py asymmetric_ndc_case
NARROW_BBOX = (0.1, 0.2, 0.0, 0.8, 0.9, 0.7)


@functools.lru_cache(maxsize=None)
def lib():
    L = build_util.c_library("order_restatement.c", oracle=True)
    L.order_keys.restype = C.c_int
    L.order_keys.argtypes = [C.POINTER(ob.OrTree), C.POINTER(ob.OrOptions), C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                             C.c_int, C.c_void_p, C.c_void_p]
    L.order_quantise.restype = C.c_uint32
    L.order_quantise.argtypes = [C.c_float, C.c_int]
    return L


def keys_of(tree, origins, dirs, bits, fp_mode=0, ndc=None, N=None, segments=False, **opt_kw):
    """The unsorted keys (uint32 [n]) of the rays; ``N``: overrides the tree's branching factor (N <= 0: no ray is
    drawn); segments: also the [n, 6] entry / exit coordinates the keys were cut from."""
    th = ob.TreeHandle(tree, ndc=ndc)
    if N is not None:
        th.struct.N = N
    opt = ob.default_options(**opt_kw)
    origins, dirs = (np.ascontiguousarray(a, np.float32) for a in (origins, dirs))
    n = origins.shape[0]
    assert origins.shape == dirs.shape == (n, 3)
    keys = np.zeros(n, np.uint32)
    seg = np.zeros((n, 6), np.float32)
    rc = lib().order_keys(C.byref(th.struct), C.byref(opt), fp_mode, n, origins.ctypes.data, dirs.ctypes.data,
                          DEFAULT_BITS if bits == 0 else bits, keys.ctypes.data, seg.ctypes.data)
    assert rc == 0
    return (keys, seg) if segments else keys


def result_of(keys):
    """The result rule: -> (order, sorted keys), order = the stable sort of 0..n-1 by key."""
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    return order, keys[order]


def morton(q, bits):
    """The key of six quantised coordinates, spelt out: bit 6 b + c = bit b of coordinate c."""
    key = 0
    for b in range(bits):
        for c in range(6):
            key |= ((int(q[c]) >> b) & 1) << (6 * b + c)
    return key


def unit_tree(depth=4, basis_dim=4, seed=21):
    """A small scene whose tree coordinates are the world's: offset 0, scale 1."""
    return dataclasses.replace(common.small_scene(depth=depth, basis_dim=basis_dim, seed=seed),
                               offset=np.zeros(3, np.float32), invradius3=np.ones(3, np.float32))


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (tree, ndc, option kwargs): "plain" (an SH4 small scene), "bbox" (the same under a narrowed render_bbox),
    "ndc" (the asymmetric NDC tree of tests/common.py)."""
    if name == "ndc":
        tree = common.asymmetric_ndc_case(4)[0]
        return tree, NDC, {}
    tree = common.small_scene(depth=5, basis_dim=4, seed=77)
    return tree, None, (dict(render_bbox=NARROW_BBOX) if name == "bbox" else {})


@functools.lru_cache(maxsize=None)
def rays(name, n, seed=3):
    """n seeded rays for a scene, read-only: arbitrary_rays (some miss); an NDC tree gets forward-facing rays from
    in front of its near plane."""
    tree, ndc, _ = scene(name)
    if ndc is None:
        o, d = ru.arbitrary_rays(tree, max(n, 600), seed)
    else:
        rng = np.random.default_rng(seed)
        m = max(n, 1)
        o = np.stack([rng.uniform(-0.6, 0.6, m), rng.uniform(-0.4, 0.4, m), rng.uniform(-0.2, 0.4, m)], 1)
        d = np.stack([rng.uniform(-0.9, 0.9, m), rng.uniform(-0.9, 0.9, m), -rng.uniform(0.5, 2.0, m)], 1)
        o, d = o.astype(np.float32), d.astype(np.float32)
    o, d = np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n])
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


@functools.lru_cache(maxsize=None)
def reference(name, n, bits, fp_mode):
    """The restatement's unsorted keys of rays(name, n), computed once and read-only."""
    tree, ndc, kw = scene(name)
    o, d = rays(name, n)
    keys = keys_of(tree, o, d, bits, fp_mode, ndc=ndc, **kw)
    keys.setflags(write=False)
    return keys
