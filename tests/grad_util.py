"""Helpers of the vr_render_backward tests: the record of the hits of the C restatement of the march with the
derivative's formulas on it (tests/cpp/grad_restatement.c over march_restatement.h), and the cases the CPU and
GPU tests share.  Scenes and option sets are those of tests/aov_util.py."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from tests import aov_util as au
from tests import build_util, common
from tests.common import ob

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


@functools.lru_cache(maxsize=None)
def lib(mutant=0):
    """The restatement; mutant = 1..3 builds it with -DGRAD_MUTANT (one deliberate mistake in grad_eval32, see the
    source), for the tests that show the error unit sees the mistake."""
    L = build_util.c_library("grad_restatement.c", (f"-DGRAD_MUTANT={mutant}",))
    L.grad_trace_frame.restype = C.c_void_p
    L.grad_trace_frame.argtypes = [C.POINTER(ob.OrTree), C.POINTER(ob.OrCamera), C.POINTER(ob.OrOptions), C.c_int]
    L.grad_trace_free.restype = None
    L.grad_trace_free.argtypes = [C.c_void_p]
    L.grad_trace_rays.restype = None
    L.grad_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.grad_trace_entered.restype = None
    L.grad_trace_entered.argtypes = [C.c_void_p, C.c_void_p]
    L.grad_trace_slots.restype = None
    L.grad_trace_slots.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.grad_trace_all_slots.restype = None
    L.grad_trace_all_slots.argtypes = [C.c_void_p, C.c_void_p]
    L.grad_eval64.restype = C.c_int
    L.grad_eval64.argtypes = [C.c_void_p] + [C.c_void_p] * 7
    L.grad_edge64.restype = C.c_int
    L.grad_edge64.argtypes = [C.c_void_p] * 5
    L.grad_eval32.restype = C.c_int
    L.grad_eval32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return L


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
        self._free = lib().grad_trace_free      # (kept here: module globals may be gone when __del__ runs)
        self.ptr = lib().grad_trace_frame(C.byref(th.struct), C.byref(cam), C.byref(opt), fp_mode)
        assert self.ptr
        self.n_hits = np.zeros(w * h, np.int64)
        stopped = np.zeros(w * h, np.uint8)
        lib().grad_trace_rays(self.ptr, _p(self.n_hits), _p(stopped))
        self.stopped = stopped.astype(bool)
        entered = np.zeros(w * h, np.uint8)
        lib().grad_trace_entered(self.ptr, _p(entered))
        self.entered = entered.astype(bool)      # the ray passed the ray/box test: the device marches it

    def __del__(self):
        if getattr(self, "ptr", None):
            self._free(self.ptr)
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

    def all_slots(self):
        """-> (slot of every hit, ray after ray; the ray of every hit), int64."""
        out = np.zeros(int(self.n_hits.sum()), np.int64)
        lib().grad_trace_all_slots(self.ptr, _p(out))
        return out, np.repeat(np.arange(self.n_hits.size), self.n_hits)

    def edge64(self, data64, g64, mag_c, under_c):
        """Adds the frame's edge-aware magnitudes M_c and U_c into mag_c / under_c (float64, the shape of data)."""
        g64 = np.ascontiguousarray(g64, np.float64)
        assert g64.shape == (self.h, self.w, 4) and data64.dtype == np.float64 and data64.flags.c_contiguous
        assert mag_c.shape == self.shape and under_c.shape == self.shape
        assert lib().grad_edge64(self.ptr, _p(data64), _p(g64), _p(mag_c), _p(under_c)) == 0
        return mag_c, under_c

    def loss64(self, data64, g64):
        """sum(g * out): the scalar whose derivative backward64 claims to be."""
        return float((self.forward64(data64)[0] * g64).sum())

    def backward32(self, data32, g32, order, grad32, mutant=0):
        g32 = np.ascontiguousarray(g32, np.float32)
        order = np.ascontiguousarray(order, np.int64)
        assert data32.dtype == np.float32 and grad32.dtype == np.float32 and grad32.shape == self.shape
        assert lib(mutant).grad_eval32(self.ptr, _p(data32), _p(g32), _p(order), order.size, _p(grad32)) == 0
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
    if name.startswith("renum_"):   # a scene of tests/renumber_util.py, pruned, in its own numbering
        from tests import renumber_util as rn
        return rn.case(name[6:], ("pruned",))["orig"], 4.0, None
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


# The cases of tests/test_gpu_sched.py, where every wave of the backward march takes several chunks: 8 poses at
# 96 x 96, so up to four times the contributions per element of the cases above.
# (tree, size, poses, option set, gkind, FP models).  Their summation constant, measured like K32
# (tests/test_grad_restatement.py::test_summation_constant_of_the_scheduling_cases): 13.855 (sh9_near without
# early stop, strict, either order; every other case 2.1-5.1).  That is below K32, so the cases use K and K_EDGE
# unchanged.
NO_STOP = (("stop_thresh", 0.0),)
SCHED_POSES, SCHED_SIZE = 8, 96
SCHED_CASES = [("sh16", SCHED_SIZE, SCHED_POSES, "default", "normal", (0, 1)),
               ("sh16", SCHED_SIZE, SCHED_POSES, "default", "alpha", (0,)),
               ("sh9_near", SCHED_SIZE, SCHED_POSES, "default", "normal", (0,)),
               ("sh9_near", SCHED_SIZE, SCHED_POSES, NO_STOP, "normal", (0,)),
               ("sh25", SCHED_SIZE, SCHED_POSES, "default", "normal", (0,)),
               ("rgba", SCHED_SIZE, SCHED_POSES, "default", "normal", (0,)),
               ("basis1", SCHED_SIZE, SCHED_POSES, "default", "normal", (0,)),
               ("n4", SCHED_SIZE, SCHED_POSES, "default", "normal", (0,))]
SCHED_K32_MEASURED = 13.855


def entering(ref):
    """Rays of the views of ``ref`` that enter the volume -- the rays a march launch hands to its waves -- and
    those among them without a hit sample -> (int, int)."""
    return (sum(int(t.entered.sum()) for t in ref["traces"]),
            sum(int((t.entered & (t.n_hits == 0)).sum()) for t in ref["traces"]))


def hit_slots(ref, rays=None):
    """bool [n_slots]: the slots a hit sample of the views of ``ref`` falls into (of the rays ``rays``, indices
    into the frames' pixels frame after frame, when given) -- what a marked backward call must mark, exactly."""
    dd = ref["grad"].shape[-1]
    hit = np.zeros(ref["grad"].size // dd, bool)
    keep = None
    if rays is not None:
        keep = np.zeros(len(ref["traces"]) * ref["w"] * ref["h"], bool)
        keep[rays] = True
    for i, t in enumerate(ref["traces"]):
        slots, ray = t.all_slots()
        hit[slots if keep is None else slots[keep[i * ref["w"] * ref["h"] + ray]]] = True
    return hit


def mark_words(hit):
    """The ``touched`` bitmap of a slot mask: bit s & 31 of word s >> 5, uint32."""
    padded = np.zeros((hit.size + 31) // 32 * 32, np.uint8)
    padded[:hit.size] = hit
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


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


# ---- the value domain: saturated colours, edge densities, non-finite rays -----------------------------------------
# unit() cannot judge a record whose sigmoid argument u is tens of units: the binary32 dot product u carries an
# absolute error of ~2^-24 sum_b |B_b k_b|, which is the relative error of exp(-u), and binary32 flushes a colour to
# 0 where binary64 keeps 1e-48.  unit_edge() covers both (M_c, U_c: tests/cpp/grad_restatement.c).
# The edge summation constant (tests/test_grad_restatement.py::test_edge_summation_constant measures it): the
# largest |binary32 - binary64| / unit_edge() of the restatement's binary32 entry point over the clean elements of
# every edge case below, both catalogues, in scanline and in shuffled ray order: 28.996 (rgba_never_stop, finite
# catalogue; the SH cases come to 1.3-3.8 with the default options and to 16.4 with stop_thresh = 0), rounded up.
# K_EDGE = 4 * K32_EDGE by the rule of K.  If the GPU exceeds K_EDGE, that is a finding about the kernel: K_EDGE
# does not move.
K32_EDGE = 29.0
K_EDGE = 4.0 * K32_EDGE


def _finite_bits(cat):
    return [b for b in cat if (b & 0x7C00) != 0x7C00]


def _half_bits(v):
    return int(np.float16(v).view(np.uint16))


# finite: the three catalogues of tests/common.py without NaN and +-inf, plus coefficients +-40 (|u| ~ 11 through
# basis 0) and +-200; full: the catalogues as they are (and grad_accum non-finite in about 1 % of the pixels)
CATALOGUES = {
    "finite": dict(coeff=_finite_bits(common.EDGE_COEFF) + [_half_bits(v) for v in (40, -40, 200, -200)],
                   rgba_colours=_finite_bits(common.EDGE_RGBA), sigmas=_finite_bits(common.EDGE_SIGMA)),
    "full": {},
}

# name -> dict(fmt, basis_dim, opt, fp_modes, frac (finite, full): the share of the leaf records that get special
# values, chosen per case so that the cap of tests/test_grad_restatement.py::test_edge_cap holds; camera "orbit" |
# "axis"; tree "edge" (a depth-`depth` value_edge_tree) | "n4" (the generic descent))
EDGE_CASES = {
    "sh16": dict(fmt="SH", basis_dim=16, opt={}, fp_modes=(0, 1), frac=(0.08, 0.08)),
    "sh16_no_stop": dict(fmt="SH", basis_dim=16, opt=dict(stop_thresh=0.0), fp_modes=(0, 1), frac=(0.08, 0.02)),
    "sh16_stop_ge_1": dict(fmt="SH", basis_dim=16, opt=dict(stop_thresh=1.5), fp_modes=(0, 1), frac=(0.08, 0.08)),
    "sh25": dict(fmt="SH", basis_dim=25, opt={}, fp_modes=(0,), frac=(0.08, 0.08)),
    "sh9_thresh_edge": dict(fmt="SH", basis_dim=9, opt=dict(sigma_thresh=0.5), fp_modes=(0,), frac=(0.08, 0.08)),
    "sh4_negative_thresh": dict(fmt="SH", basis_dim=4, opt=dict(sigma_thresh=-1.0), fp_modes=(0,), frac=(0.08, 0.04)),
    "basis1": dict(fmt="SH", basis_dim=3, opt={}, fp_modes=(0,), frac=(0.08, 0.08)),
    "rgba": dict(fmt="RGBA", basis_dim=-1, opt={}, fp_modes=(0,), frac=(0.08, 0.08)),
    "rgba_never_stop": dict(fmt="RGBA", basis_dim=-1, opt=dict(stop_thresh=-0.5), fp_modes=(0,), frac=(0.08, 0.01)),
    "rgba_stop_ge_1": dict(fmt="RGBA", basis_dim=-1, opt=dict(stop_thresh=1.0), fp_modes=(0,), frac=(0.08, 0.08),
                           camera="axis"),
    "n4": dict(tree="n4", opt={}, fp_modes=(0,), frac=(0.08, 0.08), size=40),
    "blocked": dict(fmt="SH", basis_dim=4, depth=7, opt={}, fp_modes=(0,), frac=(0.08, 0.08), blocked=True),
}
EDGE_RUNS = [(n, fp) for n, c in EDGE_CASES.items() for fp in c["fp_modes"]]
EDGE_IDS = [f"{n}-fp{fp}" for n, fp in EDGE_RUNS]


@functools.lru_cache(maxsize=None)
def edge_tree(name, catalogue):
    c = EDGE_CASES[name]
    seed = 7100 + sum(map(ord, name))
    frac = c["frac"][0 if catalogue == "finite" else 1]
    if c.get("tree") == "n4":
        return common.apply_value_edges(common.random_tree_general_n(), seed + 1, frac, **CATALOGUES[catalogue])
    return common.value_edge_tree(c["fmt"], c["basis_dim"], seed=seed, depth=c.get("depth", 5), frac=frac,
                                  **CATALOGUES[catalogue])


def edge_view(name):
    """-> (transform, w, h, focal): one pose, 56 x 56 (57 x 57 for the axis camera, whose centre row and column
    need an odd size; 40 x 40 for the generic descent)."""
    c = EDGE_CASES[name]
    size = c.get("size", 56)
    if c.get("camera") == "axis":
        return common.axis_camera(size | 1)
    return common.camera_for(pose_idx=(7100 + sum(map(ord, name))) % 8, size=size)


def edge_upstream(catalogue, h, w, seed=7):
    """grad_accum [1, h, w, 4]: upstream("normal"); in the full catalogue about 1 % of the pixels hold NaN, +inf or
    -inf in one of their four entries."""
    g = upstream("normal", 1, h, w, seed=seed).copy()
    if catalogue == "full":
        rng = np.random.default_rng(seed + 1)
        ys, xs = np.nonzero(rng.random((h, w)) < 0.01)
        for y, x in zip(ys, xs):
            g[0, y, x, int(rng.integers(4))] = (np.nan, np.inf, -np.inf)[int(rng.integers(3))]
    return g


@functools.lru_cache(maxsize=None)
def edge_reference(name, catalogue, fp_mode):
    """The float64 gradient of one edge case, its magnitudes and its clean mask, once per session and read-only.
    -> the dict of reference() plus mag_c, under_c and, per slot (bool [n_slots]): hit (a hit sample fell into it),
    dirty (a dirty ray hit it), clean (hit and not dirty).  A ray is dirty if a slot it hits holds a non-finite
    value, if its grad_accum pixel is non-finite, or if the oracle's binary32 forward of its pixel (accumulators,
    transmittance) is non-finite -- finite records that overflow in binary32: att = inf from sigma = -65504,
    s = 1 / 0 when stop_thresh >= 1 meets an att that rounds to 1."""
    c = EDGE_CASES[name]
    tree = edge_tree(name, catalogue)
    tr, w, h, f = edge_view(name)
    kw = dict(c["opt"])
    g = edge_upstream(catalogue, h, w)
    d64 = data64_of(tree)
    grad, mag, under, mag_c, under_c = (np.zeros(d64.shape, np.float64) for _ in range(5))
    t = Trace(tree, tr, w, h, f, fp_mode, **kw)
    g64 = g[0].astype(np.float64)
    t.backward64(d64, g64, grad, mag, under)
    t.edge64(d64, g64, mag_c, under_c)
    # the clean mask
    dd = tree.data_dim
    n_slots = d64.size // dd
    slots, ray_of_hit = t.all_slots()
    bad_record = ~np.isfinite(d64.reshape(n_slots, dd)).all(1)
    _, acc, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode, **kw)
    _, T, _, _ = au.restate(tree, tr, w, h, f, fp_mode, **kw)
    dirty_ray = ~np.isfinite(g[0]).all(-1).reshape(-1) | ~np.isfinite(acc).all(-1).reshape(-1) | \
        ~np.isfinite(T).reshape(-1)
    dirty_ray[ray_of_hit[bad_record[slots]]] = True
    hit, dirty = np.zeros(n_slots, bool), np.zeros(n_slots, bool)
    hit[slots] = True
    dirty[slots[dirty_ray[ray_of_hit]]] = True
    clean = hit & ~dirty
    for a in (g, grad, mag, under, mag_c, under_c, hit, dirty, clean):
        a.setflags(write=False)
    return dict(tree=tree, ndc=None, trs=[tr], w=w, h=h, f=f, g=g, grad=grad, mag=mag, under=under, mag_c=mag_c,
                under_c=under_c, traces=[t], opt=kw, hit=hit, dirty=dirty, clean=clean,
                dirty_rays=int((dirty_ray & (t.n_hits > 0)).sum()), blocked=bool(c.get("blocked")))


def unit_edge(ref):
    """The edge-aware error unit per element: 2^-24 M_c + 2^-126 U_c."""
    return EPS32 * ref["mag_c"] + TINY32 * ref["under_c"]


def clean_elements(ref):
    """bool, the shape of data: the elements of the clean slots."""
    dd = ref["grad"].shape[-1]
    return np.broadcast_to(ref["clean"][:, None], (ref["clean"].size, dd)).reshape(ref["grad"].shape)


def worst_edge_ratio(got, ref, start=None, slack=None):
    """max (|got - start - grad| - slack) / unit_edge over the clean elements with M > 0, their number, and whether
    the clean elements with M == 0 hold the bits of `start` (zeros when None)."""
    start = np.zeros(ref["grad"].shape, np.float32) if start is None else start
    clean = clean_elements(ref)
    pos = clean & (np.nan_to_num(ref["mag"], nan=0.0) > 0)
    with np.errstate(invalid="ignore"):
        diff = np.abs(np.asarray(got, np.float64) - start.astype(np.float64) - ref["grad"])
        if slack is not None:
            diff = np.maximum(diff - slack, 0.0)
    ratio = float((diff[pos] / unit_edge(ref)[pos]).max()) if pos.any() else 0.0
    zero = clean & ~pos
    same = np.asarray(got, np.float32).view(np.uint32)[zero] == start.view(np.uint32)[zero]
    return ratio, int(pos.sum()), bool(same.all())


# ---- shared by the GPU tests (torch is handed in: the module imports without it) -----------------------------------
def sentinel(shape):
    """Finite, non-zero, different from element to element: x + 0 == x bit for bit, and a write shows."""
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.int64) % 251 + 1).astype(np.float32) * np.float32(2.0 ** -40)).reshape(shape)


def upload(ref, name=None):
    from volrend_amd import api
    blocked = name == "blocked"
    if blocked:
        api.set_tuning(top_levels=2, brick_levels=3, brick_blocked=1)
    try:
        t = api.N3Tree.from_synth(ref["tree"], ndc=ref["ndc"])
    finally:
        if blocked:
            api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    if blocked:
        assert t.info()["brick_blocked"] == 1
    return t


def assert_parity(got, ref, start=None, k=K, what=""):
    """Every element: |got - start - grad| <= k * unit; elements with M == 0 keep the bits of `start`."""
    start = np.zeros(ref["grad"].shape, np.float32) if start is None else start
    diff = np.abs(got.astype(np.float64) - start.astype(np.float64) - ref["grad"])
    u = unit(ref)
    pos = ref["mag"] > 0
    # (a buffer that starts from `start` rounds every add relative to a running value that holds it: 2^-24
    # |start| per contribution at most, and U * 2^20 bounds their number -- every contribution adds 2^-20 to U)
    slack = ref["under"] * 2.0 ** 20 * EPS32 * np.abs(start.astype(np.float64))
    worst = float((np.maximum(diff - slack, 0.0)[pos] / u[pos]).max())
    print(f"{what}: worst |gpu - f64| / unit = {worst:.3f} of {k} over {int(pos.sum())} elements")
    assert worst <= k, what
    same = got.view(np.uint32) == start.view(np.uint32)
    assert same[~pos].all(), f"{what}: {int((~same[~pos]).sum())} elements nothing touches were written"


def upload_edge(ref):
    return upload(ref, "blocked" if ref["blocked"] else None)


def assert_edge_parity(got, ref, start=None, what=""):
    """An edge case (EDGE_CASES): clean elements with M > 0 within K_EDGE * unit_edge (plus the slack of
    assert_parity for a buffer that starts from `start`), clean elements with M == 0 and every slot no ray hits
    -- interior slots included -- bit-identical to `start`.  Dirty slots are not looked at."""
    start = np.zeros(ref["grad"].shape, np.float32) if start is None else start
    with np.errstate(invalid="ignore"):
        slack = ref["under"] * 2.0 ** 20 * EPS32 * np.abs(start.astype(np.float64))
    worst, n, zeros_same = worst_edge_ratio(got, ref, start, slack)
    print(f"{what}: worst |gpu - f64| / unit_edge = {worst:.3f} of {K_EDGE} over {n} clean elements; "
          f"{int(ref['dirty'].sum())} of {int(ref['hit'].sum())} hit slots dirty")
    assert n >= 200, "the case shows nothing"
    assert worst <= K_EDGE, what
    assert zeros_same, f"{what}: a clean element with M == 0 was written"
    dd = ref["grad"].shape[-1]
    same = (got.view(np.uint32) == start.view(np.uint32)).reshape(-1, dd)
    assert same[~ref["hit"]].all(), f"{what}: {int((~same[~ref['hit']]).any(1).sum())} slots no ray hits were written"
    interior = np.asarray(ref["tree"].child).reshape(-1) != 0
    assert interior.any() and not ref["hit"][interior].any()
    return worst


def assert_contained(got, ref, start, what=""):
    """assert_edge_parity, and the case shows something: a dirty slot holds a non-finite value afterwards."""
    assert_edge_parity(got, ref, start, what)
    dd = ref["grad"].shape[-1]
    assert ref["dirty"].any() and not np.isfinite(got.reshape(-1, dd)[ref["dirty"]]).all(), \
        f"{what}: no dirty slot holds a non-finite value"
