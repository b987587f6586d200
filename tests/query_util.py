"""Helpers of the point-query tests (tests/test_query_host.py, tests/test_gpu_query.py): the
oracle's answers for many points, the colour of a sample recomposed from the oracle's own pieces,
and seeded point sets."""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import binding as ob
from tests import common

HI = np.float32(1.0) - np.float32(1e-6)   # the clamp's upper end, 1 - 1e-6f

_h2f = None


def half_table():
    """or_half2float of all 65536 bit patterns."""
    global _h2f
    if _h2f is None:
        L = ob.lib()
        _h2f = np.array([L.or_half2float(h) for h in range(65536)], np.float32)
    return _h2f


def records(tree):
    """[n_slots, data_dim] float32: every record of the tree through or_half2float."""
    return half_table()[np.ascontiguousarray(tree.data).reshape(-1, tree.data_dim).view(np.uint16)]


def oracle_query(th, pts_tree):
    """or_query point by point -> dict(leaf int64 [n], depth int32 [n], local float32 [n, 3])."""
    L = ob.lib()
    pts = np.ascontiguousarray(pts_tree, np.float32)
    n = pts.shape[0]
    leaf = np.zeros(n, np.int64)
    depth = np.zeros(n, np.int32)
    local = np.zeros((n, 3), np.float32)
    xyz, cube, d = (C.c_float * 3)(), C.c_float(), C.c_int()
    fn, ts, px, pc, pd = L.or_query, C.byref(th.struct), C.byref(xyz), C.byref(cube), C.byref(d)
    for i in range(n):
        xyz[0], xyz[1], xyz[2] = pts[i]
        leaf[i] = fn(ts, px, pc, pd)
        depth[i] = d.value
        local[i] = xyz[0], xyz[1], xyz[2]
    return dict(leaf=leaf, depth=depth, local=local)


def oracle_answers(tree, th, pts, space):
    """What vr_query_points must return for ``pts``: sigma, depth, local, coeffs (all float32 / int32
    numpy) -- or_query on the tree coordinate (for world points offset + scale * x in float32, one
    rounding per operator, as or_probe_coeffs forms it)."""
    pts = np.ascontiguousarray(pts, np.float32)
    if space == "world":
        offset, scale = np.array(th.struct.offset[:], np.float32), np.array(th.struct.scale[:], np.float32)
        with np.errstate(all="ignore"):
            pts = offset[None, :] + scale[None, :] * pts
    q = oracle_query(th, pts)
    rec = records(tree)[q["leaf"]]
    return dict(sigma=rec[:, -1].copy(), depth=q["depth"], local=q["local"], coeffs=rec[:, :-1].copy(),
                leaf=q["leaf"])


def probe_coeffs(th, tree, pts_world):
    """or_probe_coeffs point by point -> float32 [n, data_dim - 1]."""
    L = ob.lib()
    pts = np.ascontiguousarray(pts_world, np.float32)
    out = np.zeros((pts.shape[0], tree.data_dim - 1), np.float32)
    opt = ob.default_options(enable_probe=1)
    row = np.zeros(tree.data_dim - 1, np.float32)
    for i in range(pts.shape[0]):
        opt.probe[0], opt.probe[1], opt.probe[2] = pts[i]
        L.or_probe_coeffs(C.byref(th.struct), C.byref(opt), row.ctypes.data)
        out[i] = row
    return out


def basis_of(th, dirs):
    """or_basis (strict) of every direction -> float32 [n, 25]."""
    L = ob.lib()
    dirs = np.ascontiguousarray(dirs, np.float32)
    out = np.zeros((dirs.shape[0], 25), np.float32)
    d, b = (C.c_float * 3)(), (C.c_float * 25)()
    for i in range(dirs.shape[0]):
        d[0], d[1], d[2] = dirs[i]
        L.or_basis(C.byref(th.struct), C.byref(d), ob.FP_STRICT, C.byref(b))
        out[i] = b[:]
    return out


def expf(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    ob.lib().or_expf_n(x.ctypes.data, out.ctypes.data, x.size)
    return out


def recompose_rgb(tree, th, coeffs, dirs):
    """The colour of a sample (rt_core.cuh:125-171 with weight 1) from the oracle's pieces: or_basis
    of the direction as given, the record as or_half2float left it (``coeffs`` float32
    [n, data_dim - 1]), the sum of rt_core.cuh:130-161 in float32 -- basis 0 first, then the groups
    of 25, 16, 9 and 4, each summed left to right before it is added -- and or_expf.
    RGBA trees: the first three entries of the record."""
    coeffs = np.ascontiguousarray(coeffs, np.float32)
    if tree.format_name == "RGBA":
        return coeffs[:, :3].copy()
    assert tree.format_name == "SH"
    B = tree.basis_dim
    basis = basis_of(th, dirs)
    out = np.zeros((coeffs.shape[0], 3), np.float32)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        for c in range(3):
            v = coeffs[:, c * B:(c + 1) * B]
            tmp = basis[:, 0] * v[:, 0]
            for size, lo, hi in ((25, 16, 24), (16, 9, 15), (9, 4, 8), (4, 1, 3)):
                if B in (25, 16, 9, 4) and B >= size:
                    g = basis[:, lo] * v[:, lo]
                    for i in range(lo + 1, hi + 1):
                        g = g + basis[:, i] * v[:, i]
                    tmp = tmp + g
            out[:, c] = one / (one + expf(-tmp))
    return out


def pixel_dirs(w, h, fx, fy):
    """View directions of an identity-rotation camera (volrend.cu:22-32, common.cuh _normalize):
    (x, y, -1) * (1 / sqrtf(x*x + y*y + 1)) with x = (ix - 0.5f W) / fx, y = -(iy - 0.5f H) / fy,
    in float32, [h, w, 3]."""
    f32 = np.float32
    ix, iy = np.meshgrid(np.arange(w), np.arange(h))
    x = (ix.astype(f32) - f32(0.5) * f32(w)) / f32(fx)
    y = -(iy.astype(f32) - f32(0.5) * f32(h)) / f32(fy)
    z = np.full_like(x, -1.0)
    inv = f32(1.0) / np.sqrt(z * z + (x * x + y * y))
    return np.stack([x * inv, y * inv, z * inv], -1).astype(f32)


def one_sample_tree(basis_dim, fmt="SH", seed=0):
    """A depth-1 tree whose 8 leaves hold the same record with sigma = 60000: the first sample of
    every ray that enters the volume is opaque, so or_render's accumulator IS that sample's colour."""
    from volrend_amd import synth
    rng = np.random.default_rng(seed)
    dd = 4 if fmt == "RGBA" else 3 * basis_dim + 1
    rec = (rng.standard_normal(dd) * 0.6).astype(np.float32)
    if fmt == "RGBA":
        rec[:3] = rng.uniform(0.05, 0.95, 3)
    rec[-1] = 60000.0
    data = np.broadcast_to(rec.astype(np.float16), (1, 2, 2, 2, dd)).copy()
    name = "RGBA" if fmt == "RGBA" else f"{fmt}{basis_dim}"
    return synth.SynthTree(np.zeros((1, 2, 2, 2), np.int32), data, np.full(3, 0.5, np.float32),
                           np.full(3, np.float32(1 / 3), np.float32), name, None, 1)   # world radius 1.5


def leaf_boxes(tree):
    """(corner float64 [m, 3], size float64 [m], depth [m] as or_query counts it, slot index [m]) of
    every leaf, in tree coordinates."""
    N = tree.N
    N3 = N ** 3
    child = tree.child.reshape(-1, N3)
    corners, sizes, depths, slots = [], [], [], []
    stack = [(0, np.zeros(3), 1.0, 0)]
    while stack:
        node, corner, size, d = stack.pop()
        s = size / N
        for k in range(N3):
            c = corner + s * np.array([k // (N * N), (k // N) % N, k % N], np.float64)
            if child[node, k] == 0:
                corners.append(c)
                sizes.append(s)
                depths.append(d)
                slots.append(node * N3 + k)
            else:
                stack.append((node + int(child[node, k]), c, s, d + 1))
    return np.array(corners), np.array(sizes), np.array(depths), np.array(slots)


def point_set(tree, n, seed, jitter=0.6, by_depth=False):
    """Tree coordinates float32 [n, 3]: half uniform over [0, 1)^3, half jittered centres (+- jitter of
    the leaf's size) of occupied leaves -- or, ``by_depth``, of leaves drawn evenly over the depths
    present, occupied or not (trees whose deep leaves uniform points cannot find)."""
    rng = np.random.default_rng(seed)
    corners, sizes, depths, slots = leaf_boxes(tree)
    sigma = tree.data.reshape(-1, tree.data_dim)[slots, -1].astype(np.float32)
    half = n // 2
    uni = rng.random((n - half, 3))
    if by_depth:
        present = np.unique(depths)
        pick_d = present[rng.integers(present.size, size=half)]
        order = np.argsort(depths, kind="stable")
        first = np.searchsorted(depths[order], present)
        count = np.diff(np.append(first, depths.size))
        at = np.searchsorted(present, pick_d)
        pick = order[first[at] + (rng.random(half) * count[at]).astype(np.int64)]
        # (occupied leaves twice as likely where a depth has some: the sigma > 0 quarter)
        occ = np.flatnonzero(sigma > 0)
        swap = rng.random(half) < 0.5
        pick = np.where(swap, occ[rng.integers(occ.size, size=half)], pick)
    else:
        occ = np.flatnonzero(sigma > 0)
        pick = occ[rng.integers(occ.size, size=half)]
    jit = (rng.random((half, 3)) * 2 - 1) * jitter
    cen = corners[pick] + sizes[pick, None] * (0.5 + jit)
    return np.concatenate([uni, cen]).astype(np.float32)


def to_world(tree, pts_tree):
    """World points whose tree coordinate is about ``pts_tree`` (the tests take whatever tree
    coordinate offset + scale * x rounds to)."""
    return ((pts_tree.astype(np.float64) - tree.offset.astype(np.float64)) /
            tree.invradius3.astype(np.float64)).astype(np.float32)


def check_point_set(tree, ans, what=""):
    """The conditions on a point set, on the ORACLE's answers: at least a quarter of the points in
    leaves with sigma > 0, and every leaf depth of the tree hit."""
    frac = float((ans["sigma"] > 0).mean())
    assert frac >= 0.25, f"{what}: only {frac:.2f} of the points fall in leaves with sigma > 0"
    present = set(np.unique(leaf_boxes(tree)[2]).tolist())
    hit = set(np.unique(ans["depth"]).tolist())
    assert hit == present, f"{what}: leaf depths {sorted(present - hit)} are never hit"
    return frac


# ---- the point sets and checks the CPU and GPU tests share ----------------------------------------------------------
# name -> (tree factory, seed of the point set, points by depth); the seeds were chosen on the CPU so
# that the oracle alone meets the conditions of query_util.check_point_set
# (tests/test_query_host.py::test_point_sets_meet_their_conditions_on_the_oracle)
POINT_TREES = {
    "SH4_d5": (lambda: common.small_scene(depth=5, basis_dim=4, seed=11), 101, False),
    "SH16_d6": (lambda: common.small_scene(depth=6, basis_dim=16, seed=12), 102, False),
    "SH1": (lambda: common.small_scene(depth=5, basis_dim=1, seed=13), 103, False),
    "SH9": (lambda: common.small_scene(depth=5, basis_dim=9, seed=14), 104, False),
    "SH25": (lambda: common.small_scene(depth=5, basis_dim=25, seed=15), 105, False),
    "RGBA": (lambda: common.small_scene(depth=5, basis_dim=0, fmt="RGBA", seed=16), 106, False),
    "SG7": (lambda: common.small_scene(depth=5, basis_dim=7, fmt="SG", seed=17), 107, False),
    "ASG4": (lambda: common.small_scene(depth=5, basis_dim=4, fmt="ASG", seed=18), 108, False),
    "edge_SH9": (lambda: common.value_edge_tree("SH", 9, seed=3), 109, False),
    "fog_SH16": (lambda: common.fog_tree("SH", 16, seed=5, depth=5), 110, False),
    "N3": (lambda: common.random_tree_general_n(N=3, depth=4, basis_dim=4, seed=21), 111, False),
    "N4": (lambda: common.random_tree_general_n(N=4, depth=3, basis_dim=9, seed=22), 112, False),
    "chain28": (lambda: common.deep_chain_tree_n2(28, basis_dim=4, seed=2)[0], 113, True),
}


def make_point_tree(name, n=100_000):
    factory, seed, by_depth = POINT_TREES[name]
    tree = factory()
    return tree, point_set(tree, n, seed, by_depth=by_depth)


def same_words(got, want, what):
    """Bit equality of 32-bit words; a NaN must meet a NaN (any payload)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    if got.dtype == np.float32:
        ng, nw = np.isnan(got), np.isnan(want)
        assert np.array_equal(ng, nw), f"{what}: NaN in {int((ng & ~nw).sum())} kernel / {int((nw & ~ng).sum())} oracle words only"
        diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nw
    else:
        diff = got != want
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ (first at {np.argwhere(diff)[0].tolist()})"


def gpu_query(torch, t, pts, dirs=None, want=("sigma", "depth", "local", "coeffs"), space="tree", stream=None):
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
    d = None if dirs is None else torch.from_numpy(np.ascontiguousarray(dirs, np.float32)).cuda()
    out = t.query(p, d, want=want, space=space, stream=stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_against_oracle(torch, t, tree, th, pts, space, what, ans=None):
    ans = ans or oracle_answers(tree, th, pts, space)
    got = gpu_query(torch, t, pts, space=space)
    for k in ("sigma", "depth", "local", "coeffs"):
        same_words(got[k], ans[k], f"{what} {space} {k}")
    return ans


def direction_set(n, seed):
    """Unit vectors, un-normalised ones (x 0.3, x 3), exact axes and zero directions."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[1::4] *= 0.3
    d[2::4] *= 3.0
    d[3::64] = 0.0
    d[5::64] = (0.0, 0.0, -1.0)
    d[7::64] = (1.0, 0.0, 0.0)
    return d.astype(np.float32)


def grid_coords(lo, hi, res):
    """lo + ((float)i + 0.5f) * ((hi - lo) / (float)res) per axis in float32 -> [r0, r1, r2, 3]."""
    f32 = np.float32
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    ax = []
    for a in range(3):
        cell = (hi[a] - lo[a]) / f32(res[a])
        ax.append(lo[a] + (np.arange(res[a]).astype(f32) + f32(0.5)) * cell)
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    assert g.dtype == f32
    return np.ascontiguousarray(g)
