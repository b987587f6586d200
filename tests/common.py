"""Shared helpers for the parity tests: seeded scenes + oracle/kernel runners."""
from __future__ import annotations

import dataclasses
import hashlib
import json
import os

import numpy as np

from oracle import binding as ob
from volrend_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_ref_pins = {}


def _pins(name):
    if name not in _ref_pins:
        path = os.path.join(GOLDEN, name)
        _ref_pins[name] = json.load(open(path)) if name.endswith(".json") else np.load(path)
    return _ref_pins[name]


def digest(a) -> str:
    """SHA-256 of an array's dtype, shape and bytes."""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def _record(key, what, value):
    path = os.path.join(os.environ["VOLREND_RECORD_REF_PINS"], key.replace("/", "__") + what)
    if what == ".npy":
        np.save(path, value)
    else:
        open(path, "w").write(value)


def _live(available):
    return ob.ref_lib() is not None if available is None else available


def assert_ref_equal(key, got, live, available=None, msg=""):
    """``got`` equals output ``key`` of the reference's own code (its device code compiled for the
    host, oracle/_ref, or its GLSL backend) bit for bit.  The reference's output is stored as a
    SHA-256 digest in tests/golden/ref_pins_v1.json (tests/golden/make_ref_pins.py), so the pin holds
    where the reference is not built.  Where it is (``available``, default: the host build loads),
    ``live()`` recomputes the output and ``got`` must equal it as well.  With
    VOLREND_RECORD_REF_PINS=DIR the digest of ``live()`` is recorded into DIR (make_ref_pins.py)."""
    got = np.ascontiguousarray(got)
    recording = bool(os.environ.get("VOLREND_RECORD_REF_PINS"))
    if recording or _live(available):
        want = np.ascontiguousarray(live())
        assert want.dtype == got.dtype and want.shape == got.shape and want.tobytes() == got.tobytes(), \
            f"{key}: differs from the reference {msg}"
        if recording:
            _record(key, ".sha256", digest(want))
            return
    assert digest(got) == _pins("ref_pins_v1.json")[key], f"{key}: differs from the reference {msg}"


def ref_array(key, live, available=None):
    """Output ``key`` of the reference's code where a test computes with its values instead of testing
    equality: stored as it is in tests/golden/ref_frames_v1.npz.  Where the reference is available,
    ``live()`` recomputes it and must equal the stored copy."""
    if os.environ.get("VOLREND_RECORD_REF_PINS"):
        want = np.asarray(live())
        _record(key, ".npy", want)
        return want
    want = _pins("ref_frames_v1.npz")[key]
    if _live(available):
        got = np.asarray(live())
        assert got.dtype == want.dtype and np.array_equal(got, want), \
            f"{key}: the reference no longer reproduces its stored output (tests/golden/make_ref_pins.py)"
    return want


def small_scene(depth=5, basis_dim=16, fmt="SH", seed=11, **kw):
    tree = synth.make_tree(depth=depth, basis_dim=basis_dim, fmt=fmt, seed=seed, **kw)
    return tree


def camera_for(pose_idx=1, n_poses=8, size=96, focal=None, phi=-30.0, radius=4.0):
    poses = synth.make_poses(n_poses, phi_deg=phi, radius=radius)
    focal = focal if focal is not None else size * 1111.111 / 800.0
    return synth.c2w_to_transform(poses[pose_idx]), size, size, focal


def oracle_frame(tree, transform, w, h, focal, fp_mode=ob.FP_STRICT, ndc=None, region=None,
                 offscreen=True, rgba_init=None, depth_init=None, fy=None, **opt_kw):
    th = ob.TreeHandle(tree, ndc=ndc)
    cam = ob.make_camera(transform, w, h, focal, fy)
    opt = ob.default_options(**opt_kw)
    return ob.render(th, cam, opt, fp_mode, region=region, offscreen=offscreen,
                     rgba_init=rgba_init, depth_init=depth_init)


def ulp_diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in units-in-the-last-place between two float32 arrays."""
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


def random_tree_general_n(N=4, depth=3, basis_dim=4, fmt="SH", seed=0, p_refine=0.35,
                          p_occupied=0.5):
    """A random N^3-tree with arbitrary branching factor (the svox format allows any N;
    upstream warns 'N != 2 probably doesn't work', our kernels take the literal float
    descent for it).  Breadth-first numbering, relative child offsets."""
    from volrend_amd import synth
    rng = np.random.default_rng(seed)
    N3 = N ** 3
    data_dim = 4 if fmt == "RGBA" else 3 * basis_dim + 1
    levels = [1]
    child_rows = []
    n_total = 1
    for d in range(depth):
        n = levels[d]
        if d + 1 < depth:
            refine = rng.random((n, N3)) < p_refine
        else:
            refine = np.zeros((n, N3), dtype=bool)
        ids = np.zeros((n, N3), dtype=np.int64)
        k = int(refine.sum())
        ids[refine] = n_total + np.arange(k)
        n_total += k
        child_rows.append(ids)
        levels.append(k)
        if k == 0:
            break
    cap = n_total
    child = np.zeros((cap, N3), dtype=np.int32)
    base = 0
    for ids in child_rows:
        n = ids.shape[0]
        node = (base + np.arange(n))[:, None]
        child[base:base + n] = np.where(ids != 0, ids - node, 0)
        base += n
    data = np.zeros((cap, N3, data_dim), dtype=np.float32)
    occ = (rng.random((cap, N3)) < p_occupied) & (child == 0)
    data[..., :-1] = rng.standard_normal((cap, N3, data_dim - 1)) * 0.6
    if fmt == "RGBA":
        data[..., :3] = rng.uniform(0.05, 0.95, size=(cap, N3, 3))
    data[..., -1] = np.where(occ, np.exp(rng.uniform(np.log(2), np.log(60), size=(cap, N3))), 0)
    data[child != 0] = 0
    name = "RGBA" if fmt == "RGBA" else f"{fmt}{basis_dim}"
    return synth.SynthTree(child.reshape(cap, N, N, N),
                           data.astype(np.float16).reshape(cap, N, N, N, data_dim),
                           np.full(3, 0.5, np.float32), np.full(3, np.float32(1 / 3), np.float32),
                           name, None, depth)


def write_quantised_npz(tree, path, n_retain=1, compressed=True):
    """The compress_octree.py layout (reference scripts/compress_octree.py:106-119) of a
    synthetic tree: the first ``n_retain`` basis functions uncompressed, one exact
    codebook (all distinct RGB triples, <= 65536) per remaining basis function."""
    import numpy as np
    cap, dd = tree.capacity, tree.data_dim
    nb = (dd - 1) // 3
    data = tree.data.reshape(-1, dd)
    n_slots = data.shape[0]
    coeff = data[:, :-1].reshape(n_slots, 3, nb)            # [slot, channel, basis]
    n_q = nb - n_retain
    qc = np.zeros((n_q, 65536, 3), np.float16)
    qm = np.zeros((n_q, n_slots), np.uint16)
    for j in range(n_retain, nb):
        uniq, inv = np.unique(coeff[:, :, j], axis=0, return_inverse=True)
        assert len(uniq) <= 65536
        qc[j - n_retain, :len(uniq)] = uniq
        qm[j - n_retain] = inv.reshape(-1).astype(np.uint16)
    N = tree.child.shape[1]
    arrays = dict(data_dim=np.int64(dd), data_format=np.array(tree.data_format),
                  child=tree.child, invradius3=tree.invradius3, offset=tree.offset,
                  quant_colors=qc, quant_map=qm.reshape(n_q, cap, N, N, N),
                  sigma=data[:, -1].reshape(cap, N, N, N))
    if n_retain:
        ret = np.stack([coeff[:, :, j] for j in range(n_retain)])  # [n_ret, slot, 3]
        arrays["data_retained"] = ret.reshape(n_retain, cap, N, N, N, 3)
    (np.savez_compressed if compressed else np.savez)(path, **arrays)


def random_configuration(seed):
    """Seeded random (tree, transform, w, h, focal, ndc, option kwargs): formats, basis sizes,
    odd image sizes, cameras inside the volume, degenerate thresholds, bbox / basis range /
    view rotation / depth mode, NDC."""
    import numpy as np
    rng = np.random.default_rng(9000 + seed)
    fmt, bd = [("SH", 1), ("SH", 4), ("SH", 9), ("SH", 16), ("SH", 25), ("RGBA", 0), ("SG", 4),
               ("SG", 16), ("ASG", 9), ("SG", 7)][int(rng.integers(10))]
    tree = small_scene(depth=int(rng.integers(3, 7)), basis_dim=bd, fmt=fmt,
                       seed=int(rng.integers(1 << 30)))
    w, h = int(rng.integers(9, 70)), int(rng.integers(9, 70))
    tr = np.array(camera_for(pose_idx=int(rng.integers(8)), size=64)[0], dtype=np.float32)
    tr[9:12] *= np.float32(rng.choice([1.0, 0.6, 0.25, 0.05]))  # move towards / into the volume
    focal = float(rng.uniform(0.4, 2.5) * w)
    lo = rng.uniform(0.0, 0.4, 3)
    hi = rng.uniform(0.6, 1.0, 3)
    bmin = int(rng.integers(0, 3))
    kw = dict(step_size=float(10 ** rng.uniform(-5, -2)),
              sigma_thresh=float(rng.choice([0.0, 1e-2, 0.5, 20.0])),
              stop_thresh=float(rng.choice([0.0, 1e-3, 1e-2, 0.3])),
              background_brightness=float(rng.choice([0.0, 0.5, 1.0])),
              render_bbox=tuple(lo) + tuple(hi) if rng.random() < 0.5 else (0, 0, 0, 1, 1, 1),
              basis_minmax=(bmin, int(rng.integers(bmin, 25))) if rng.random() < 0.4 else (0, 24),
              rot_dirs=tuple(rng.normal(size=3) * 0.7) if rng.random() < 0.3 else (0, 0, 0),
              render_depth=int(rng.random() < 0.2))
    ndc = (float(w), float(h), float(focal)) if rng.random() < 0.25 else None
    return tree, tr, w, h, focal, ndc, kw, (fmt, bd)


def deep_chain_tree_n2(depth=28, basis_dim=4, fmt="SH", seed=0, target=(3.1e-4, 5.3e-4, 4.2e-4)):
    """An N = 2 tree that is a CHAIN towards `target`: at every level the child that contains the
    target is refined again (and one more child of the node into a node of leaves), `depth` levels
    deep -- a few dozen nodes with leaves of every depth 1..depth.  Deeper than 24 levels the
    integer lookup of the kernels (exact digits of a binary32 coordinate) does not apply and
    vr_tree_upload routes the tree to the literal float descent, which the reference runs for
    every tree (n3tree_query.hpp:22-47).  offset 0 / scale 1: tree coordinates = world
    coordinates, so that a camera placed AT the target (coordinates ~1e-4: binary32 resolves
    2^-36 there) starts every ray inside the deepest leaf.  Returns (tree, target as float32)."""
    from volrend_amd import synth
    rng = np.random.default_rng(seed)
    T = np.asarray(target, dtype=np.float32)
    data_dim = 4 if fmt == "RGBA" else 3 * basis_dim + 1
    child_rows, level_of = [np.zeros(8, np.int64)], [0]   # absolute child ids, 0 = leaf
    x = T.astype(np.float64).copy()
    node = 0
    for lvl in range(depth - 1):
        x *= 2.0
        k = np.floor(x).astype(np.int64)
        x -= k
        slot = int(k[0] * 4 + k[1] * 2 + k[2])            # x is the most significant digit
        nxt = len(child_rows)
        child_rows.append(np.zeros(8, np.int64))
        level_of.append(lvl + 1)
        child_rows[node][slot] = nxt
        other = int((slot + 1 + rng.integers(7)) % 8)     # one sibling becomes a node of leaves
        side = len(child_rows)
        child_rows.append(np.zeros(8, np.int64))
        level_of.append(lvl + 1)
        child_rows[node][other] = side
        node = nxt
    cap = len(child_rows)
    ids = np.stack(child_rows)
    child = np.where(ids != 0, ids - np.arange(cap)[:, None], 0).astype(np.int32)
    data = np.zeros((cap, 8, data_dim), dtype=np.float32)
    data[..., :-1] = rng.standard_normal((cap, 8, data_dim - 1)) * 0.6
    if fmt == "RGBA":
        data[..., :3] = rng.uniform(0.05, 0.95, size=(cap, 8, 3))
    lvl = np.asarray(level_of)[:, None]
    occ = (rng.random((cap, 8)) < 0.6) & (child == 0)
    # steps near the target are ~1e-8 long: deep leaves get large densities so that they still weigh in
    sig = np.where(lvl >= 14, np.exp(rng.uniform(np.log(2e3), np.log(6e4), size=(cap, 8))),
                   np.exp(rng.uniform(np.log(2.0), np.log(200.0), size=(cap, 8))))
    data[..., -1] = np.where(occ, sig, 0)
    data[child != 0] = 0
    name = "RGBA" if fmt == "RGBA" else f"{fmt}{basis_dim}"
    tree = synth.SynthTree(child.reshape(cap, 2, 2, 2), data.astype(np.float16).reshape(cap, 2, 2, 2, data_dim),
                           np.zeros(3, np.float32), np.ones(3, np.float32), name, None, depth)
    return tree, T


def camera_at(position, look_at=(0.5, 0.5, 0.5), size=40, focal=28.0):
    """12-float transform (columns right, up, back, centre) of a camera AT `position` (float32,
    kept bit for bit) looking at `look_at`."""
    c = np.asarray(position, dtype=np.float32)
    back = c.astype(np.float64) - np.asarray(look_at, np.float64)
    back /= np.linalg.norm(back)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    tr = np.concatenate([right, up, back]).astype(np.float32)
    return np.concatenate([tr, c]).astype(np.float32), size, size, focal


# Special values of the value-domain tests, as binary16 bit patterns.
#   sigma: -0, negative, smallest / largest subnormal, 65504, +-inf, NaN, and 0.5 (a sigma_thresh that
#   binary16 represents) with its neighbours one half-ulp below / above
EDGE_SIGMA = [0x8000, 0xB800, 0xC000, 0x0001, 0x03FF, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0x3800, 0x37FF, 0x3801]
#   SH / SG / ASG coefficients: NaN, +-inf, +-65504 (sums overflow, inf meets -inf, inf meets a basis
#   value of 0), and values that put the sigmoid argument -0.2821 * c of basis 0 into the subnormal
#   band of exp ([-104, -87]: c in [308, 369]), at +-88 / 89 (c = +-312, +-316) and beyond the clamp
EDGE_COEFF = [0x7E00, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF] + [
    int(np.float16(s * v).view(np.uint16)) for v in (308, 312, 316, 330, 350, 369, 390, 1000) for s in (1, -1)]
#   RGBA colours: negative, > 1, the largest finite, +-inf, NaN
EDGE_RGBA = [0xB800, 0xC200, 0x3E00, 0x4700, 0x7BFF, 0x7C00, 0xFC00, 0x7E00]


def apply_value_edges(tree, seed, frac=0.08, coeff=None, rgba_colours=None, sigmas=None):
    """Overwrites a seeded fraction ``frac`` of the leaf records of ``tree`` (occupied and empty
    alike) with special values: in each chosen record 1-3 colour entries from EDGE_COEFF / EDGE_RGBA
    (for SH / SG / ASG basis 0 of a channel half the time, whose basis value is the constant 0.2821)
    and, in half of them, sigma from EDGE_SIGMA.  SG / ASG lobes get special parameters too: lambda
    NaN, inf, 0 and 1e30 in lobes 0-3 and a mu of length 2 in lobe 4.  ``coeff``, ``rgba_colours`` and
    ``sigmas`` replace the three catalogues (binary16 bit patterns).  Returns a new tree."""
    import dataclasses
    rng = np.random.default_rng(seed)
    dd = tree.data_dim
    data = tree.data.reshape(-1, dd).view(np.uint16).copy()
    leaf = np.flatnonzero(tree.child.reshape(-1) == 0)
    pick = leaf[rng.random(leaf.size) < frac]
    rgba = tree.format_name == "RGBA"
    bd = max(tree.basis_dim, 1)
    coeff = EDGE_COEFF if coeff is None else coeff
    rgba_colours = EDGE_RGBA if rgba_colours is None else rgba_colours
    sigmas = EDGE_SIGMA if sigmas is None else sigmas
    cat = np.array(rgba_colours if rgba else coeff, np.uint16)
    for r in pick:
        for _ in range(int(rng.integers(1, 4))):
            ch = int(rng.integers(3))
            j = ch if rgba else ch * bd + (0 if rng.random() < 0.5 else int(rng.integers(bd)))
            data[r, j] = cat[rng.integers(cat.size)]
        if rng.random() < 0.5:
            data[r, dd - 1] = sigmas[int(rng.integers(len(sigmas)))]
    extra = tree.extra
    if extra is not None:
        extra = extra.copy()
        ex = extra.reshape(bd, -1)      # one row per lobe: SG [lambda, mu], ASG [lambda_x, lambda_y, axes]
        for lobe, lam in zip(range(4), (np.nan, np.inf, 0.0, 1e30)):
            if lobe < bd:
                ex[lobe, 0] = lam
        if bd > 4:
            ex[4, 1:4] *= 2.0
    return dataclasses.replace(tree, data=data.view(np.float16).reshape(tree.data.shape), extra=extra)


def value_edge_tree(fmt="SH", basis_dim=16, seed=0, depth=5, frac=0.08, **catalogues):
    """A seeded small_scene with special values in a fraction of its leaf records (apply_value_edges)."""
    return apply_value_edges(small_scene(depth=depth, basis_dim=basis_dim, fmt=fmt, seed=seed), seed + 1, frac,
                             **catalogues)


def axis_camera(size=63, focal=70.0, dist=4.0):
    """A camera on the +z axis looking down -z with an identity rotation: for an odd ``size`` the
    centre row and column of rays have direction components that are exactly 0 (SH basis values
    such as y, x*y are exactly 0 there)."""
    tr = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, dist], dtype=np.float32)
    return tr, size, size, focal


def fog_tree(fmt="SH", basis_dim=16, seed=0, depth=5, sigma=(0.05, 0.4)):
    """A full tree (every node refined down to ``depth`` levels, all 8^depth leaves occupied) of
    low density: rays cross the whole volume and every sample is a hit, so the deferred shading
    (colour queues, the wave ring and its flushes) runs under full pressure.  Colours as
    small_scene; sigma uniform in ``sigma``."""
    rng = np.random.default_rng(seed)
    data_dim = 4 if fmt == "RGBA" else 3 * basis_dim + 1
    n_inner = sum(8 ** d for d in range(depth - 1))       # nodes whose 8 slots are nodes
    cap = n_inner + 8 ** (depth - 1)
    child = np.zeros((cap, 8), np.int32)
    node = np.arange(n_inner)
    child[:n_inner] = (8 * node[:, None] + 1 + np.arange(8)[None, :]) - node[:, None]   # breadth-first
    data = np.zeros((cap, 8, data_dim), np.float32)
    data[..., :-1] = rng.standard_normal((cap, 8, data_dim - 1)) * 0.6
    if fmt == "RGBA":
        data[..., :3] = rng.uniform(0.05, 0.95, size=(cap, 8, 3))
    data[..., -1] = rng.uniform(*sigma, size=(cap, 8))
    data[child != 0] = 0
    base = small_scene(depth=2, basis_dim=basis_dim, fmt=fmt, seed=seed)   # offset, scale, SG / ASG lobes
    name = "RGBA" if fmt == "RGBA" else f"{fmt}{basis_dim}"
    return synth.SynthTree(child.reshape(cap, 2, 2, 2), data.astype(np.float16).reshape(cap, 2, 2, 2, data_dim),
                           base.offset, base.invradius3, name, base.extra, depth)


def assert_same_values(rgba_g, acc_g, rgba_o, acc_o, what=""):
    """NaN-aware equality for the value-domain tests: RGBA8 bytes equal; fp32 words bit-equal or
    both NaN, with the NaNs in exactly the same places (only the sign and payload of a NaN may
    differ: x86 makes 0xFFC00000 where gfx950 makes 0x7FC00000)."""
    bad_px = int((rgba_g != rgba_o).any(-1).sum())
    assert bad_px == 0, f"{what}: {bad_px} RGBA8 pixels differ"
    if acc_o is None:
        return
    ng, no = np.isnan(acc_g), np.isnan(acc_o)
    assert np.array_equal(ng, no), f"{what}: NaN in {int((ng & ~no).sum())} kernel / {int((no & ~ng).sum())} " \
                                   f"oracle accumulator words only"
    diff = (acc_g.view(np.uint32) != acc_o.view(np.uint32)) & ~no
    assert not diff.any(), f"{what}: {int(diff.sum())} accumulator words differ"


# The value-domain cases (tests/test_oracle_vs_ref.py, tests/test_gpu_value_domain.py):
#   name -> (fmt, basis_dim, camera: "orbit" | "axis", render options)
VALUE_CASES = {
    "SH1": ("SH", 1, "orbit", {}),
    "SH4": ("SH", 4, "orbit", {}),
    "SH9": ("SH", 9, "orbit", {}),
    "SH16": ("SH", 16, "orbit", {}),
    "SH25": ("SH", 25, "orbit", {}),
    "RGBA": ("RGBA", 0, "orbit", {}),
    "SG7": ("SG", 7, "orbit", dict(basis_minmax=(1, 6))),        # lobe 0 (lambda NaN) left out
    "SG9_nan_lobe": ("SG", 9, "orbit", {}),                       # ... and taken: every colour NaN
    "ASG4": ("ASG", 4, "orbit", dict(basis_minmax=(1, 3))),
    "SH16_axis": ("SH", 16, "axis", {}),                          # inf coefficient x basis value 0
    "SH9_basis_range": ("SH", 9, "axis", dict(basis_minmax=(1, 5))),
    "SH9_thresh_edge": ("SH", 9, "orbit", dict(sigma_thresh=0.5)),
    "SH4_negative_thresh": ("SH", 4, "orbit", dict(sigma_thresh=-1.0)),   # every sample a hit
    "SH16_stop_ge_1": ("SH", 16, "orbit", dict(stop_thresh=1.5, background_brightness=-0.75)),
    "RGBA_never_stop": ("RGBA", 0, "orbit", dict(stop_thresh=-0.5, background_brightness=3e7)),
    "RGBA_stop_ge_1": ("RGBA", 0, "axis", dict(stop_thresh=1.0, background_brightness=1.5)),
    "SH16_depth": ("SH", 16, "orbit", dict(render_depth=1)),
}


def value_case(name, size=56):
    """-> (tree, transform, w, h, focal, option kwargs) of VALUE_CASES[name]."""
    fmt, bd, cam, kw = VALUE_CASES[name]
    seed = 7000 + sum(map(ord, name))
    tree = value_edge_tree(fmt, bd, seed=seed)
    tr, w, h, f = axis_camera(size | 1) if cam == "axis" else camera_for(pose_idx=seed % 8, size=size)
    return tree, tr, w, h, f, dict(kw)


# fog scenes: name -> (fmt, basis_dim, render options)
FOG_CASES = {
    "SH16": ("SH", 16, {}),
    "SH25": ("SH", 25, {}),
    "SG7": ("SG", 7, {}),
    "RGBA": ("RGBA", 0, {}),
    "SH16_negative_thresh": ("SH", 16, dict(sigma_thresh=-0.5)),  # zero-density samples queue items too
}


def fog_case(name, size=48):
    """-> (tree, transform, w, h, focal, option kwargs) of FOG_CASES[name]: a depth-6 fog tree
    (every sample a hit, ~90 hits per ray, no early stop).  The negative-threshold variant zeroes a
    third of the leaves' densities."""
    fmt, bd, kw = FOG_CASES[name]
    seed = 8000 + sum(map(ord, name))
    tree = fog_tree(fmt, bd, seed=seed, depth=6)
    if kw.get("sigma_thresh", 0.0) < 0:
        rng = np.random.default_rng(seed)
        d = tree.data.reshape(-1, tree.data_dim)
        d[rng.random(d.shape[0]) < 1 / 3, -1] = 0
    tr, w, h, f = camera_for(pose_idx=seed % 8, size=size)
    return tree, tr, w, h, f, dict(kw)


def edge_probe_point(tree, seed=0):
    """A world point whose leaf holds a non-finite colour coefficient (vr_probe_coeffs / the
    probe overlay then see it)."""
    import ctypes as C
    th = ob.TreeHandle(tree)
    rng = np.random.default_rng(seed)
    out = np.zeros(tree.data_dim - 1, np.float32)
    for _ in range(20000):
        p = tuple(float(v) for v in rng.uniform(-1.4, 1.4, 3))
        ob.lib().or_probe_coeffs(C.byref(th.struct), C.byref(ob.default_options(enable_probe=1, probe=p)),
                                 out.ctypes.data)
        if not np.isfinite(out[:3 * max(tree.basis_dim, 1)]).all():
            return p
    raise AssertionError("no leaf with a non-finite coefficient found")


# ---- asymmetric geometry: no two of scale[3], offset[3], (fx, fy), (ndc width, height, focal) equal ----
ASYM_FACTORS = (0.7, 1.3, 0.45)
ASYM_OFFSET = (0.42, 0.55, 0.61)
ASYM_FORMATS = [("SH", 1), ("SH", 9), ("SH", 16), ("SH", 25), ("RGBA", 0), ("SG", 4), ("ASG", 4)]
ASYM_OPTIONS = {
    "plain": {},
    "rot_dirs": dict(rot_dirs=(0.3, -0.2, 0.9)),
    "depth": dict(render_depth=1),
    "bbox": dict(render_bbox=(0.1, 0.2, 0.0, 0.8, 0.9, 0.7)),
}
ASYM_PROBE = (0.1, -0.15, 0.2)


def asymmetric(tree, factors=ASYM_FACTORS, offset=ASYM_OFFSET):
    """``tree`` with a scale and an offset that differ on every axis: invradius3 * factors (float32, one
    rounding) and the given offset.  Nodes and records are shared with ``tree``."""
    scale = np.asarray(tree.invradius3, np.float32) * np.asarray(factors, np.float32)
    return dataclasses.replace(tree, invradius3=scale.astype(np.float32), offset=np.asarray(offset, np.float32))


def asymmetric_camera():
    """-> (transform, w, h, fx, fy): pose 2 of the orbit on a 64 x 48 frame with fx = 1.2 f, fy = 0.7 f."""
    tr, _, _, f = camera_for(pose_idx=2, size=64)
    return tr, 64, 48, 1.2 * f, 0.7 * f


def asymmetric_scene(fmt="SH", basis_dim=9, depth=5):
    """The asymmetric tree of a format (a seeded small_scene) -- one per format for every test that names it."""
    return asymmetric(small_scene(depth=depth, basis_dim=basis_dim, fmt=fmt, seed=300 + basis_dim))


def asymmetric_ndc_case(basis_dim=4):
    """-> (tree, transform, w, h, fx, fy, ndc): an NDC tree whose scale, offset, camera and NDC numbers all
    differ from each other (ndc = width, height, focal; none is the camera's own)."""
    from tests import aov_util
    tree = dataclasses.replace(small_scene(depth=5, basis_dim=basis_dim, seed=351),
                               invradius3=np.array([0.4, 0.55, 0.3], np.float32),
                               offset=np.array([0.45, 0.52, 0.58], np.float32))
    return tree, aov_util.NDC_TRANSFORM.copy(), 96, 72, 80.0, 65.0, (120.0, 60.0, 95.0)


def non_orthonormal(transform):
    """The pose mirrored (``right`` negated: a left-handed frame, as other pose conventions produce) and
    sheared in length (``up`` x 1.7).  The reference normalises the direction after the matrix product."""
    tr = np.array(transform, np.float32).copy()
    tr[0:3] = -tr[0:3]
    tr[3:6] = tr[3:6] * np.float32(1.7)
    return tr


def mesh_underlay(w, h, seed=5):
    """-> (rgba uint8 [h, w, 4], depth float32 [h, w]): a frame to composite over and a mesh depth plane that
    ends part of the rays inside the volume."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8),
            rng.uniform(2.0, 6.0, size=(h, w)).astype(np.float32))


# ---- stand-ins for the Python API's argument checks (no GPU, no library) -------------------------
class FakeTree:
    """A duck-typed tree whose handle is never followed.  ``attrs``: the attributes it has (the defaults are
    those of a 10-node N = 2 SH16 tree); ``info``: "raises" (the tree must not be asked anything), or the device
    index ``info()`` answers.  ``info_calls`` counts either way."""
    HANDLE = 0x1000

    def __init__(self, info="raises", **attrs):
        self._info, self.info_calls = info, 0
        for k, v in dict(dict(handle=self.HANDLE, capacity=10, N=2, data_dim=49, data_format=("SH", 16)), **attrs).items():
            if v is not None:   # (None: the fake does not have that attribute)
                setattr(self, k, v)

    def info(self):
        self.info_calls += 1
        if self._info == "raises":
            raise AssertionError("the tree must not be asked anything")
        return {"device": self._info}


class FakeCudaTensor:
    """What the argument checks read of a torch CUDA tensor, with no GPU behind it: the address is never followed."""

    class _Dtype(str):
        __repr__ = __str__ = lambda self: "torch." + str.__str__(self)

    class _Device:
        def __init__(self, kind, index):
            self.type, self.index = kind, index

        def __str__(self):
            return self.type if self.index is None else f"{self.type}:{self.index}"

    def __init__(self, shape, dtype="float32", ptr=0x7000, contiguous=True, is_cuda=True, index=0):
        self.shape, self.dtype, self._ptr, self._contiguous = tuple(shape), self._Dtype(dtype), ptr, contiguous
        self.is_cuda, self.device = is_cuda, self._Device("cuda" if is_cuda else "cpu", index if is_cuda else None)

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def dim(self):
        return len(self.shape)


# ---- child arrays for the host walks (tests/test_tree_walk.py, tests/test_weights_file_order.py) ------------------
def rows_of(tree):
    return tree.child.reshape(tree.capacity, -1).astype(np.int64)


def scrambled(child, seed=7, new_of=None):
    """The construction of tests/test_gpu_chain.py::test_tree_with_backward_links on the child array:
    the nodes in a random order, root first (or in the order ``new_of``, a permutation that keeps node 0).
    -> (new child array, new index of every old node)."""
    cap = child.shape[0]
    if new_of is None:
        new_of = np.concatenate([[0], 1 + np.random.default_rng(seed).permutation(cap - 1)])
    new_of = np.asarray(new_of, np.int64)
    assert new_of[0] == 0 and np.array_equal(np.sort(new_of), np.arange(cap))
    tgt = np.where(child != 0, np.arange(cap)[:, None] + child, -1)
    out = np.zeros_like(child)
    out[new_of] = np.where(tgt >= 0, new_of[np.maximum(tgt, 0)] - new_of[:, None], 0)
    return out, new_of


def with_unreachable(child):
    """Five nodes behind the tree that nothing links to: one links on to the next, one back into the tree."""
    extra = np.zeros((5, child.shape[1]), np.int64)
    extra[1, 2] = 1
    extra[3, 0] = -(child.shape[0] + 2)       # -> node 1 of the tree
    return np.concatenate([child, extra])


def node_levels(child):
    """int [capacity]: the number of links from node 0 to each node of a child array [capacity, N^3]; -1 for a node
    the root does not reach.  A link outside [1, capacity) is not followed."""
    child = np.asarray(child).astype(np.int64)
    cap = child.shape[0]
    level = np.full(cap, -1, np.int64)
    level[0] = 0
    front, d = np.array([0]), 0
    while front.size:
        tgt = (front[:, None] + child[front])[child[front] != 0]
        front = tgt[(tgt >= 1) & (tgt < cap)]
        d += 1
        assert (level[front] < 0).all(), "not a tree"
        level[front] = d
    return level


def subtree_sizes(child):
    """int [capacity]: nodes in the subtree of every node the root reaches (itself included); 0 for the others."""
    child = np.asarray(child).astype(np.int64)
    level = node_levels(child)
    size = (level >= 0).astype(np.int64)
    for d in range(int(level.max()), 0, -1):
        n, j = np.nonzero((child != 0) & (level == d - 1)[:, None])
        np.add.at(size, n, size[n + child[n, j]])
    return size


# The kinds of renumbered(), in the order in which they are applied.
#   pruned        one internal slot of depth `prune_depth` loses its link: a leaf with the record it holds; its
#                 subtree (>= 8 nodes) stays in the array with its values, linked among itself, out of the root's reach
#                 -- a caller who prunes without compacting
#   random        scrambled()'s order, root first: links forward and backward
#   reversed      node i >= 1 at capacity - i: every link backward, the general walk's worst order
#   slack_zero    7 all-zero nodes behind the tree: a file saved with more capacity than it uses
#   slack_linked  with_unreachable()'s five nodes (one links to the next, one into the tree: node 1 is linked from two
#                 slots), one of them with a further link outside [1, capacity); all five hold dense, bright records
#                 (every coefficient 3.0, sigma 200): whatever reaches them changes a pixel, a weight or a gradient
RENUMBER_KINDS = ("pruned", "random", "reversed", "slack_zero", "slack_linked")
SLACK_ZERO_NODES = 7
BRIGHT_COEFF, BRIGHT_SIGMA = 3.0, 200.0


def renumbered(tree, kinds, seed=7, prune_depth=2):
    """``tree`` (a SynthTree) restated as the same scene under another numbering and with nodes the root does not
    reach: the ``kinds`` of RENUMBER_KINDS, applied in that order whatever order they are given in.  Records move
    with their nodes; ``extra``, offset and scale are carried along.  -> (tree2, new_of): ``new_of[old node]`` is
    the node's index in ``tree2`` (the nodes a slack kind appends have no old index)."""
    kinds = tuple(kinds)
    assert kinds and all(k in RENUMBER_KINDS for k in kinds) and len(set(kinds)) == len(kinds), kinds
    cap, N = tree.capacity, tree.N
    N3, dd = N ** 3, tree.data_dim
    child = rows_of(tree).copy()
    data = np.array(tree.data, np.float16).reshape(cap, N3, dd)
    new_of = np.arange(cap)
    if "pruned" in kinds:
        size = subtree_sizes(child)
        n, j = np.nonzero((child != 0) & (node_levels(child) == prune_depth - 1)[:, None])
        big = size[n + child[n, j]] >= 8
        assert big.any(), f"no internal slot of depth {prune_depth} has a subtree of 8 nodes"
        child[n[big][0], j[big][0]] = 0
    for kind in ("random", "reversed"):
        if kind in kinds:
            order = None if kind == "random" else np.concatenate([[0], cap - np.arange(1, cap)])
            child, p = scrambled(child, seed, order)
            moved = np.empty_like(data)
            moved[p] = data
            data, new_of = moved, p[new_of]
    if "slack_zero" in kinds:
        child = np.concatenate([child, np.zeros((SLACK_ZERO_NODES, N3), np.int64)])
        data = np.concatenate([data, np.zeros((SLACK_ZERO_NODES, N3, dd), np.float16)])
    if "slack_linked" in kinds:
        child = with_unreachable(child)
        child[-1, N3 - 1] = 9                 # -> capacity + 8: outside the array, never followed
        bright = np.full((5, N3, dd), BRIGHT_COEFF, np.float16)
        bright[..., -1] = BRIGHT_SIGMA
        data = np.concatenate([data, bright])
    cap2 = child.shape[0]
    tree2 = dataclasses.replace(tree, child=child.astype(np.int32).reshape(cap2, N, N, N),
                                data=np.ascontiguousarray(data).reshape(cap2, N, N, N, dd))
    return tree2, new_of


def orphan_nodes(tree):
    """bool [capacity]: the nodes of a tree that the root does not reach."""
    return node_levels(rows_of(tree)) < 0


# ---- one frame on the GPU against the oracle (torch is handed in) --------------------------------------------------
def gpu_frame(torch, tree, transform, w, h, focal, fp_mode=0, ndc=None, offscreen=True,
              rgba_init=None, depth_init=None, shard=None, fy=None, **opt_kw):
    from volrend_amd import api
    t = api.N3Tree.from_synth(tree, ndc=ndc)
    cam = api.Camera(w, h, focal, focal if fy is None else fy)
    cam.transform = np.asarray(transform, dtype=np.float32)
    opts = api.RenderOptions(**opt_kw)
    if rgba_init is not None:
        img = torch.from_numpy(rgba_init.copy()).cuda()
    else:
        img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    dep = torch.from_numpy(depth_init).cuda() if depth_init is not None else None
    api.launch_renderer(t, cam, opts, img, dep, torch.cuda.current_stream(), offscreen,
                        accum=acc, shard=shard, fp_mode=fp_mode)
    torch.cuda.synchronize()
    out = img.cpu().numpy(), acc.cpu().numpy()
    t.free_device()
    return out


def assert_parity(rgba_g, acc_g, rgba_o, acc_o):
    ulp = ulp_diff(acc_g, acc_o)
    bad_px = int((rgba_g != rgba_o).any(-1).sum())
    assert ulp.max() <= 1, f"accumulators differ by up to {ulp.max()} ulp"
    assert bad_px == 0, f"{bad_px} RGBA8 pixels differ"
    assert np.array_equal(acc_g.view(np.uint32), acc_o.view(np.uint32)), "accumulators not bit-equal"
