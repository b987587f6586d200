"""The oracle's pin: the C restatement (oracle/vr_oracle.c, strict mode) against the
reference's OWN device code compiled for the host (oracle/_ref/libvolrend_ref.so, built
by oracle/ref_build/Makefile from /root/reference/src/cuda/volrend.cu and the headers it
includes).  Bit equality of the fp32 accumulators and of RGBA8 is required.

The _ref library is built by __graft_entry__.build() where the reference is mounted.  Its outputs
for these cases are stored as SHA-256 digests in tests/golden/ref_pins_v1.json (tests/common.py
assert_ref_equal), so the pins hold everywhere; where the library is built, every output is
recomputed and compared directly as well."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests.common import assert_ref_equal, ob, ref_array


def both(key, tree, tr, w, h, f, ndc=None, msg="", fy=None, **opt_kw):
    th = ob.TreeHandle(tree, ndc=ndc)
    cam = ob.make_camera(tr, w, h, f, fy)
    opt = ob.default_options(**opt_kw)
    rgba_o, acc_o, _ = ob.render(th, cam, opt, ob.FP_STRICT)
    assert_ref_equal(key + "/rgba", rgba_o, lambda: ob.ref_render(th, cam, opt), msg=msg)
    return rgba_o, acc_o, (th, cam, opt)


def assert_accum_equal(key, acc_o, th, cam, opt, msg=""):
    """The oracle's accumulators == the reference's trace_ray, as uint32 bit patterns."""
    assert_ref_equal(key + "/accum", acc_o.view(np.uint32), lambda: ob.ref_trace(th, cam, opt).view(np.uint32),
                     msg=msg)


@pytest.mark.parametrize("fmt,basis_dim", [("SH", 1), ("SH", 4), ("SH", 9), ("SH", 16), ("SH", 25),
                                            ("RGBA", 0), ("SG", 9), ("SG", 25), ("ASG", 4)])
def test_formats_bit_exact(request, fmt, basis_dim):
    key = request.node.name
    tree = common.small_scene(depth=5, basis_dim=basis_dim, fmt=fmt, seed=100 + basis_dim)
    tr, w, h, f = common.camera_for(pose_idx=2, size=64)
    rgba_o, acc_o, (th, cam, opt) = both(key, tree, tr, w, h, f)
    assert_accum_equal(key, acc_o, th, cam, opt)
    assert (rgba_o[..., :3] != 255).any(), "scene must not be empty"


@pytest.mark.parametrize("kw", [
    dict(step_size=1e-3, sigma_thresh=0.5, stop_thresh=0.1, background_brightness=0.25),
    dict(render_bbox=(0.1, 0.2, 0.0, 0.8, 0.9, 0.7)),
    dict(basis_minmax=(1, 5)),
    dict(rot_dirs=(0.3, -0.2, 0.9)),
    dict(render_depth=1),
    dict(step_size=1e-5, stop_thresh=1e-4),
    dict(background_brightness=0.0, sigma_thresh=5.0),
])
def test_options_bit_exact(request, kw):
    key = request.node.name
    tree = common.small_scene(depth=6, basis_dim=9, seed=141)
    tr, w, h, f = common.camera_for(pose_idx=3, size=56)
    rgba_o, acc_o, (th, cam, opt) = both(key, tree, tr, w, h, f, **kw)
    if not kw.get("rot_dirs"):  # ref_trace takes the un-rotated prologue of render_kernel too
        pass
    assert_accum_equal(key, acc_o, th, cam, opt)


def test_ndc_bit_exact(request):
    key = request.node.name
    tree = common.small_scene(depth=5, basis_dim=4, seed=151)
    tr = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.05, -0.02, 0.3], dtype=np.float32)
    rgba_o, acc_o, (th, cam, opt) = both(key, tree, tr, 96, 72, 80.0, ndc=(96.0, 72.0, 80.0))
    assert_accum_equal(key, acc_o, th, cam, opt)


def test_compositing_over_existing_frame(request):
    tree = common.small_scene(depth=5, basis_dim=9, seed=171)
    tr, w, h, f = common.camera_for(pose_idx=4, size=48)
    rng = np.random.default_rng(5)
    init = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    depth = rng.uniform(2.0, 6.0, size=(h, w)).astype(np.float32)
    th = ob.TreeHandle(tree)
    cam = ob.make_camera(tr, w, h, f)
    opt = ob.default_options()
    rgba_o, _, _ = ob.render(th, cam, opt, offscreen=False, rgba_init=init, depth_init=depth)
    assert_ref_equal(request.node.name + "/rgba", rgba_o,
                     lambda: ob.ref_render(th, cam, opt, offscreen=False, rgba_init=init, depth_init=depth))


@pytest.mark.parametrize("fmt,bd,minmax,offscreen", [
    ("SH", 4, (0, 3), True), ("SH", 16, (2, 11), True), ("SH", 25, (0, 24), True),
    ("SG", 9, (0, 8), True), ("ASG", 4, (0, 3), False), ("RGBA", 0, (0, 24), True)])
def test_probe_overlay(request, fmt, bd, minmax, offscreen):
    tree = common.small_scene(depth=5, basis_dim=bd, fmt=fmt, seed=181)
    tr, w, h, f = common.camera_for(pose_idx=5, size=72)
    th = ob.TreeHandle(tree)
    cam = ob.make_camera(tr, w, h, f)
    # basis_minmax narrowed to the coefficients that exist (what VolumeRenderer::set does,
    # src/cuda_renderer.cpp:176-177); upstream reads out of bounds otherwise
    opt = ob.default_options(enable_probe=1, probe=(0.1, 0.0, 0.2), probe_disp_size=30,
                             basis_minmax=minmax)
    kw = {}
    if not offscreen:
        rng = np.random.default_rng(8)
        kw = dict(offscreen=False, rgba_init=rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8),
                  depth_init=rng.uniform(2.0, 6.0, size=(h, w)).astype(np.float32))
    rgba_o, _, _ = ob.render(th, cam, opt, **kw)
    assert_ref_equal(request.node.name + "/rgba", rgba_o, lambda: ob.ref_render(th, cam, opt, **kw))
    # probe coefficients: retrieve_cursor_lumisphere_kernel (volrend.cu:175-191)
    n = tree.data_dim - 1
    a = np.zeros(n, np.float32)
    ob.lib().or_probe_coeffs(C.byref(th.struct), C.byref(opt), a.ctypes.data)

    def ref_coeffs():
        b = np.zeros(n, np.float32)
        ob.ref_lib().ref_probe_coeffs(C.byref(th.struct), C.byref(opt), b.ctypes.data)
        return b.view(np.uint32)
    assert_ref_equal(request.node.name + "/probe_coeffs", a.view(np.uint32), ref_coeffs)


def test_point_query_and_basis(request):
    tree = common.small_scene(depth=6, basis_dim=25, seed=191)
    th = ob.TreeHandle(tree)
    rng = np.random.default_rng(3)
    pts, dirs = [], []
    for _ in range(500):
        pts.append(rng.uniform(-0.1, 1.1, size=3).astype(np.float32))
        d = rng.standard_normal(3).astype(np.float32)
        d /= np.linalg.norm(d)
        dirs.append(d)

    def run(query, basis):
        """-> per point: [leaf index, cube size, the point after the query (3), basis (25)] as uint32 bits"""
        rows = []
        for p, d in zip(pts, dirs):
            q, c = (C.c_float * 3)(*p), C.c_float()
            leaf = query(q, c)
            dv, out = (C.c_float * 3)(*d), (C.c_float * 25)()
            basis(dv, out)
            rows.append(np.concatenate([np.array([leaf], np.int64).astype(np.uint32),
                                        np.array([c.value, *q, *out], np.float32).view(np.uint32)]))
        return np.stack(rows)
    L = ob.lib()
    depth = C.c_int()
    got = run(lambda q, c: L.or_query(C.byref(th.struct), C.byref(q), C.byref(c), C.byref(depth)),
              lambda dv, out: L.or_basis(C.byref(th.struct), C.byref(dv), ob.FP_STRICT, C.byref(out)))

    def ref():
        R = ob.ref_lib()
        return run(lambda q, c: R.ref_query(C.byref(th.struct), C.byref(q), C.byref(c)),
                   lambda dv, out: R.ref_basis(C.byref(th.struct), C.byref(dv), C.byref(out)))
    assert_ref_equal(request.node.name + "/query_basis", got, ref)


def test_libm_expf_build_is_close(request):
    """With glibc's expf instead of the deterministic one the reference build differs by
    rounding noise only: bounds the cost of fixing the exp implementation."""
    tree = common.small_scene(depth=6, basis_dim=16, seed=201)
    tr, w, h, f = common.camera_for(pose_idx=1, size=96)
    th = ob.TreeHandle(tree)
    cam = ob.make_camera(tr, w, h, f)
    opt = ob.default_options()
    a, _, _ = ob.render(th, cam, opt, ob.FP_STRICT, want_accum=False)
    assert_ref_equal(request.node.name + "/rgba", a, lambda: ob.ref_render(th, cam, opt))
    b = ref_array(request.node.name + "/rgba_libm", lambda: ob.ref_render(th, cam, opt, libm_expf=True))
    a, b = a.astype(np.int32), b.astype(np.int32)
    diff = np.abs(a - b)
    assert diff.max() <= 1
    assert (diff > 0).any(-1).mean() < 0.02


def test_fma_model_noise_floor():
    """strict vs nvcc-like FMA contraction: the parity noise floor reported in DESIGN.md."""
    tree = common.small_scene(depth=6, basis_dim=16, seed=211)
    tr, w, h, f = common.camera_for(pose_idx=6, size=96)
    a, acc_a, _ = common.oracle_frame(tree, tr, w, h, f, ob.FP_STRICT)
    b, acc_b, _ = common.oracle_frame(tree, tr, w, h, f, ob.FP_FMA)
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    assert d.max() <= 1
    mse = float((d.astype(np.float64) ** 2).mean())
    psnr = 10 * np.log10(255.0 ** 2 / mse) if mse > 0 else np.inf
    assert psnr > 60.0


@pytest.mark.parametrize("N,depth,fmt,basis_dim", [(4, 3, "SH", 4), (3, 3, "RGBA", 0), (8, 2, "SH", 9)])
def test_general_branching_factor_bit_exact(request, N, depth, fmt, basis_dim):
    """N != 2: the float recurrence of query_single_from_root is no longer exact for every N
    (N = 3), so this pins the literal restatement, rounding included."""
    tree = common.random_tree_general_n(N, depth, basis_dim, fmt, seed=500 + N)
    tr, w, h, f = common.camera_for(pose_idx=3, size=48)
    rgba_o, acc_o, (th, cam, opt) = both(request.node.name, tree, tr, w, h, f)
    assert_accum_equal(request.node.name, acc_o, th, cam, opt)
    assert (rgba_o[..., :3] != 255).any()


@pytest.mark.parametrize("seed", range(24))
def test_random_configurations_bit_exact(request, seed):
    """Seeded sweep of the pin: random format / basis size / tree / camera / options (including
    odd image sizes, cameras inside the volume, degenerate thresholds and NDC) -- RGBA8 and fp32
    accumulators of the oracle equal the reference host build's bit for bit."""
    tree, tr, w, h, focal, ndc, kw, (fmt, bd) = common.random_configuration(seed)
    rgba_o, acc_o, (th, cam, opt) = both(request.node.name, tree, tr, w, h, focal, ndc=ndc, msg=str((fmt, bd, kw)), **kw)
    assert_accum_equal(request.node.name, acc_o, th, cam, opt, msg=str((fmt, bd, kw)))


@pytest.mark.parametrize("depth,step", [(26, 1e-8), (28, 1e-4), (30, 1e-8)])
def test_deep_n2_chain_tree(request, depth, step):
    """Trees deeper than 24 levels (the kernels' float-descent fallback for N = 2,
    tests/test_gpu_parity.py): the oracle's root descent equals the reference's
    query_single_from_root (n3tree_query.hpp:22-47) at every depth the format allows -- the camera
    sits inside the deepest leaf of a 26-30 level chain and every ray samples every level."""
    tree, T = common.deep_chain_tree_n2(depth=depth, basis_dim=4, seed=depth)
    tr, w, h, f = common.camera_at(T)
    th = ob.TreeHandle(tree)
    cam = ob.make_camera(tr, w, h, f)
    opt = ob.default_options(step_size=step)
    rgba_o, acc_o, cnt = ob.render(th, cam, opt, ob.FP_STRICT)
    assert cnt["hit_samples"] > 5000 and cnt["child_reads"] > 8 * cnt["samples"]
    assert_ref_equal(request.node.name + "/rgba", rgba_o, lambda: ob.ref_render(th, cam, opt))
    assert_accum_equal(request.node.name, acc_o, th, cam, opt)


@pytest.mark.parametrize("case", list(common.VALUE_CASES))
def test_special_values_bit_exact(request, case):
    """Leaf records with special values (tests/common.py apply_value_edges: sigma -0 / negative /
    subnormal / 65504 / +-inf / NaN / at a threshold; colour coefficients NaN / +-inf / +-65504 /
    sigmoid arguments in exp's subnormal band, at its overflow edge and beyond its clamp; RGBA
    colours outside [0, 1]; SG / ASG lobes with lambda NaN / inf / 0 / 1e30) and the options at the
    edges of their domains: the oracle's RGBA8 and fp32 accumulators equal the reference build's bit
    for bit, NaNs included."""
    tree, tr, w, h, f, kw = common.value_case(case)
    rgba_o, acc_o, (th, cam, opt) = both(request.node.name, tree, tr, w, h, f, msg=str(kw), **kw)
    assert_accum_equal(request.node.name, acc_o, th, cam, opt, msg=str(kw))
    assert np.isfinite(acc_o).any() and (np.isnan(acc_o).any() or kw.get("render_depth"))


@pytest.mark.parametrize("kind", ["N3", "chain26"])
def test_special_values_generic_trees(request, kind):
    """The same special values in an N = 3 tree and in a 26-level N = 2 chain around the camera
    (both take the float descent)."""
    if kind == "N3":
        tree = common.apply_value_edges(common.random_tree_general_n(3, 3, 4, "SH", seed=703), 704, frac=0.15)
        tr, w, h, f = common.camera_for(pose_idx=3, size=48)
        kw = {}
    else:
        tree, T = common.deep_chain_tree_n2(depth=26, basis_dim=4, seed=705)
        tree = common.apply_value_edges(tree, 706, frac=0.3)
        tr, w, h, f = common.camera_at(T)
        kw = dict(step_size=1e-8)
    rgba_o, acc_o, (th, cam, opt) = both(request.node.name, tree, tr, w, h, f, **kw)
    assert_accum_equal(request.node.name, acc_o, th, cam, opt)
    assert np.isnan(acc_o).any() and np.isfinite(acc_o).any()


@pytest.mark.parametrize("fmt,bd", [("SH", 9), ("SG", 4)])
def test_special_values_probe(request, fmt, bd):
    """Probe overlay and probe coefficients at a leaf that holds a non-finite coefficient."""
    tree = common.value_edge_tree(fmt, bd, seed=710 + bd)
    p = common.edge_probe_point(tree, seed=bd)
    tr, w, h, f = common.camera_for(pose_idx=5, size=48)
    th = ob.TreeHandle(tree)
    cam = ob.make_camera(tr, w, h, f)
    opt = ob.default_options(enable_probe=1, probe=p, probe_disp_size=30, basis_minmax=(0, bd - 1))
    rgba_o, _, _ = ob.render(th, cam, opt)
    assert_ref_equal(request.node.name + "/rgba", rgba_o, lambda: ob.ref_render(th, cam, opt))
    n = tree.data_dim - 1
    a = np.zeros(n, np.float32)
    ob.lib().or_probe_coeffs(C.byref(th.struct), C.byref(opt), a.ctypes.data)
    assert not np.isfinite(a).all()

    def ref_coeffs():
        b = np.zeros(n, np.float32)
        ob.ref_lib().ref_probe_coeffs(C.byref(th.struct), C.byref(opt), b.ctypes.data)
        return b.view(np.uint32)
    assert_ref_equal(request.node.name + "/probe_coeffs", a.view(np.uint32), ref_coeffs)


@pytest.mark.parametrize("case", list(common.FOG_CASES))
def test_fog_bit_exact(request, case):
    """Fog (every sample of ~90 per ray a hit, tests/common.py fog_tree) against the reference build."""
    tree, tr, w, h, f, kw = common.fog_case(case)
    rgba_o, acc_o, (th, cam, opt) = both(request.node.name, tree, tr, w, h, f, **kw)
    assert_accum_equal(request.node.name, acc_o, th, cam, opt)


# ---- asymmetric geometry (tests/common.py): scale, offset, fx / fy and the NDC numbers all differ per axis ----
ASYM_CASES = [f"{fmt}{bd}-{o}" for fmt, bd in common.ASYM_FORMATS for o in common.ASYM_OPTIONS] + \
    ["ndc", "non_orthonormal", "compositing", "probe"]


@pytest.mark.parametrize("case", ASYM_CASES)
def test_asymmetric_geometry_bit_exact(request, case):
    """A tree whose scale and offset differ on every axis under a camera with fx != fy (and, for the NDC
    tree, ndc width / height / focal that are neither each other's nor the camera's): an index mix-up in
    the ray set-up, or a per-ray delta_scale taken for a constant, shows here and nowhere else."""
    key = request.node.name
    tr, w, h, fx, fy = common.asymmetric_camera()
    if case == "ndc":
        tree, tr, w, h, fx, fy, ndc = common.asymmetric_ndc_case()
        rgba_o, acc_o, (th, cam, opt) = both(key, tree, tr, w, h, fx, ndc=ndc, fy=fy)
    elif case == "non_orthonormal":
        rgba_o, acc_o, (th, cam, opt) = both(key, common.asymmetric_scene(), common.non_orthonormal(tr), w, h, fx, fy=fy)
    elif case == "compositing":
        th = ob.TreeHandle(common.asymmetric_scene())
        cam, opt = ob.make_camera(tr, w, h, fx, fy), ob.default_options()
        init, depth = common.mesh_underlay(w, h)
        rgba_o, _, _ = ob.render(th, cam, opt, offscreen=False, rgba_init=init, depth_init=depth)
        assert_ref_equal(key + "/rgba", rgba_o,
                         lambda: ob.ref_render(th, cam, opt, offscreen=False, rgba_init=init, depth_init=depth))
        free, _, _ = ob.render(th, cam, opt, offscreen=False, rgba_init=init)
        assert not np.array_equal(rgba_o, free), "the mesh depth must cut some rays short"
        return
    elif case == "probe":
        tree = common.asymmetric_scene()
        rgba_o, acc_o, (th, cam, opt) = both(key, tree, tr, w, h, fx, fy=fy, enable_probe=1, probe=common.ASYM_PROBE,
                                             probe_disp_size=30, basis_minmax=(0, tree.basis_dim - 1))
        a = np.zeros(tree.data_dim - 1, np.float32)
        ob.lib().or_probe_coeffs(C.byref(th.struct), C.byref(opt), a.ctypes.data)

        def ref_coeffs():
            b = np.zeros(tree.data_dim - 1, np.float32)
            ob.ref_lib().ref_probe_coeffs(C.byref(th.struct), C.byref(opt), b.ctypes.data)
            return b.view(np.uint32)
        assert_ref_equal(key + "/probe_coeffs", a.view(np.uint32), ref_coeffs)
        return                         # (ref_trace has no overlay: RGBA8 and the coefficients are the pin)
    else:
        name, o = case.split("-")
        fmt, bd = next(f for f in common.ASYM_FORMATS if f"{f[0]}{f[1]}" == name)
        rgba_o, acc_o, (th, cam, opt) = both(key, common.asymmetric_scene(fmt, bd), tr, w, h, fx, fy=fy,
                                             **common.ASYM_OPTIONS[o])
    assert_accum_equal(key, acc_o, th, cam, opt)
    assert (acc_o[..., 3] != 0).mean() >= 0.2, "the case shows too little"


def _swapped(v, i, j):
    v = np.array(v, np.float32).copy()
    v[[i, j]] = v[[j, i]]
    return v


def test_asymmetric_cases_have_teeth():
    """Every mix-up the asymmetric cases are there to catch changes the oracle's accumulators on at least
    half of the pixels either frame hits, with at least a fifth of the frame hit -- conditions on the
    cases, checked on the oracle alone."""
    import dataclasses
    from tests import aov_util as au
    tree = common.asymmetric_scene()
    tr, w, h, fx, fy = common.asymmetric_camera()
    s, o = tree.invradius3, tree.offset
    base = common.oracle_frame(tree, tr, w, h, fx, fy=fy)[1]
    rep = dataclasses.replace
    changes = {
        "fy := fx": (tree, fx, fx),
        "fx <-> fy": (tree, fy, fx),
        "scale x <-> y": (rep(tree, invradius3=_swapped(s, 0, 1)), fx, fy),
        "scale y <-> z": (rep(tree, invradius3=_swapped(s, 1, 2)), fx, fy),
        "scale := scale[0]": (rep(tree, invradius3=np.full(3, s[0], np.float32)), fx, fy),
        "offset x <-> y": (rep(tree, offset=_swapped(o, 0, 1)), fx, fy),
        "offset y <-> z": (rep(tree, offset=_swapped(o, 1, 2)), fx, fy),
    }
    frames = {k: (base, common.oracle_frame(t, tr, w, h, a, fy=b)[1]) for k, (t, a, b) in changes.items()}
    ntree, ntr, nw, nh, nfx, nfy, (ndw, ndh, ndf) = common.asymmetric_ndc_case()
    nbase = common.oracle_frame(ntree, ntr, nw, nh, nfx, fy=nfy, ndc=(ndw, ndh, ndf))[1]
    for k, ndc in (("ndc_width <-> ndc_height", (ndh, ndw, ndf)), ("ndc_focal := fx", (ndw, ndh, nfx))):
        frames[k] = (nbase, common.oracle_frame(ntree, ntr, nw, nh, nfx, fy=nfy, ndc=ndc)[1])
    for k, (a, b) in frames.items():
        hit = (a[..., 3] != 0) | (b[..., 3] != 0)
        differ = (a.view(np.uint32) != b.view(np.uint32)).any(-1)
        print(f"{k}: hit share {hit.mean():.2f}, differing share of the hit pixels {differ[hit].mean():.2f}")
        assert hit.mean() >= 0.2, f"{k}: only {hit.mean():.2f} of the frame is hit"
        assert differ[hit].mean() >= 0.5, f"{k}: only {differ[hit].mean():.2f} of the hit pixels differ"
    # delta_scale is per-ray state under this tree: it spans more than 10 % and takes > 500 values
    ds = au.restate(tree, tr, w, h, fx, fy=fy)[2]
    print(f"delta_scale: {np.unique(ds.view(np.uint32)).size} values, spread {(ds.max() - ds.min()) / ds.min():.3f}")
    assert (ds.max() - ds.min()) / ds.min() > 0.10
    assert np.unique(ds.view(np.uint32)).size > 500
