"""-m gpu: asymmetric geometry on the HIP kernels -- a tree whose scale[3] and offset[3] differ on every
axis, a camera with fx != fy on a frame with w != h, NDC numbers that are neither each other's nor the
camera's, a pose that is not orthonormal (tests/common.py: asymmetric, asymmetric_camera,
asymmetric_ndc_case, non_orthonormal).

Every other test renders a cube under a square pixel: there a swapped axis index, a scale[0] used for
all axes or an fy taken from fx changes nothing, delta_scale = 1 / |dir * scale| is one number for all
rays, and the world direction equals the march direction.  Here delta_scale differs from ray to ray by
tens of percent, so a value handed to the wrong ray (on refill, in the attenuation, in tmax / delta_scale,
in the VR_DEPTH_WORLD plane) changes the output.

Bar: everything bit-equal to the oracle (pinned to the reference on these very cases by
tests/test_oracle_vs_ref.py::test_asymmetric_geometry_bit_exact) or to the restatements tied to it, in
both FP models wherever the entry point has them."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import common
from tests import aov_util as au
from tests import query_util as qu
from tests import weights_util as wu
from tests.common import ob

pytestmark = pytest.mark.gpu

FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
# many refills per lane: a wave goes back to the ray queue after every round / with every free lane
KNOBS = [dict(refill_min=1), dict(refill_min=64, march_max=1), dict(waves_per_cu=1)]
KNOB_IDS = ["-".join(f"{a}{b}" for a, b in k.items()) for k in KNOBS]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def poses(n):
    return [common.camera_for(pose_idx=i, size=64)[0] for i in range(n)]


def chain_case():
    """The 26-level chain made asymmetric, the camera at the world point of its target."""
    tree, T = common.deep_chain_tree_n2(depth=26, basis_dim=4, seed=26)
    tree = common.asymmetric(tree)
    scale, offset = tree.invradius3.astype(np.float64), tree.offset.astype(np.float64)
    tr, w, h, f = common.camera_at(((T - offset) / scale).astype(np.float32), look_at=tuple((0.5 - offset) / scale))
    return tree, tr, w, h, 1.2 * f, 0.7 * f


def compare(torch, tree, tr, w, h, fx, fy, fp_mode, ndc=None, nan=False, **kw):
    """One frame on the GPU against the oracle: RGBA8 and accumulators bit for bit."""
    rgba_o, acc_o, cnt = common.oracle_frame(tree, tr, w, h, fx, fp_mode, ndc=ndc, fy=fy, **kw)
    rgba_g, acc_g = common.gpu_frame(torch, tree, tr, w, h, fx, fp_mode, ndc=ndc, fy=fy, **kw)
    if nan:
        common.assert_same_values(rgba_g, acc_g, rgba_o, acc_o)
    else:
        common.assert_parity(rgba_g, acc_g, rgba_o, acc_o)
    return acc_o, cnt


# ---- colour and accumulators ----------------------------------------------------------------------------------
@FP
@pytest.mark.parametrize("fmt,basis_dim", common.ASYM_FORMATS, ids=[f"{a}{b}" for a, b in common.ASYM_FORMATS])
def test_every_format_and_option(torch_cuda, fmt, basis_dim, fp_mode):
    """SH1 / SH9 / SH16 / SH25 / RGBA / SG4 / ASG4 (the FAST and the FULL flavours), plain and with rot_dirs,
    render_depth and render_bbox."""
    tree = common.asymmetric_scene(fmt, basis_dim)
    tr, w, h, fx, fy = common.asymmetric_camera()
    for name, kw in common.ASYM_OPTIONS.items():
        acc_o, _ = compare(torch_cuda, tree, tr, w, h, fx, fy, fp_mode, **kw)
        assert (acc_o[..., 3] != 0).mean() >= 0.2, name


@FP
def test_non_orthonormal_transform(torch_cuda, fp_mode):
    tr, w, h, fx, fy = common.asymmetric_camera()
    for fmt, bd in (("SH", 9), ("SH", 16)):
        acc_o, _ = compare(torch_cuda, common.asymmetric_scene(fmt, bd), common.non_orthonormal(tr), w, h, fx, fy,
                           fp_mode)
        assert (acc_o[..., 3] != 0).mean() >= 0.2


@FP
@pytest.mark.parametrize("fmt,basis_dim", [("SH", 16), ("SH", 9), ("RGBA", 0)], ids=["SH16", "SH9", "RGBA"])
def test_value_edge_tree(torch_cuda, fmt, basis_dim, fp_mode):
    tr, w, h, fx, fy = common.asymmetric_camera()
    tree = common.asymmetric(common.value_edge_tree(fmt, basis_dim, seed=9))
    acc_o, _ = compare(torch_cuda, tree, tr, w, h, fx, fy, fp_mode, nan=True)
    assert np.isnan(acc_o).any() and np.isfinite(acc_o).any()


@FP
@pytest.mark.parametrize("fmt,basis_dim", [("SH", 16), ("SH", 25), ("RGBA", 0)], ids=["SH16", "SH25", "RGBA"])
def test_fog_tree(torch_cuda, fmt, basis_dim, fp_mode):
    """Every sample a hit: shading under full pressure while delta_scale varies from ray to ray."""
    tr, w, h, fx, fy = common.asymmetric_camera()
    tree = common.asymmetric(common.fog_tree(fmt, basis_dim, seed=7, depth=5))
    _, cnt = compare(torch_cuda, tree, tr, w, h, fx, fy, fp_mode)
    assert cnt["hit_samples"] > 30 * w * h


# ---- the generic flavour: float descent ---------------------------------------------------------------------------
@FP
@pytest.mark.parametrize("kind", ["N3", "chain26"])
def test_generic_flavour(torch_cuda, kind, fp_mode):
    from volrend_amd import _abi, api
    if kind == "N3":
        tree = common.asymmetric(common.random_tree_general_n(N=3, depth=3, basis_dim=4, seed=503))
        tr, w, h, fx, fy = common.asymmetric_camera()
        kw = {}
    else:
        tree, tr, w, h, fx, fy = chain_case()
        kw = dict(step_size=1e-8)
    t = api.N3Tree.from_synth(tree)
    mode = t.info()["query_mode"]
    t.free_device()
    assert mode == _abi.QUERY_DESCENT
    _, cnt = compare(torch_cuda, tree, tr, w, h, fx, fy, fp_mode, **kw)
    assert cnt["hit_samples"] > 5000
    if kind == "chain26":
        assert cnt["child_reads"] > 8 * cnt["samples"]


# ---- compositing: tmax_bg /= delta_scale -----------------------------------------------------------------------------
@FP
def test_compositing_over_a_mesh_depth_plane(torch_cuda, fp_mode):
    tr, w, h, fx, fy = common.asymmetric_camera()
    tree = common.asymmetric_scene()
    init, depth = common.mesh_underlay(w, h)
    acc_o, _ = compare(torch_cuda, tree, tr, w, h, fx, fy, fp_mode, offscreen=False, rgba_init=init, depth_init=depth)
    free = common.oracle_frame(tree, tr, w, h, fx, fp_mode, fy=fy, offscreen=False, rgba_init=init)[1]
    assert not np.array_equal(acc_o, free), "the mesh depth must cut some rays short"


# ---- vr_render_aov ------------------------------------------------------------------------------------------------
@FP
def test_aov_batch_with_a_pose_per_frame(torch_cuda, fp_mode):
    """Both depth units and T over a five-pose batch.  VR_DEPTH_WORLD is D * delta_scale of the ray itself."""
    _, w, h, fx, fy = common.asymmetric_camera()
    want = au.check(torch_cuda, common.asymmetric_scene("SH", 16), poses(5), w, h, fx, fp_mode, fy=fy)
    for D, T, ds, stop in want:
        assert (D != 0).mean() >= 0.2 and stop.any()
        assert (ds.max() - ds.min()) / ds.min() > 0.10


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_aov_under_many_refills(torch_cuda, knobs):
    _, w, h, fx, fy = common.asymmetric_camera()
    au.check(torch_cuda, common.asymmetric_scene("SH", 16), poses(5), w, h, fx, 0, fy=fy, tree_tuning=knobs)
    au.check(torch_cuda, common.asymmetric_scene("SH", 9), poses(5), w, h, fx, 1, fy=fy, units=("world",),
             tree_tuning=knobs)


def test_aov_with_a_mesh_depth_plane(torch_cuda):
    tr, w, h, fx, fy = common.asymmetric_camera()
    init, depth = common.mesh_underlay(w, h)
    au.check(torch_cuda, common.asymmetric_scene(), [tr], w, h, fx, 0, fy=fy, offscreen=False, rgba_init=init,
             depth_init=depth)


# ---- vr_accumulate_weights ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights_reference(fp_mode):
    _, w, h, fx, fy = common.asymmetric_camera()
    tree, trs = common.asymmetric_scene("SH", 16), poses(3)
    mw, hc, _ = wu.restate(tree, trs, w, h, fx, fp_mode, fy=fy)
    mw.setflags(write=False)
    hc.setflags(write=False)
    return tree, trs, w, h, fx, fy, mw, hc


def check_weights(torch, tree, trs, w, h, fx, fy, want_mw, want_hits, fp_mode, ndc=None, tuning=None):
    from volrend_amd import api
    t = api.N3Tree.from_synth(tree, ndc=ndc)
    try:
        if tuning:
            t.set_tuning(**tuning)
        mw, hc = wu.accumulate(torch, t, w, h, fx, trs, fp_mode, tree=tree, fy=fy)
        torch.cuda.synchronize()
        assert t.status() == 0
        wu.assert_same_slots(wu.host(mw), wu.host(hc), *wu.expected(want_mw, want_hits))
    finally:
        t.free_device()
    assert (want_hits == 0).any() and (want_mw > 0).sum() > 500, "the case shows nothing"


@FP
def test_weights_every_slot(torch_cuda, fp_mode):
    tree, trs, w, h, fx, fy, mw, hc = weights_reference(fp_mode)
    check_weights(torch_cuda, tree, trs, w, h, fx, fy, mw, hc, fp_mode)


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_weights_under_many_refills(torch_cuda, knobs):
    tree, trs, w, h, fx, fy, mw, hc = weights_reference(0)
    check_weights(torch_cuda, tree, trs, w, h, fx, fy, mw, hc, 0, tuning=knobs)


# ---- point queries in world space, the probe ------------------------------------------------------------------------
QUERY_TREES = {
    "SH9": (lambda: common.asymmetric_scene("SH", 9), False),
    "N3": (lambda: common.asymmetric(common.random_tree_general_n(N=3, depth=4, basis_dim=4, seed=21)), False),
    "chain26": (lambda: common.asymmetric(common.deep_chain_tree_n2(26, basis_dim=4, seed=2)[0]), True),
}


@pytest.mark.parametrize("name", list(QUERY_TREES))
def test_world_points(torch_cuda, name):
    """VR_SPACE_WORLD: points from the inverse map (tree - offset) / scale; sigma, depth, local, coeffs and rgb
    word for word.  A float32 world coordinate resolves about 2^-25 of the chain's tree space: the points
    reach leaves of every depth down to the 25th level."""
    from volrend_amd import api
    factory, by_depth = QUERY_TREES[name]
    tree = factory()
    n = 20_000
    world = qu.to_world(tree, qu.point_set(tree, n, 120 + len(name), by_depth=by_depth))
    th = ob.TreeHandle(tree)
    ans = qu.oracle_answers(tree, th, world, "world")
    assert (ans["sigma"] > 0).mean() >= 0.25
    present = np.unique(qu.leaf_boxes(tree)[2])
    assert set(np.unique(ans["depth"]).tolist()) >= set(present[present <= 24].tolist())
    # the oracle's answer for a world point IS or_probe_coeffs there (pinned to the reference on this geometry)
    qu.same_words(ans["coeffs"][::16], qu.probe_coeffs(th, tree, world[::16]), f"{name}: or_probe_coeffs")
    t = api.N3Tree.from_synth(tree)
    try:
        qu.check_against_oracle(torch_cuda, t, tree, th, world, "world", name, ans)
        dirs = qu.direction_set(n, 130 + len(name))
        got = qu.gpu_query(torch_cuda, t, world, dirs, want=("rgb",), space="world")
        qu.same_words(got["rgb"], qu.recompose_rgb(tree, th, ans["coeffs"], dirs), f"{name} rgb")
    finally:
        t.free_device()


def test_world_grid(torch_cuda):
    """vr_query_grid in world space over a box whose three extents, and three resolutions, differ."""
    torch = torch_cuda
    from volrend_amd import api
    tree = common.asymmetric_scene("SH", 9)
    th = ob.TreeHandle(tree)
    lo, hi, res, direction = (-1.5, -1.0, -3.5), (2.2, 0.9, 2.3), (37, 5, 64), (0.3, -0.5, 0.8)
    coords = qu.grid_coords(lo, hi, res).reshape(-1, 3)
    ans = qu.oracle_answers(tree, th, coords, "world")
    assert (ans["sigma"] > 0).any() and np.unique(ans["depth"]).size > 2
    rgb = qu.recompose_rgb(tree, th, ans["coeffs"], np.broadcast_to(np.float32(direction), coords.shape))
    t = api.N3Tree.from_synth(tree)
    try:
        g = t.query_grid(lo, hi, res, direction, want=("sigma", "depth", "local", "coeffs", "rgb"), space="world")
        torch.cuda.synchronize()
        for k, want in (("sigma", ans["sigma"]), ("depth", ans["depth"]), ("local", ans["local"]),
                        ("coeffs", ans["coeffs"]), ("rgb", rgb)):
            got = g[k].cpu().numpy()
            assert got.shape[:3] == res, (k, got.shape)
            qu.same_words(got.reshape(want.shape), want, f"grid {k}")
    finally:
        t.free_device()


@FP
def test_probe_coeffs_and_overlay(torch_cuda, fp_mode):
    """A probe point whose three coordinates differ: vr_probe_coeffs and the overlay in the frame."""
    torch = torch_cuda
    from volrend_amd import _abi, api
    tree = common.asymmetric_scene()
    tr, w, h, fx, fy = common.asymmetric_camera()
    kw = dict(enable_probe=1, probe=common.ASYM_PROBE, probe_disp_size=30, basis_minmax=(0, tree.basis_dim - 1))
    compare(torch, tree, tr, w, h, fx, fy, fp_mode, **kw)
    n = tree.data_dim - 1
    want = np.zeros(n, np.float32)
    ob.lib().or_probe_coeffs(C.byref(ob.TreeHandle(tree).struct), C.byref(ob.default_options(**kw)), want.ctypes.data)
    assert (want != 0).any(), "the probe must sit in an occupied leaf"
    t = api.N3Tree.from_synth(tree)
    try:
        out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        o = api.RenderOptions(enable_probe=True, probe=common.ASYM_PROBE).to_c()
        _abi.check(_abi.lib().vr_probe_coeffs(t.handle, C.byref(o), out.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        t.free_device()


# ---- the asymmetric NDC tree -------------------------------------------------------------------------------------
@FP
def test_ndc_colour_aov_and_weights(torch_cuda, fp_mode):
    tree, tr, w, h, fx, fy, ndc = common.asymmetric_ndc_case()
    acc_o, _ = compare(torch_cuda, tree, tr, w, h, fx, fy, fp_mode, ndc=ndc)
    assert (acc_o[..., 3] != 0).mean() >= 0.2
    tr2 = tr.copy()
    tr2[9:12] += np.float32(0.05)
    au.check(torch_cuda, tree, [tr, tr2], w, h, fx, fp_mode, ndc=ndc, fy=fy)
    mw, hc, _ = wu.restate(tree, [tr, tr2], w, h, fx, fp_mode, ndc=ndc, fy=fy)
    check_weights(torch_cuda, tree, [tr, tr2], w, h, fx, fy, mw, hc, fp_mode, ndc=ndc)


# ---- tile shards ---------------------------------------------------------------------------------------------------
def test_tile_shards_reassemble(torch_cuda):
    """world = 3, tiles of 16 x 8, COMPACT layout: a ray generation that takes a tile axis for a frame axis
    (or fx for fy inside a tile) shows under this camera."""
    torch = torch_cuda
    from volrend_amd import api
    tree = common.asymmetric_scene("SH", 16)
    tr, w, h, fx, fy = common.asymmetric_camera()
    want = common.oracle_frame(tree, tr, w, h, fx, fy=fy)[0]
    t = api.N3Tree.from_synth(tree)
    try:
        cam = api.Camera(w, h, fx, fy)
        cam.transform = np.asarray(tr, np.float32)
        world, tw, th = 3, 16, 8
        sh0 = api.TileShard(tw, th, 0, world, compact=True)
        gathered = torch.zeros((world, api.compact_bytes(w, h, sh0)), dtype=torch.uint8, device="cuda")
        frame = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        for r in range(world):
            api.launch_renderer(t, cam, api.RenderOptions(), frame, None, None, True,
                                shard=api.TileShard(tw, th, r, world, compact=False))
            api.launch_renderer(t, cam, api.RenderOptions(), gathered[r], None, None, True,
                                shard=api.TileShard(tw, th, r, world, compact=True))
        out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        api.assemble_tiles(out, gathered, w, h, sh0)
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    assert np.array_equal(frame.cpu().numpy(), want), "FRAME layout"
    assert np.array_equal(out.cpu().numpy(), want), "COMPACT layout, assembled"
