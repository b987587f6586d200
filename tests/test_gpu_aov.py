"""vr_render_aov on the GPU: the depth and transmittance planes are bit-equal to the restatement of
trace_ray's loop (tests/cpp/aov_restatement.c, tied to the oracle by tests/test_aov_restatement.py)
on EVERY pixel, NaNs in the same places, and colour / accum of the same launch equal what
vr_render_batch writes for the same arguments."""
import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests.aov_util import SENTINEL, assert_colour_unchanged, check, host_f32, render_both, sentinel_planes

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


FORMATS = [("SH", 1), ("SH", 4), ("SH", 9), ("SH", 16), ("SH", 25), ("RGBA", 0), ("SG", 9), ("ASG", 4)]


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
@pytest.mark.parametrize("fmt,basis_dim", FORMATS, ids=[f"{a}{b}" for a, b in FORMATS])
def test_every_format_both_fp_models_both_units(torch_cuda, fmt, basis_dim, fp_mode):
    tree = common.small_scene(depth=5, basis_dim=basis_dim, fmt=fmt, seed=20 + basis_dim)
    tr, w, h, f = common.camera_for(pose_idx=2, size=96)
    want = check(torch_cuda, tree, [tr], w, h, f, fp_mode)
    D, T, _, stop = want[0]
    assert (D != 0).sum() > 500 and stop.any() and (~stop & (D != 0)).any()


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
@pytest.mark.parametrize("basis_dim", [0, 4, 9, 16, 25])
def test_blocked_brick_order(torch_cuda, basis_dim, fp_mode):
    """Bricks in 4 x 4 x 2 line blocks (the BLK flavours).  A small tree only gets bricks under a small top
    grid: depth 7 under a 2^2 top grid with 8^3 bricks, the (2, 3, 1) geometry of tests/test_gpu_parity.py."""
    from volrend_amd import api
    tree = common.small_scene(depth=7, basis_dim=basis_dim, fmt="SH" if basis_dim else "RGBA", seed=1201)
    tr, w, h, f = common.camera_for(pose_idx=3, size=72)
    api.set_tuning(top_levels=2, brick_levels=3, brick_blocked=1)
    try:
        t = api.N3Tree.from_synth(tree)
        blocked = t.info()["brick_blocked"]
        t.free_device()
        assert blocked == 1
        want = check(torch_cuda, tree, [tr], w, h, f, fp_mode, units=("world",))
    finally:
        api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    assert (want[0][0] != 0).sum() > 500


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
@pytest.mark.parametrize("N", [3, 4])
def test_general_branching_factor(torch_cuda, N, fp_mode):
    tree = common.random_tree_general_n(N=N, depth=3, basis_dim=4, seed=N)
    tr, w, h, f = common.camera_for(pose_idx=1, size=64)
    want = check(torch_cuda, tree, [tr], w, h, f, fp_mode)
    assert (want[0][0] != 0).any()


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
def test_26_level_chain_takes_the_float_descent(torch_cuda, fp_mode):
    tree, T = common.deep_chain_tree_n2(depth=26, basis_dim=4, seed=26)
    tr, w, h, f = common.camera_at(T)
    want = check(torch_cuda, tree, [tr], w, h, f, fp_mode, step_size=1e-8)
    assert (want[0][0] != 0).any()


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
def test_ndc_tree(torch_cuda, fp_mode):
    tree = common.small_scene(depth=5, basis_dim=4, seed=51)
    want = check(torch_cuda, tree, [au.NDC_TRANSFORM], 96, 72, 80.0, fp_mode, ndc=au.NDC)
    assert (want[0][0] != 0).any()


def test_render_bbox_and_options(torch_cuda):
    tree = common.small_scene(depth=6, basis_dim=9, seed=41)
    tr, w, h, f = common.camera_for(pose_idx=3, size=72)
    full = au.restate(tree, tr, w, h, f)
    want = check(torch_cuda, tree, [tr], w, h, f, render_bbox=(0.1, 0.2, 0.0, 0.8, 0.9, 0.7))
    assert not np.array_equal(want[0][0], full[0])
    for kw in (au.OPTION_SETS["no_early_stop"], au.OPTION_SETS["coarse"],
               dict(step_size=1e-3, sigma_thresh=0.5, stop_thresh=0.1, background_brightness=0.25),
               dict(rot_dirs=(0.3, -0.2, 0.9), basis_minmax=(1, 5))):
        check(torch_cuda, tree, [tr], w, h, f, units=("world",), **kw)


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
def test_mesh_depth_plane(torch_cuda, fp_mode):
    """offscreen = 0: composite over an existing frame, tmax from a mesh depth plane."""
    tree = common.small_scene(depth=5, basis_dim=9, seed=71)
    tr, w, h, f = common.camera_for(pose_idx=4, size=64)
    rng = np.random.default_rng(5)
    init = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    depth = rng.uniform(2.0, 6.0, size=(h, w)).astype(np.float32)
    want = check(torch_cuda, tree, [tr], w, h, f, fp_mode, offscreen=False, rgba_init=init, depth_init=depth)
    free = au.restate(tree, tr, w, h, f, fp_mode)
    assert not np.array_equal(want[0][0], free[0]), "the mesh depth must cut some rays short"


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
@pytest.mark.parametrize("name", ["SH16", "SH9", "SH25", "RGBA", "SG7", "SH4_negative_thresh", "SH16_stop_ge_1",
                                  "RGBA_never_stop"])
def test_value_edge_trees(torch_cuda, name, fp_mode):
    """NaN / inf / subnormal densities and coefficients: NaNs of the planes sit where the restatement's do."""
    tree, tr, w, h, f, kw = common.value_case(name)
    check(torch_cuda, tree, [tr], w, h, f, fp_mode, **kw)


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
@pytest.mark.parametrize("name", ["SH16", "SH25", "RGBA", "SH16_negative_thresh"])
def test_fog_trees(torch_cuda, name, fp_mode):
    """Every sample a hit: ~90 terms per depth sum, the colour ring under full pressure."""
    tree, tr, w, h, f, kw = common.fog_case(name)
    want = check(torch_cuda, tree, [tr], w, h, f, fp_mode, **kw)
    assert (want[0][0] != 0).sum() > 1000


def test_ragged_image_and_a_pose_that_misses(torch_cuda):
    tree = common.small_scene(depth=4, basis_dim=4, seed=61)
    tr, _, _, f = common.camera_for(pose_idx=1, size=61)
    tr2 = np.array(tr, np.float32).copy()
    tr2[9:12] = [50.0, 50.0, 50.0]
    want = check(torch_cuda, tree, [tr, tr2], 61, 37, f)
    assert (want[0][0] != 0).any()
    assert (want[1][0] == 0).all() and (want[1][1] == 1).all()     # every ray misses: D = 0, T = 1


@pytest.mark.parametrize("which", ["depth", "transmittance"])
def test_one_plane_only_and_padded_pitch(torch_cuda, which):
    """Only one plane asked for; rows padded by 5 words whose bytes must stay untouched."""
    from volrend_amd import api
    tree = common.small_scene(depth=5, basis_dim=16, seed=36)
    tr, w, h, f = common.camera_for(pose_idx=2, size=80)
    D, T, ds, _ = au.restate(tree, tr, w, h, f)
    t = api.N3Tree.from_synth(tree)
    try:
        r = render_both(torch_cuda, t, w, h, f, [tr], units="world", want=(which,), pad_words=5)
    finally:
        t.free_device()
    assert_colour_unchanged(r)
    other = "trans" if which == "depth" else "depth"
    assert r[other] is None
    plane = r["depth" if which == "depth" else "trans"][0]
    au.assert_same_bits(plane[:, :w], au.world_depth(D, ds) if which == "depth" else T, which)
    assert (plane[:, w:].view(np.int32) == SENTINEL).all(), "padding was written"


def test_batches_with_a_pose_per_frame_on_two_streams(torch_cuda):
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=5, basis_dim=9, seed=1301)
    w, h, f = 150, 107, 170.0
    trs = [common.camera_for(pose_idx=i, size=64)[0] for i in range(6)]
    want = [au.restate(tree, tr, w, h, f) for tr in trs]
    t = api.N3Tree.from_synth(tree)
    t.reserve(w, h, 3)
    cam = api.Camera(w, h, f, f)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    imgs = torch.zeros((6, h, w, 4), dtype=torch.uint8, device="cuda")
    dp, tp = sentinel_planes(torch, 6, h, w), sentinel_planes(torch, 6, h, w)
    torch.cuda.synchronize()
    try:
        for rep in range(3):                       # the two streams alternate over the two halves
            for s, lo in ((0, 0), (1, 3)):
                with torch.cuda.stream(streams[s]):
                    api.launch_renderer_batch(t, cam, trs[lo:lo + 3], api.RenderOptions(), list(imgs[lo:lo + 3]),
                                              streams[s], True,
                                              aov=[api.AovPlanes(dp[i], tp[i]) for i in range(lo, lo + 3)],
                                              depth_units="tree")
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    for i, (D, T, _, _) in enumerate(want):
        assert np.array_equal(imgs[i].cpu().numpy(), common.oracle_frame(tree, trs[i], w, h, f)[0]), i
        au.assert_same_bits(host_f32(dp[i]), D, f"depth frame {i}")
        au.assert_same_bits(host_f32(tp[i]), T, f"transmittance frame {i}")


@pytest.mark.parametrize("compact", [False, True], ids=["frame", "compact"])
def test_tile_shards_write_only_their_own_pixels(torch_cuda, compact):
    """Planes are addressed in frame position in both layouts; a rank leaves the pixels of other ranks'
    tiles untouched, and the ranks' planes together are the unsharded ones."""
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=5, basis_dim=4, seed=81)
    tr, w, h, f = common.camera_for(pose_idx=6, size=100)
    D, T, ds, _ = au.restate(tree, tr, w, h, f)
    Dw = au.world_depth(D, ds)
    world, tw, th = 3, 32, 16
    ys, xs = np.mgrid[0:h, 0:w]
    owner = ((ys // th) * ((w + tw - 1) // tw) + xs // tw) % world
    t = api.N3Tree.from_synth(tree)
    try:
        seen = np.zeros((h, w), bool)
        for rank in range(world):
            sh = api.TileShard(tw, th, rank, world, compact=compact)
            r = render_both(torch, t, w, h, f, [tr], units="world", shard=sh)
            assert_colour_unchanged(r, f"rank {rank}")
            mine = owner == rank
            for plane, want in ((r["depth"][0], Dw), (r["trans"][0], T)):
                assert (plane.view(np.int32)[~mine] == SENTINEL).all(), f"rank {rank} wrote foreign pixels"
                assert au.same_bits(plane, want)[mine].all(), f"rank {rank}"
            seen |= mine
        assert seen.all()
    finally:
        t.free_device()


@pytest.mark.parametrize("knobs", [dict(refill_min=1), dict(refill_min=64, march_max=1), dict(march_max=64),
                                   dict(waves_per_cu=1), dict(waves_per_cu=3, raygen_waves=1),
                                   dict(raygen_waves=4, frame_group=1), dict(frame_group=2, super_block=3)],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_scheduling_knobs_change_nothing(torch_cuda, knobs):
    tree = common.small_scene(depth=5, basis_dim=16, seed=1401)
    w, h, f = 90, 70, 100.0
    trs = [common.camera_for(pose_idx=i, size=64)[0] for i in range(3)]
    check(torch_cuda, tree, trs, w, h, f, units=("world",), tree_tuning=knobs)
    tree = common.small_scene(depth=5, basis_dim=4, seed=1402)
    check(torch_cuda, tree, trs, w, h, f, 1, units=("tree",), tree_tuning=knobs)
