"""-m gpu: the lead-in march of ray generation (include/volrend_hip.h vr_tree_head_stats; tuning keys head_march,
head_min_lanes, head_max).

Ray generation takes a ray's samples in front of its first hit sample and hands the ray over at the t it has
reached; a ray that reaches tmax without a hit sample ends there.  The sample sequence is the march kernel's own,
so every comparison here is equality: RGBA8 bytes and fp32 accumulators against the oracle and against the same
launch with head_march = 0, whatever head_min_lanes and head_max say.  Depth-6 trees, frames of 96 x 80 pixels
(12 x 10 blocks) and one of 100 x 52 (ragged blocks on both edges).  status() stays 0."""
import functools

import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import cull_util as cu
from tests.common import ob

pytestmark = pytest.mark.gpu

W, H = 96, 80
F = 96 * 1111.111 / 800.0
FORMATS = {"SH1": ("SH", 1), "SH9": ("SH", 9), "SH16": ("SH", 16), "SH25": ("SH", 25), "RGBA": ("RGBA", 0)}
FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
DEFAULTS = dict(head_march=1, head_min_lanes=0, head_max=0, block_cull=1, max_iter=1 << 22)
TO_THE_END = dict(head_min_lanes=1, head_max=1 << 20)     # every ray marches to its first hit or its tmax
ZERO = {"entered": 0, "retired": 0, "samples": 0}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


@functools.lru_cache(maxsize=None)
def scene(name, depth=6):
    fmt, bd = FORMATS[name]
    return common.small_scene(depth=depth, basis_dim=bd, fmt=fmt, seed=500 + bd)


def pose(i):
    return common.camera_for(pose_idx=(2, 5, 7)[i], size=W)[0]


@functools.lru_cache(maxsize=None)
def oracle_pose(name, i, fp_mode, w=W, h=H):
    """-> (rgba, accum) of pose i of the orbit; computed once, shared, never written to."""
    r, a, _ = common.oracle_frame(scene(name), pose(i), w, h, F, fp_mode)
    return r, a


def oracle(name, n, fp_mode, w=W, h=H):
    frames = [oracle_pose(name, i, fp_mode, w, h) for i in range(n)]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])


def launch(torch, t, trs, w=W, h=H, f=F, fp_mode=0, tuning=None, fy=None, offscreen=True, rgba_init=None, **opt_kw):
    """One vr_render_batch launch under DEFAULTS + tuning -> (rgba [n, h, w, 4], accum [n, h, w, 4], head_stats)."""
    from volrend_amd import api
    t.set_tuning(**dict(DEFAULTS, **(tuning or {})))
    t.head_stats(reset=True)
    cam = api.Camera(w, h, f, f if fy is None else fy)
    if rgba_init is None:
        img = torch.zeros((len(trs), h, w, 4), dtype=torch.uint8, device="cuda")
    else:
        img = torch.from_numpy(np.broadcast_to(rgba_init, (len(trs),) + rgba_init.shape).copy()).cuda()
    acc = torch.zeros((len(trs), h, w, 4), dtype=torch.float32, device="cuda")
    api.launch_renderer_batch(t, cam, trs, api.RenderOptions(**opt_kw), list(img), None, offscreen, accums=list(acc),
                              fp_mode=fp_mode)
    torch.cuda.synchronize()
    assert t.status() == 0
    return img.cpu().numpy(), acc.cpu().numpy(), t.head_stats(reset=True)


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: RGBA8 differs"
    au.assert_same_bits(got[1], want[1], f"{what}: accumulators")


@FP
@pytest.mark.parametrize("n", [1, 3])      # 4 / 16 waves per ray-generation workgroup, row-major / super-block order
@pytest.mark.parametrize("name", list(FORMATS))
def test_formats_modes_and_launch_sizes(torch_cuda, name, n, fp_mode):
    from volrend_amd import api
    trs, want = [pose(i) for i in range(n)], oracle(name, n, fp_mode)
    t = api.N3Tree.from_synth(scene(name))
    try:
        on = launch(torch_cuda, t, trs, fp_mode=fp_mode)
        end = launch(torch_cuda, t, trs, fp_mode=fp_mode, tuning=TO_THE_END)
        off = launch(torch_cuda, t, trs, fp_mode=fp_mode, tuning=dict(head_march=0))
    finally:
        t.free_device()
    same(on, want, "lead-in on / oracle")
    same(end, want, "lead-in to the end / oracle")
    same(off, want, "lead-in off / oracle")
    assert off[2] == ZERO
    for st in (on[2], end[2]):
        assert 0 < st["entered"] <= n * W * H and st["retired"] <= st["entered"] and st["samples"] > 0, st
    assert end[2]["entered"] == on[2]["entered"] and end[2]["samples"] >= on[2]["samples"]
    assert end[2]["retired"] >= on[2]["retired"]


@pytest.mark.parametrize("n", [1, 3])
def test_ragged_frame(torch_cuda, n):
    """100 x 52: the last block column holds 4 pixels of a row, the last block row 4 rows."""
    from volrend_amd import api
    w, h = 100, 52
    trs, want = [pose(i) for i in range(n)], oracle("SH9", n, 0, w, h)
    t = api.N3Tree.from_synth(scene("SH9"))
    try:
        for tuning in ({}, TO_THE_END, dict(head_max=2, head_min_lanes=1), dict(head_march=0)):
            same(launch(torch_cuda, t, trs, w, h, tuning=tuning), want, f"100 x 52, {tuning}")
    finally:
        t.free_device()


@FP
def test_line_block_brick_order(torch_cuda, fp_mode):
    """Bricks in 4 x 4 x 2 line blocks, forced by the upload-time key: the lead-in reads them in that order."""
    from volrend_amd import api
    trs, want = [pose(i) for i in range(3)], oracle("SH16", 3, fp_mode)
    api.set_tuning(top_levels=2, brick_levels=3, brick_blocked=1)
    try:
        t = api.N3Tree.from_synth(scene("SH16"))
    finally:
        api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    try:
        assert t.info()["brick_blocked"] == 1
        on = launch(torch_cuda, t, trs, fp_mode=fp_mode, tuning=TO_THE_END)
        off = launch(torch_cuda, t, trs, fp_mode=fp_mode, tuning=dict(head_march=0))
    finally:
        t.free_device()
    same(on, want, "blocked bricks, lead-in on / oracle")
    same(off, want, "blocked bricks, lead-in off / oracle")
    assert on[2]["samples"] > 0 and off[2] == ZERO


@pytest.mark.parametrize("n", [1, 3])
def test_hand_over_points(torch_cuda, n):
    """Hand-over in the middle of the lead-in, at once, and at its end: the same bytes."""
    from volrend_amd import api
    trs, want = [pose(i) for i in range(n)], oracle("SH16", n, 0)
    t = api.N3Tree.from_synth(scene("SH16"))
    stats = {}
    try:
        for head_max in (1, 2, 3, 7, 0):
            for min_lanes in (1, 16, 64):
                got = launch(torch_cuda, t, trs, tuning=dict(head_max=head_max, head_min_lanes=min_lanes))
                same(got, want, f"head_max {head_max}, head_min_lanes {min_lanes}")
                stats[head_max, min_lanes] = got[2]
    finally:
        t.free_device()
    entered = stats[1, 1]["entered"]
    assert entered > 0 and all(s["entered"] == entered for s in stats.values())
    for (head_max, min_lanes), s in stats.items():
        if head_max:
            assert s["samples"] <= head_max * entered, (head_max, min_lanes, s)
    # more rounds, or a lower bound on the marching lanes, never march fewer samples
    for min_lanes in (1, 16, 64):
        run = [stats[m, min_lanes]["samples"] for m in (1, 2, 3, 7)]
        assert run == sorted(run) and run[0] <= run[-1]
    for head_max in (1, 2, 3, 7, 0):
        assert stats[head_max, 1]["samples"] >= stats[head_max, 16]["samples"] >= stats[head_max, 64]["samples"]
    assert stats[7, 1]["samples"] > stats[1, 1]["samples"] > 0


def no_hit_case():
    """-> (tree, transform, per-pixel samples, per-pixel hits, counters) of a frame in which blocks hold both rays
    with a hit and rays that cross the volume without one."""
    tree, tr = scene("SH9"), pose(1)
    th, opt = ob.TreeHandle(tree), ob.default_options()
    samples, hits, cnt = ob.render_maps(th, ob.make_camera(tr, W, H, F), opt, 0)
    return tree, tr, samples, hits, cnt


def test_rays_without_a_hit(torch_cuda):
    from volrend_amd import api
    tree, tr, samples, hits, cnt = no_hit_case()
    # the expected counts, from the oracle alone
    marched, no_hit = samples > 0, (samples > 0) & (hits == 0)
    assert cnt["rays_hit_box"] == int(marched.sum()) > 0
    blocks = cu.hit_blocks(hits)
    in_hit_block = np.repeat(np.repeat(blocks, 8, 0), 8, 1)[:H, :W]
    assert int((no_hit & in_hit_block).sum()) > 0, "no block holds rays with and without a hit"
    assert int(no_hit.sum()) < int(marched.sum())
    want = oracle_pose("SH9", 1, 0)
    t = api.N3Tree.from_synth(tree)
    try:
        got = launch(torch_cuda, t, [tr], tuning=dict(TO_THE_END, block_cull=0))
        assert got[2]["entered"] == cnt["rays_hit_box"]
        assert got[2]["retired"] == int(no_hit.sum())
        assert got[2]["samples"] <= cnt["samples"] - cnt["hit_samples"]
        same(got, (want[0][None], want[1][None]), "to the end, no cull / oracle")
        # with the cull the culled blocks' rays never enter
        culled = launch(torch_cuda, t, [tr], tuning=TO_THE_END)
        same(culled, (want[0][None], want[1][None]), "to the end, cull / oracle")
        assert culled[2]["entered"] - culled[2]["retired"] == got[2]["entered"] - got[2]["retired"]
        # such a pixel over a background brightness, and over the frame's own pixels and a mesh depth
        for tuning in (TO_THE_END, dict(head_march=0)):
            bg = launch(torch_cuda, t, [tr], tuning=tuning, background_brightness=0.5)
            r, a, _ = common.oracle_frame(tree, tr, W, H, F, background_brightness=0.5)
            same(bg, (r[None], a[None]), f"background 0.5, {tuning}")
        rgba_init, _ = common.mesh_underlay(W, H)
        r, a, _ = common.oracle_frame(tree, tr, W, H, F, offscreen=False, rgba_init=rgba_init)
        for tuning in (TO_THE_END, {}, dict(head_march=0)):
            over = launch(torch_cuda, t, [tr], tuning=tuning, offscreen=False, rgba_init=rgba_init)
            same(over, (r[None], a[None]), f"over rgba_init, {tuning}")
    finally:
        t.free_device()


def test_lead_in_of_zero(torch_cuda):
    from volrend_amd import api
    tree = scene("SH9")
    t = api.N3Tree.from_synth(tree)
    try:
        # every sample is a hit: nothing moves
        for tuning in ({}, TO_THE_END):
            neg = launch(torch_cuda, t, [pose(0)], tuning=tuning, sigma_thresh=-1.0)
            r, a, _ = common.oracle_frame(tree, pose(0), W, H, F, sigma_thresh=-1.0)
            same(neg, (r[None], a[None]), "sigma_thresh = -1")
            assert neg[2]["entered"] > 0 and neg[2]["retired"] == 0 and neg[2]["samples"] == 0, neg[2]
        # the camera in the middle of an occupied cell: the rays start in a dense leaf
        g, grid = cu.occupancy(tree)
        scale, offset = np.asarray(tree.invradius3, np.float64), np.asarray(tree.offset, np.float64)
        to_world = lambda p: tuple(((np.asarray(p) - offset) / scale).astype(np.float32))
        tr, w, h, fi = common.camera_at(to_world((cu.boundary_cells(grid)[0] + 0.5) / (1 << g)),
                                        look_at=to_world((0.52, 0.47, 0.55)), size=W, focal=60.0)
        r, a, _ = common.oracle_frame(tree, tr, w, h, fi)
        for tuning in ({}, TO_THE_END, dict(head_march=0)):
            same(launch(torch_cuda, t, [tr], w, h, fi, tuning=tuning), (r[None], a[None]), f"camera inside, {tuning}")
        # a render_bbox inside the unit cube, and one beyond it (samples outside are clamped into the border leaves)
        for bbox in ((0.1, 0.2, 0.0, 0.8, 0.9, 0.7), (-0.2, -0.1, 0.0, 1.3, 1.1, 1.2)):
            r, a, _ = common.oracle_frame(tree, pose(2), W, H, F, render_bbox=bbox)
            for tuning in ({}, TO_THE_END, dict(head_march=0)):
                got = launch(torch_cuda, t, [pose(2)], tuning=tuning, render_bbox=bbox)
                same(got, (r[None], a[None]), f"render_bbox {bbox}, {tuning}")
                assert (got[2]["entered"] > 0) == (tuning.get("head_march", 1) == 1)
    finally:
        t.free_device()


@FP
@pytest.mark.parametrize("tuning", [{}, dict(TO_THE_END, block_cull=0), dict(head_max=3, head_min_lanes=1)],
                         ids=["auto", "to_the_end", "three_rounds"])
def test_aov_planes(torch_cuda, tuning, fp_mode):
    """Depth (both depth units) and transmittance of every pixel against the restatement of the march."""
    from volrend_amd import api
    tree, trs = scene("SH16"), [pose(i) for i in range(3)]
    au.check(torch_cuda, tree, trs, W, H, F, fp_mode, tree_tuning=dict(DEFAULTS, **tuning))
    t = api.N3Tree.from_synth(tree)
    try:
        t.set_tuning(**dict(DEFAULTS, **tuning))
        t.head_stats(reset=True)
        au.render_both(torch_cuda, t, W, H, F, trs, fp_mode)
        st = t.head_stats(reset=True)
    finally:
        t.free_device()
    assert st["entered"] > 0 and st["entered"] % 2 == 0 and st["samples"] % 2 == 0, st   # the colour and the AOV launch


def test_compact_tile_shards(torch_cuda):
    """Two ranks' compact shards, assembled, equal the unsharded frame."""
    torch = torch_cuda
    from volrend_amd import api
    want = oracle_pose("SH9", 0, 0)
    t = api.N3Tree.from_synth(scene("SH9"))
    cam = api.Camera(W, H, F, F)
    cam.transform = pose(0)
    try:
        t.set_tuning(**dict(DEFAULTS, **TO_THE_END))
        whole = launch(torch, t, [pose(0)], tuning=TO_THE_END)
        for world, tw, th in [(2, 16, 8), (2, 96, 8)]:
            sh0 = api.TileShard(tw, th, 0, world, compact=True)
            gathered = torch.zeros((world, api.compact_bytes(W, H, sh0)), dtype=torch.uint8, device="cuda")
            t.head_stats(reset=True)
            for r in range(world):
                api.launch_renderer(t, cam, api.RenderOptions(), gathered[r], None, None, True,
                                    shard=api.TileShard(tw, th, r, world, compact=True))
            out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
            api.assemble_tiles(out, gathered, W, H, sh0)
            torch.cuda.synchronize()
            assert t.status() == 0
            assert np.array_equal(out.cpu().numpy(), whole[0][0]), (world, tw, th)
            assert t.head_stats(reset=True) == whole[2], (world, tw, th)
    finally:
        t.free_device()
    assert np.array_equal(whole[0][0], want[0])


def test_off_where_it_must_be(torch_cuda):
    """Launches that take the parent's path leave the counters at zero."""
    torch = torch_cuda
    from volrend_amd import api
    tree, tr = scene("SH9"), pose(0)
    want = oracle_pose("SH9", 0, 0)
    t = api.N3Tree.from_synth(tree)
    cam = api.Camera(W, H, F, F)
    try:
        assert launch(torch, t, [tr])[2]["entered"] > 0           # (the control: this tree's plain launch marches)
        # the FULL flavour: depth visualisation, counters
        depth = launch(torch, t, [tr], render_depth=1)
        r, a, _ = common.oracle_frame(tree, tr, W, H, F, render_depth=1)
        same(depth, (r[None], a[None]), "render_depth")
        assert depth[2] == ZERO
        t.set_tuning(**DEFAULTS)
        img = torch.zeros((1, H, W, 4), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros((1, 7), dtype=torch.int64, device="cuda")
        api.launch_renderer_batch(t, cam, [tr], api.RenderOptions(), list(img), None, True, counters=list(cnt))
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy()[0], want[0]) and t.status() == 0
        _, _, oc = common.oracle_frame(tree, tr, W, H, F)
        assert [int(v) for v in cnt[0].cpu()] == list(oc.values())     # (the oracle's, to the integer)
        assert t.head_stats(reset=True) == ZERO
        # a ray list
        n = 1000
        rng = np.random.default_rng(5)
        origins = torch.from_numpy(np.tile(np.asarray(tr[9:12], np.float32), (n, 1))).cuda()
        dirs = torch.from_numpy((-np.asarray(tr[9:12], np.float32) + rng.normal(0, 0.3, (n, 3))).astype(np.float32)).cuda()
        out = t.render_rays(origins, dirs, api.RenderOptions())
        torch.cuda.synchronize()
        assert out["accum"].shape == (n, 4) and float(out["accum"][:, 3].max()) > 0 and t.status() == 0
        assert t.head_stats(reset=True) == ZERO
        # max_iter below its default (and far above what a ray of this scene needs)
        low = launch(torch, t, [tr], tuning=dict(max_iter=(1 << 22) - 1))
        same(low, (want[0][None], want[1][None]), "max_iter lowered")
        assert low[2] == ZERO
        assert launch(torch, t, [tr])[2]["entered"] > 0
    finally:
        t.free_device()
    # a tree off the N == 2 lookup path
    tree3 = common.random_tree_general_n(3, 3, 4, "SH", seed=703)
    r, a, _ = common.oracle_frame(tree3, tr, W, H, F)
    t = api.N3Tree.from_synth(tree3)
    try:
        got = launch(torch, t, [tr])
    finally:
        t.free_device()
    same(got, (r[None], a[None]), "N = 3")
    assert got[2] == ZERO


@FP
@pytest.mark.parametrize("case", ["SH16", "SH9_thresh_edge", "RGBA", "SH4_negative_thresh", "SH25"])
def test_non_finite_values(torch_cuda, case, fp_mode):
    """Leaves with sigma NaN, +-inf, -0 and subnormal, and NaN / inf colour coefficients (common.value_case)."""
    from volrend_amd import api
    tree, tr, w, h, f, kw = common.value_case(case)
    sig = tree.data.reshape(-1, tree.data_dim)[:, -1]
    assert np.isnan(sig).any() and np.isposinf(sig).any() and (sig.view(np.uint16) == 0x8000).any()
    assert np.isnan(tree.data.reshape(-1, tree.data_dim)[:, :-1]).any()
    r, a, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode, **kw)
    t = api.N3Tree.from_synth(tree)
    try:
        for tuning in ({}, TO_THE_END, dict(head_max=2, head_min_lanes=1), dict(head_march=0)):
            got = launch(torch_cuda, t, [tr], w, h, f, fp_mode, tuning=tuning, **kw)
            common.assert_same_values(got[0][0], got[1][0], r, a, f"{case}, {tuning}")
    finally:
        t.free_device()
