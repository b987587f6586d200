"""-m gpu: the block cull of ray generation (include/volrend_hip.h vr_tree_cull_stats, tuning key block_cull).

Depth-6 trees on 96 x 96 frames: a 64^3 occupancy grid and 12 x 12 blocks of 8 x 8 pixels.
  * Frames, accumulators and AOV planes with the cull on are byte-equal to those with it off and to the oracle:
    one frame, three frames (the super-block ray order), tile shards, both FP models.
  * The culled count is positive, never above the number of blocks the oracle's hit map shows empty, and zero
    where the cull must be off: sigma_thresh < 0, an NDC tree, a camera inside the volume.
  * After update_data and after a tree step that move the density into the opposite octant, the picture is the
    oracle's picture of the new values: the occupancy follows the node words.
  * status() stays 0."""
import dataclasses

import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import cull_util as cu
from tests import query_util as qu
from tests.common import ob

pytestmark = pytest.mark.gpu

SIZE = 96
TREES = {"SH16": dict(depth=6, basis_dim=16, seed=3), "SH9": dict(depth=6, basis_dim=9, seed=41)}
FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
TREE = pytest.mark.parametrize("name", list(TREES))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def scene(name):
    return common.small_scene(**TREES[name])


def poses(n):
    return [common.camera_for(pose_idx=i, size=SIZE)[0] for i in (2, 5, 7)[:n]]


def render(torch, t, trs, w, h, fx, fp_mode=0, cull=1, shards=(None,), fy=None, **opt_kw):
    """One launch per shard into the same frames -> (rgba [n, h, w, 4], accum [n, h, w, 4], cull_stats summed)."""
    from volrend_amd import api
    t.set_tuning(block_cull=cull)
    t.cull_stats(reset=True)
    cam = api.Camera(w, h, fx, fx if fy is None else fy)
    img = torch.zeros((len(trs), h, w, 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((len(trs), h, w, 4), dtype=torch.float32, device="cuda")
    for shard in shards:
        api.launch_renderer_batch(t, cam, trs, api.RenderOptions(**opt_kw), list(img), None, True, accums=list(acc),
                                  shard=shard, fp_mode=fp_mode)
    torch.cuda.synchronize()
    assert t.status() == 0
    return img.cpu().numpy(), acc.cpu().numpy(), t.cull_stats(reset=True)


def oracle(tree, trs, w, h, fx, fp_mode=0, fy=None, ndc=None, **opt_kw):
    """-> (rgba [n, h, w, 4], accum [n, h, w, 4], blocks without a hit summed over the frames)."""
    th, opt = ob.TreeHandle(tree, ndc=ndc), ob.default_options(**opt_kw)
    rgba, acc, empty = [], [], 0
    for tr in trs:
        cam = ob.make_camera(tr, w, h, fx, fy)
        r, a, _ = ob.render(th, cam, opt, fp_mode)
        rgba.append(r)
        acc.append(a)
        empty += int((~cu.hit_blocks(ob.render_maps(th, cam, opt, fp_mode)[1])).sum())
    return np.stack(rgba), np.stack(acc), empty


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: RGBA8 differs"
    au.assert_same_bits(got[1], want[1], f"{what}: accumulators")


@FP
@TREE
@pytest.mark.parametrize("n", [1, 3])
def test_frames_equal_cull_off_and_the_oracle(torch_cuda, name, n, fp_mode):
    from volrend_amd import api
    tree, trs = scene(name), poses(n)
    want = oracle(tree, trs, SIZE, SIZE, SIZE * 1111.111 / 800.0, fp_mode)
    t = api.N3Tree.from_synth(tree)
    try:
        f = SIZE * 1111.111 / 800.0
        on = render(torch_cuda, t, trs, SIZE, SIZE, f, fp_mode, cull=1)
        off = render(torch_cuda, t, trs, SIZE, SIZE, f, fp_mode, cull=0)
    finally:
        t.free_device()
    same(on, off, "cull on / off")
    same(on, want, "cull on / oracle")
    blocks = n * (SIZE // 8) ** 2
    assert on[2]["blocks"] == blocks and 0 < on[2]["culled"] <= want[2], (on[2], want[2])
    assert off[2] == {"blocks": 0, "culled": 0}


@TREE
def test_tile_shards(torch_cuda, name):
    """Tiles of 16 x 8 dealt to two ranks: each rank's launch culls by the frame's mask, whatever its tiles."""
    from volrend_amd import api
    tree, trs, f = scene(name), poses(1), SIZE * 1111.111 / 800.0
    want = oracle(tree, trs, SIZE, SIZE, f)
    t = api.N3Tree.from_synth(tree)
    try:
        one = [api.TileShard(16, 8, 1, 2)]
        on1 = render(torch_cuda, t, trs, SIZE, SIZE, f, cull=1, shards=one)
        off1 = render(torch_cuda, t, trs, SIZE, SIZE, f, cull=0, shards=one)
        both = render(torch_cuda, t, trs, SIZE, SIZE, f, cull=1, shards=[api.TileShard(16, 8, r, 2) for r in (0, 1)])
    finally:
        t.free_device()
    same(on1, off1, "rank 1 of 2, cull on / off")
    assert on1[2]["blocks"] == (SIZE // 8) ** 2 // 2 and on1[2]["culled"] > 0
    same(both, want, "both ranks / oracle")
    assert both[2]["blocks"] == (SIZE // 8) ** 2 and 0 < both[2]["culled"] <= want[2]


@FP
@TREE
def test_aov_planes(torch_cuda, name, fp_mode):
    """vr_render_aov with the cull on (the default): depth and transmittance of every pixel against the
    restatement, colour equal to vr_render_batch's; and the AOV launch culls."""
    from volrend_amd import api
    tree, trs, f = scene(name), poses(3), SIZE * 1111.111 / 800.0
    au.check(torch_cuda, tree, trs, SIZE, SIZE, f, fp_mode)
    t = api.N3Tree.from_synth(tree)
    try:
        t.cull_stats(reset=True)
        r = au.render_both(torch_cuda, t, SIZE, SIZE, f, trs, fp_mode)
        stats = t.cull_stats()
        t.set_tuning(block_cull=0)
        r0 = au.render_both(torch_cuda, t, SIZE, SIZE, f, trs, fp_mode)
    finally:
        t.free_device()
    assert stats["blocks"] == 2 * 3 * (SIZE // 8) ** 2 and stats["culled"] > 0 and stats["culled"] % 2 == 0
    for k in ("img1", "acc1", "depth", "trans"):
        au.assert_same_bits(r[k], r0[k], f"{k}: cull on / off")


def test_asymmetric_geometry(torch_cuda):
    """Per-axis scale and offset, fx != fy, w != h."""
    from volrend_amd import api
    tree = common.asymmetric_scene("SH", 9, depth=6)
    tr, w, h, fx, fy = common.asymmetric_camera()
    want = oracle(tree, [tr], w, h, fx, fy=fy)
    t = api.N3Tree.from_synth(tree)
    try:
        on = render(torch_cuda, t, [tr], w, h, fx, fy=fy)
    finally:
        t.free_device()
    same(on, want, "asymmetric / oracle")
    assert on[2]["blocks"] == (w // 8) * (h // 8) and on[2]["culled"] <= want[2]


def test_cull_is_off_where_it_must_be(torch_cuda):
    from volrend_amd import api
    tree, f = scene("SH9"), SIZE * 1111.111 / 800.0
    trs = poses(1)
    t = api.N3Tree.from_synth(tree)
    try:
        # sigma_thresh < 0: empty space is a hit
        neg = render(torch_cuda, t, trs, SIZE, SIZE, f, sigma_thresh=-1.0)
        same(neg, oracle(tree, trs, SIZE, SIZE, f, sigma_thresh=-1.0), "sigma_thresh = -1")
        assert neg[2]["culled"] == 0
        # the camera inside the volume, in the middle of a listed cell
        g, grid = cu.occupancy(tree)
        scale, offset = np.asarray(tree.invradius3, np.float64), np.asarray(tree.offset, np.float64)
        to_world = lambda p: tuple(((np.asarray(p) - offset) / scale).astype(np.float32))
        tr, w, h, fi = common.camera_at(to_world((cu.boundary_cells(grid)[0] + 0.5) / (1 << g)),
                                        look_at=to_world((0.52, 0.47, 0.55)), size=SIZE, focal=60.0)
        inside = render(torch_cuda, t, [tr], w, h, fi)
        same(inside, oracle(tree, [tr], w, h, fi), "camera inside")
        assert inside[2] == {"blocks": (SIZE // 8) ** 2, "culled": 0}
    finally:
        t.free_device()
    # an NDC tree
    tree, tr, w, h, fx, fy, ndc = common.asymmetric_ndc_case()
    t = api.N3Tree.from_synth(tree, ndc=ndc)
    try:
        got = render(torch_cuda, t, [tr], w, h, fx, fy=fy)
    finally:
        t.free_device()
    same(got, oracle(tree, [tr], w, h, fx, fy=fy, ndc=ndc), "NDC")
    assert got[2]["culled"] == 0


def octant_pair(name):
    """The scene with its density kept in the octant below (0.5, 0.5, 0.5) only, and in the octant above it only."""
    tree = scene(name)
    corners, sizes, _, slots = qu.leaf_boxes(tree)
    centre = corners + 0.5 * sizes[:, None]
    out = []
    for keep in ((centre < 0.5).all(1), (centre > 0.5).all(1)):
        data = tree.data.copy()
        data.reshape(-1, tree.data_dim)[slots[~keep], -1] = 0
        out.append(dataclasses.replace(tree, data=data))
    return out


@pytest.mark.parametrize("how", ["update_data", "tree_step"])
def test_occupancy_follows_the_values(torch_cuda, how):
    torch = torch_cuda
    from volrend_amd import api
    low, high = octant_pair("SH16")
    trs, f = poses(3), SIZE * 1111.111 / 800.0
    want_low, want_high = oracle(low, trs, SIZE, SIZE, f), oracle(high, trs, SIZE, SIZE, f)
    assert not np.array_equal(want_low[0], want_high[0]) and want_low[1][..., 3].any() and want_high[1][..., 3].any()
    t = api.N3Tree.from_synth(low)
    try:
        first = render(torch, t, trs, SIZE, SIZE, f)
        same(first, want_low, "before the update")
        if how == "update_data":
            t.update_data(torch.from_numpy(high.data).cuda())
        else:  # a step over every slot with a zero gradient: the tree takes float16(master)
            master = torch.from_numpy(high.data.astype(np.float32)).cuda()
            grad = torch.zeros_like(master)
            n_slots = low.capacity * 8
            touched = torch.full(((n_slots + 31) // 32,), -1, dtype=torch.int32, device="cuda")
            t.step(master, grad, touched, kind="sgd", lr=1.0)
        after = render(torch, t, trs, SIZE, SIZE, f)
    finally:
        t.free_device()
    same(after, want_high, f"after {how}")
    assert 0 < first[2]["culled"] <= want_low[2] and 0 < after[2]["culled"] <= want_high[2]
