"""The block cull's rule against the oracle, without a GPU: no 8x8 pixel block that the numpy restatement
(tests/cull_util.py) leaves unmarked holds a pixel with a hit sample in the oracle's per-pixel hit map, over
cube and asymmetric geometry, cameras far from, just outside and inside the volume; and the rule does cull."""
import numpy as np
import pytest

from tests import common
from tests import cull_util as cu
from tests.common import ob

SIZE = 96


def hit_map(tree, tr, w, h, fx, fy=None, **opt_kw):
    _, hits, cnt = ob.render_maps(ob.TreeHandle(tree), ob.make_camera(tr, w, h, fx, fy), ob.default_options(**opt_kw))
    return hits, cnt


def world_point(tree, p):
    return ((np.asarray(p, np.float64) - np.asarray(tree.offset, np.float64)) /
            np.asarray(tree.invradius3, np.float64)).astype(np.float32)


def check(tree, tr, w, h, fx, fy=None, **opt_kw):
    """-> (culled share of the blocks, share of the blocks without a hit)."""
    hits, cnt = hit_map(tree, tr, w, h, fx, fy, **opt_kw)
    marked = cu.block_mask(tree, tr, w, h, fx, fy)
    occupied = cu.hit_blocks(hits)
    assert marked.shape == occupied.shape
    wrong = np.argwhere(occupied & ~marked)
    assert len(wrong) == 0, f"{len(wrong)} culled blocks hold a hit, first (by, bx) = {wrong[0]}"
    return float((~marked).mean()), float((~occupied).mean())


@pytest.mark.parametrize("depth,basis_dim,seed", [(5, 16, 11), (6, 9, 41), (6, 16, 3)])
def test_orbit_poses_cull_only_empty_blocks(depth, basis_dim, seed):
    tree = common.small_scene(depth=depth, basis_dim=basis_dim, seed=seed)
    shares = []
    for pose in (0, 2, 5, 7):
        tr, w, h, f = common.camera_for(pose_idx=pose, size=SIZE)
        culled, empty = check(tree, tr, w, h, f)
        assert culled <= empty
        shares.append(culled)
    assert max(shares) > 0, "the rule culls nothing on any pose of the orbit"


def test_asymmetric_scale_offset_and_focal_lengths():
    tree = common.asymmetric_scene("SH", 9, depth=6)
    tr, _, _, f = common.camera_for(pose_idx=2, size=SIZE)
    culled = [check(tree, tr, SIZE, SIZE, 1.2 * f, 0.7 * f)[0]]
    tr, w, h, fx, fy = common.asymmetric_camera()  # 64 x 48
    culled.append(check(tree, tr, w, h, fx, fy)[0])
    assert max(culled) > 0


def test_thresholds_and_bbox_inside_the_cube_only_remove_hits():
    tree = common.small_scene(depth=6, basis_dim=9, seed=41)
    tr, w, h, f = common.camera_for(pose_idx=3, size=SIZE)
    check(tree, tr, w, h, f, sigma_thresh=0.0)
    check(tree, tr, w, h, f, sigma_thresh=0.5, stop_thresh=0.1)
    check(tree, tr, w, h, f, render_bbox=(0.1, 0.2, 0.0, 0.8, 0.9, 0.7))


@pytest.mark.parametrize("where", [(1.06, 0.5, 0.5), (0.5, -0.08, 0.45), (1.02, 1.03, 1.04)])
def test_camera_just_outside_the_volume(where):
    tree = common.small_scene(depth=6, basis_dim=16, seed=3)
    tr, w, h, f = common.camera_at(world_point(tree, where), look_at=tuple(world_point(tree, (0.5, 0.5, 0.5))),
                                   size=SIZE, focal=60.0)
    check(tree, tr, w, h, f)


def test_camera_inside_the_volume_marks_the_whole_frame():
    tree = common.small_scene(depth=5, basis_dim=16, seed=11)
    g, grid = cu.occupancy(tree)
    cell = cu.boundary_cells(grid)[0]  # the camera sits in the middle of a listed cell
    pos = world_point(tree, (cell + 0.5) / (1 << g))
    tr, w, h, f = common.camera_at(pos, look_at=tuple(world_point(tree, (0.52, 0.47, 0.55))), size=SIZE, focal=60.0)
    assert cu.block_mask(tree, tr, w, h, f).all()
    check(tree, tr, w, h, f)


def test_non_orthonormal_pose_marks_the_whole_frame():
    tree = common.small_scene(depth=5, basis_dim=16, seed=11)
    tr, w, h, f = common.camera_for(pose_idx=2, size=SIZE)
    assert cu.block_mask(tree, common.non_orthonormal(tr), w, h, f).all()


def test_occupancy_counts_sigma_as_a_float():
    """NaN, -0 and negative sigma set no cell; the smallest subnormal does."""
    tree = common.small_scene(depth=5, basis_dim=4, seed=11)
    data = tree.data.copy()
    sig = data.reshape(-1, tree.data_dim)[:, -1].view(np.uint16)
    sig[:] = np.resize(np.array([0x8000, 0xB800, 0x7E00, 0xFC00, 0x0000], np.uint16), sig.shape)
    import dataclasses
    assert not cu.occupancy(dataclasses.replace(tree, data=data))[1].any()
    sig[:] = 0x0001
    assert cu.occupancy(dataclasses.replace(tree, data=data))[1].all()
