"""The yardstick of the ray-list tests is tied to the oracle (no GPU needed).

tests/rays_util.oracle_rays sends one ray through the oracle as pixel (1, 1) of a 2 x 2 camera whose matrix
product yields the ray's direction exactly; tests/rays_util.rays_of_camera forms a camera's rays in numpy.
Here the two are pinned against whole frames of the oracle, accumulators and RGBA8 bit for bit:
  strict model  any pose (the numpy product rounds as the strict product does);
  FMA model     signed-permutation poses, whose product is exact fused or not.
This validates the yardstick, not the feature."""
import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import grad_util as gu
from tests import rays_util as ru
from tests.common import ob

FP = pytest.mark.parametrize("fp_mode", [ob.FP_STRICT, ob.FP_FMA], ids=["strict", "fma"])


def tie(tree, tr, w, h, fx, fp_mode, fy=None, ndc=None, shows=None, **kw):
    """Every pixel of the frame equals its ray through oracle_rays -> the frame's counters."""
    rgba, accum, cnt = common.oracle_frame(tree, tr, w, h, fx, fp_mode, ndc=ndc, fy=fy, **kw)
    o, d = ru.rays_of_camera(tr, w, h, fx, fy)
    r_rgba, r_accum, hit = ru.oracle_rays(tree, o, d, fp_mode, ndc=ndc, **kw)
    bad = (r_accum.view(np.uint32) != accum.reshape(-1, 4).view(np.uint32)).any(1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} accumulators differ"
    assert np.array_equal(r_rgba, rgba.reshape(-1, 4))
    assert hit == cnt["rays_hit_box"] and cnt["rays"] == w * h
    assert (accum[..., 3] > 0).sum() > (w * h // 10 if shows is None else shows), "the case shows nothing"
    return cnt


def test_general_pose_strict_sh16():
    tree = gu.tree_of("sh16")[0]
    tr, _, _, f = common.camera_for(size=33)
    tie(tree, tr, 33, 33, f, ob.FP_STRICT)


def test_asymmetric_scene_strict():
    tree = common.asymmetric_scene("SH", 9)
    tr, _, _, fx, fy = common.asymmetric_camera()
    tie(tree, tr, 21, 21, fx * 21 / 64, ob.FP_STRICT, fy=fy * 21 / 48, rot_dirs=(0.3, -0.2, 0.9))


@FP
def test_permutation_pose_both_models(fp_mode):
    tree = gu.tree_of("sh16")[0]
    tie(tree, ru.permutation_pose(), 35, 27, 30.0, fp_mode)


@FP
def test_ndc_tree(fp_mode):
    """(the NDC pose of the other tests is the identity rotation: a signed permutation)"""
    tree, _, ndc = gu.tree_of("ndc")
    tie(tree, au.NDC_TRANSFORM, 47, 35, 40.0, fp_mode, ndc=ndc)


def test_short_focal_some_rays_miss_the_box():
    tree = gu.tree_of("sh4")[0]
    tr, _, _, _ = common.camera_for(size=25)
    cnt = tie(tree, tr, 25, 25, 9.0, ob.FP_STRICT, shows=40)   # (a view this wide sees the volume in few pixels)
    assert 0 < cnt["rays_hit_box"] < cnt["rays"]


@FP
def test_origins_inside_the_volume(fp_mode):
    tree = gu.tree_of("sh9_near")[0]
    lo, hi = ru.world_box(tree)
    centre = lo + (hi - lo) * np.array([0.45, 0.55, 0.4])
    if fp_mode == ob.FP_STRICT:
        tr = common.camera_at(centre, look_at=lo + (hi - lo) * 0.7, size=23, focal=12.0)[0]
    else:
        tr = ru.permutation_pose(centre=centre)
    cnt = tie(tree, tr, 23, 23, 12.0, fp_mode)
    assert cnt["rays_hit_box"] == cnt["rays"]


def test_helpers():
    o, d = ru.arbitrary_rays(gu.tree_of("sh16")[0], 600, seed=1)
    assert o.shape == d.shape == (600, 3) and o.dtype == d.dtype == np.float32
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    assert ln.min() < 0.05 and ln.max() > 20 and 0.0099 < ln.min() and ln.max() < 101
    tr = ru.permutation_pose()
    m = tr[:9].reshape(3, 3)
    assert np.array_equal(np.abs(m).sum(0), np.ones(3)) and np.array_equal(np.abs(m).sum(1), np.ones(3))
