"""The yardstick of the vr_render_aov tests is tied to the oracle (no GPU needed).

tests/cpp/march_restatement.h restates trace_ray's loop without the colour -- the one restatement, which
the leaf-weight and backward yardsticks march with too -- and tests/cpp/aov_restatement.c returns, per pixel,
the depth sum D, the final transmittance T, delta_scale and "ended by stop_thresh".  The oracle
shows both only in disguise, and this test compares those disguises on EVERY pixel, bit for bit
(NaN == NaN):
  depth mode  accum[0] == fl(min(fl(D * 0.3f), 1)), times fl(1 / (1 - T)) where the ray was stopped;
  colour mode accum[3] == 1 where stopped, else fl(1 - T).
This validates the yardstick, not the feature."""
import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests.common import ob


def tie(tree, tr, w, h, f, fp_mode, ndc=None, offscreen=True, depth_init=None, fy=None, **kw):
    D, T, ds, stop = au.restate(tree, tr, w, h, f, fp_mode, ndc=ndc, offscreen=offscreen, depth_init=depth_init,
                                fy=fy, **kw)
    init = np.zeros((h, w, 4), np.uint8) if not offscreen else None
    _, acc_d, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode, ndc=ndc, offscreen=offscreen, rgba_init=init,
                                      depth_init=depth_init, fy=fy, render_depth=1, **kw)
    _, acc_c, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode, ndc=ndc, offscreen=offscreen, rgba_init=init,
                                      depth_init=depth_init, fy=fy, **kw)
    one = np.float32(1)
    with np.errstate(all="ignore"):
        v = np.fmin((D * np.float32(0.3)).astype(np.float32), one)   # the oracle's vr_minf: min(NaN, 1) = 1
        scale = (one / (one - T)).astype(np.float32)
        want_d = np.where(stop, (v * scale).astype(np.float32), v)
        want_a = np.where(stop, one, (one - T).astype(np.float32))
    return D, T, stop, acc_d[..., 0], want_d, acc_c[..., 3], want_a


def check(tree, tr, w, h, f, fp_mode, **kw):
    D, T, stop, got_d, want_d, got_a, want_a = tie(tree, tr, w, h, f, fp_mode, **kw)
    au.assert_same_bits(got_d, want_d, "depth-mode accum[0]")
    au.assert_same_bits(got_a, want_a, "colour-mode accum[3]")
    return D, T, stop


@pytest.mark.parametrize("fp_mode", [ob.FP_STRICT, ob.FP_FMA], ids=["strict", "fma"])
@pytest.mark.parametrize("scene,optset", au.TIE_CASES, ids=[f"{s}-{o}" for s, o in au.TIE_CASES])
def test_restatement_equals_the_oracle_on_every_pixel(scene, optset, fp_mode):
    tree, tr, w, h, f = au.scene(scene)
    D, T, stop = check(tree, tr, w, h, f, fp_mode, **au.OPTION_SETS[optset])
    assert (D != 0).any(), "the case shows nothing: no pixel has a hit"
    if optset == "no_early_stop":
        assert not stop.any()


@pytest.mark.parametrize("fp_mode", [ob.FP_STRICT, ob.FP_FMA], ids=["strict", "fma"])
def test_restatement_with_a_mesh_depth_plane(fp_mode):
    """offscreen = 0 and a depth_init plane: tmax comes from the mesh; some rays end in front of the box."""
    tree = common.small_scene(depth=5, basis_dim=9, seed=71)
    tr, w, h, f = common.camera_for(pose_idx=4, size=64)
    depth = np.random.default_rng(5).uniform(2.0, 6.0, size=(h, w)).astype(np.float32)
    D, T, stop = check(tree, tr, w, h, f, fp_mode, offscreen=False, depth_init=depth)
    D0, _, _, _ = au.restate(tree, tr, w, h, f, fp_mode)
    assert (D != 0).any() and not np.array_equal(D, D0), "the mesh depth must cut some rays short"


@pytest.mark.parametrize("fp_mode", [ob.FP_STRICT, ob.FP_FMA], ids=["strict", "fma"])
def test_restatement_on_an_ndc_tree(fp_mode):
    tree = common.small_scene(depth=5, basis_dim=4, seed=51)
    D, T, stop = check(tree, au.NDC_TRANSFORM, 96, 72, 80.0, fp_mode, ndc=au.NDC)
    assert (D != 0).any()


@pytest.mark.parametrize("fp_mode", [ob.FP_STRICT, ob.FP_FMA], ids=["strict", "fma"])
def test_restatement_under_asymmetric_geometry(fp_mode):
    """Scale and offset that differ per axis, fx != fy: delta_scale is a different number for every ray."""
    tr, w, h, fx, fy = common.asymmetric_camera()
    D, T, stop = check(common.asymmetric_scene(), tr, w, h, fx, fp_mode, fy=fy)
    assert (D != 0).mean() >= 0.2 and stop.any()
    init_depth = common.mesh_underlay(w, h)[1]
    Dm, _, _ = check(common.asymmetric_scene(), tr, w, h, fx, fp_mode, fy=fy, offscreen=False, depth_init=init_depth)
    assert not np.array_equal(Dm, D), "the mesh depth must cut some rays short"


@pytest.mark.parametrize("fp_mode", [ob.FP_STRICT, ob.FP_FMA], ids=["strict", "fma"])
def test_restatement_on_the_asymmetric_ndc_tree(fp_mode):
    tree, tr, w, h, fx, fy, ndc = common.asymmetric_ndc_case()
    D, T, stop = check(tree, tr, w, h, fx, fp_mode, fy=fy, ndc=ndc)
    assert (D != 0).mean() >= 0.2
