"""The yardstick of the vr_accumulate_weights tests is tied to the oracle (no GPU needed).

tests/cpp/weights_restatement.c applies the per-leaf rule (hits += 1; max over the weights > 0) to the hit
samples of the one restatement of trace_ray's loop (tests/cpp/march_restatement.h).  The oracle has no per-leaf
output, so the tie goes through what it does have, bit for bit in both FP models:
  per pixel  D, T and "ended by stop_thresh" equal tests/aov_util.restate (itself tied to or_render on every
             pixel by tests/test_aov_restatement.py; the same C loop, here with the callback: this half pins the
             callback path and the Python plumbing);
  per frame  hits.sum() equals the oracle's counters.hit_samples: every hit sample was counted in some slot.
This validates the yardstick, not the feature."""
import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import weights_util as wu
from tests.common import ob

FP = pytest.mark.parametrize("fp_mode", [ob.FP_STRICT, ob.FP_FMA], ids=["strict", "fma"])


def tie(tree, tr, w, h, f, fp_mode, ndc=None, fy=None, **kw):
    r = wu.restate_frame(tree, tr, w, h, f, fp_mode, ndc=ndc, fy=fy, **kw)
    D, T, _, stop = au.restate(tree, tr, w, h, f, fp_mode, ndc=ndc, fy=fy, **kw)
    au.assert_same_bits(r["D"], D, "D")
    au.assert_same_bits(r["T"], T, "T")
    assert np.array_equal(r["stop"], stop)
    counters = common.oracle_frame(tree, tr, w, h, f, fp_mode, ndc=ndc, fy=fy, **kw)[2]
    assert int(r["hits"].sum(dtype=np.uint64)) == counters["hit_samples"]
    # the rule itself, on what the restatement returned
    assert not np.isnan(r["max_weight"]).any() and (r["max_weight"] >= 0).all()
    assert not (r["max_weight"][r["hits"] == 0] != 0).any(), "a maximum without a hit"
    return r


@FP
@pytest.mark.parametrize("scene,optset", wu.TIE_CASES, ids=[f"{s}-{o}" for s, o in wu.TIE_CASES])
def test_restatement_is_tied_to_the_oracle(scene, optset, fp_mode):
    tree, tr, w, h, f = wu.scene(scene)
    r = tie(tree, tr, w, h, f, fp_mode, **wu.OPTION_SETS[optset])
    assert (r["max_weight"] > 0).any(), "the case shows nothing: no leaf has a positive weight"
    if optset == "no_early_stop":
        assert not r["stop"].any()


@FP
def test_later_frames_raise_maxima(fp_mode):
    """Frames accumulate: after three poses some leaf holds a maximum the first pose did not give it, and
    frame-by-frame accumulation equals the element-wise max / sum of the frames taken alone."""
    tree, _, w, h, f = wu.scene("sh16")
    trs = wu.poses(3, size=w)
    first = wu.restate_frame(tree, trs[0], w, h, f, fp_mode)
    mw, hc, _ = wu.restate(tree, trs, w, h, f, fp_mode)
    assert (mw > first["max_weight"]).any(), "no leaf's maximum comes from a later frame"
    alone = [wu.restate_frame(tree, tr, w, h, f, fp_mode) for tr in trs]
    assert np.array_equal(wu.bits(mw), wu.bits(np.maximum.reduce([a["max_weight"] for a in alone])))
    assert np.array_equal(hc, np.add.reduce([a["hits"] for a in alone]))


@FP
def test_negative_threshold_gives_weights_that_only_count(fp_mode):
    """sigma_thresh = -1 on the value-edge tree: negative densities become hits, their weights are <= 0 (or
    NaN once light_intensity has met an infinity) and must count in hits without touching the maximum."""
    tree, tr, w, h, f = wu.scene("value_edge")
    r = tie(tree, tr, w, h, f, fp_mode, **wu.NEGATIVE)
    assert r["nonpositive"] > 0, "the case shows nothing: no hit sample has a weight <= 0 or NaN"
    assert (r["max_weight"] > 0).any()
    assert ((r["hits"] > 0) & (r["max_weight"] == 0)).any(), "no slot was hit by non-positive weights alone"


@FP
def test_restatement_on_an_ndc_tree(fp_mode):
    tree = common.small_scene(depth=5, basis_dim=4, seed=51)
    r = tie(tree, au.NDC_TRANSFORM, 96, 72, 80.0, fp_mode, ndc=au.NDC)
    assert (r["max_weight"] > 0).any()


@FP
def test_restatement_under_asymmetric_geometry(fp_mode):
    """Scale and offset that differ per axis, fx != fy: delta_scale is a different number for every ray."""
    tr, w, h, fx, fy = common.asymmetric_camera()
    r = tie(common.asymmetric_scene(), tr, w, h, fx, fp_mode, fy=fy)
    assert (r["max_weight"] > 0).sum() > 500 and r["stop"].any()


@FP
def test_restatement_on_the_asymmetric_ndc_tree(fp_mode):
    tree, tr, w, h, fx, fy, ndc = common.asymmetric_ndc_case()
    r = tie(tree, tr, w, h, fx, fp_mode, fy=fy, ndc=ndc)
    assert (r["max_weight"] > 0).sum() > 500
