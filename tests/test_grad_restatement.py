"""The yardstick of the vr_render_backward tests (tests/cpp/grad_restatement.c, tests/grad_util.py), tied down
without a GPU: its forward is the oracle's function, its formulas are that forward's derivative, and the
binary32 evaluation of them gives the summation constant the GPU tolerance is made of."""
import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import grad_util as gu

FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])

# ---- 1. same function as the oracle -------------------------------------------------------------------
# |float64 out - oracle accumulator| / (the pixel's sum of w_i): the largest value over all cases below was
# measured at 4.55e-6 (sh16, default / no_early_stop, fma: 76 units of 2^-24 -- the oracle adds hundreds of
# binary32 terms per ray).  The bound is four times that.
ORACLE_MEASURED = 4.55e-6
ORACLE_BOUND = 4 * ORACLE_MEASURED


def _tie_scene(name):
    if name in ("sh16", "sh9_near", "n4"):
        return au.scene(name)
    return (gu.tree_of(name)[0],) + common.camera_for(size=64)


@FP
@pytest.mark.parametrize("optset", list(au.OPTION_SETS))
@pytest.mark.parametrize("name", ["sh16", "sh9_near", "n4", "rgba", "sh4"])
def test_forward_is_the_oracles_function(name, optset, fp_mode):
    tree, tr, w, h, f = _tie_scene(name)
    kw = au.OPTION_SETS[optset]
    _, acc, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode, **kw)
    t = gu.Trace(tree, tr, w, h, f, fp_mode, **kw)
    out, wsum = t.forward64(gu.data64_of(tree))
    dev = np.abs(out - acc.astype(np.float64))
    hit = wsum > 0
    assert hit.sum() > 1000
    assert (dev[~hit] == 0).all(), "a pixel without a hit sample differs"
    worst = float((dev[hit] / wsum[hit][:, None]).max())
    print(f"{name} {optset} fp{fp_mode}: worst deviation / sum w = {worst:.3e}")
    assert worst <= ORACLE_BOUND
    # the stop flag: alpha is 1 exactly where the restatement says the ray was stopped
    stopped = t.stopped.reshape(h, w)
    assert ((acc[..., 3] == 1.0) | ~stopped).all() and (stopped.any() or optset == "no_early_stop")


# ---- 2. the formulas are the derivative ----------------------------------------------------------------
def _frame(name, gkind, seed):
    tree = gu.tree_of(name)[0]
    trs, w, h, f = gu.views(name, 24, 1)
    t = gu.Trace(tree, trs[0], w, h, f, 0)
    g = gu.upstream(gkind, 1, h, w, seed=seed)[0].astype(np.float64)
    d64 = gu.data64_of(tree)
    grad, mag, _ = t.backward64(d64, g)
    return tree, t, g, d64, grad, mag


def _central_difference(t, g, d64, idx):
    v = d64[idx]
    h = 1e-5 * max(abs(v), 1.0)
    d64[idx] = v + h
    up = t.forward64(d64)[0]
    d64[idx] = v - h
    dn = t.forward64(d64)[0]
    d64[idx] = v
    return float(((up - dn) * g).sum() / (2 * h))   # (pixel by pixel: a pixel the element does not reach adds an exact 0)


def _sigma_slots_by_stop(t):
    """Slots only stopped rays touch, and slots only unstopped rays touch."""
    by_stopped, by_open = set(), set()
    for r in np.nonzero(t.n_hits)[0]:
        (by_stopped if t.stopped[r] else by_open).update(t.slots(r).tolist())
    return sorted(by_stopped - by_open), sorted(by_open - by_stopped)


def _draw(rng, candidates, what):
    assert len(candidates) > 0, f"no candidate for {what}"
    return candidates[int(rng.integers(len(candidates)))]


@pytest.mark.parametrize("name,gkind", [("sh16", "normal"), ("rgba", "normal"), ("n4", "normal"), ("sh16", "alpha")])
def test_formulas_are_the_derivative(name, gkind):
    tree, t, g, d64, grad, mag = _frame(name, gkind, seed=21)
    rng = np.random.default_rng(99)
    dd, bd = tree.data_dim, tree.basis_dim
    flat_mag = mag.reshape(-1, dd)
    picks = []
    only_stopped, only_open = _sigma_slots_by_stop(t)
    for slots, what in ((only_stopped, "sigma, stopped rays only"), (only_open, "sigma, unstopped rays only")):
        cand = [s for s in slots if flat_mag[s, dd - 1] > 0]
        if gkind == "alpha" and what.startswith("sigma, stopped"):
            assert not cand, "g = (0, 0, 0, 1) reaches no sigma through a stopped ray"
            continue
        picks.append((_draw(rng, cand, what), dd - 1, what))
    if gkind != "alpha":
        touched = np.nonzero(flat_mag[:, 0] > 0)[0]
        if bd > 0:
            groups = [g_ for g_ in ((0, 0), (1, 3), (4, 8), (9, 15)) if g_[1] < bd]
            for lo, hi in groups:
                ch, b = int(rng.integers(3)), int(rng.integers(lo, hi + 1))
                picks.append((_draw(rng, touched.tolist(), f"b {lo}-{hi}"), ch * bd + b, f"coefficient b={b}"))
        else:
            picks.append((_draw(rng, touched.tolist(), "rgba"), int(rng.integers(3)), "RGBA colour entry"))
    assert len(picks) >= (1 if gkind == "alpha" else 3)
    for slot, e, what in picks:
        idx = np.unravel_index(slot * dd + e, d64.shape)
        cd = _central_difference(t, g, d64, idx)
        err, m = abs(cd - grad[idx]), mag[idx]
        print(f"{name} {gkind} {what}: grad {grad[idx]:.6e} central difference {cd:.6e} |diff| / M = {err / m:.2e}")
        assert m > 0 and err <= 1e-6 * m, (what, grad[idx], cd, m)
    if gkind == "alpha":   # colour entries get nothing at all
        cols = np.ones(dd, bool)
        cols[dd - 1] = False
        assert (mag.reshape(-1, dd)[:, cols] == 0).all() and (grad.reshape(-1, dd)[:, cols] == 0).all()


# ---- 3. the summation constant -------------------------------------------------------------------------
def test_summation_constant():
    """The binary32 entry point, rays in scanline order and in a seeded shuffled order, against float64 over
    the cases of the GPU parity test: the largest |diff| / unit is K32 (tests/grad_util.py), measured 36.70."""
    worst = 0.0
    for name, size, n, optset, gkind in gu.PARITY_CASES:
        for fp_mode in (0, 1):
            ref = gu.reference(name, optset, fp_mode, n, size, gkind)
            d32 = np.ascontiguousarray(ref["tree"].data, np.float16).astype(np.float32)
            n_rays = ref["w"] * ref["h"]
            rng = np.random.default_rng(5)
            for shuffled in (False, True):
                got = np.zeros(d32.shape, np.float32)
                for i, t in enumerate(ref["traces"]):
                    t.backward32(d32, ref["g"][i], rng.permutation(n_rays) if shuffled else np.arange(n_rays), got)
                ratio, zeros_same = gu.worst_ratio(got, ref)
                assert zeros_same
                worst = max(worst, ratio)
    print(f"k32 measured: {worst:.3f}")
    assert worst <= gu.K32 and gu.K32 - worst < 1.0, worst
    assert gu.K == 4 * gu.K32
