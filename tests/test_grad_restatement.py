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


def test_summation_constant_of_the_scheduling_cases():
    """test_summation_constant over the cases of tests/test_gpu_sched.py (tests/grad_util.py SCHED_CASES: 8 poses
    per element instead of at most 2): the largest |diff| / unit is 13.855, below K32 -- those cases are judged
    with K as it stands."""
    worst = 0.0
    for name, size, n, optset, gkind, fp_modes in gu.SCHED_CASES:
        for fp_mode in fp_modes:
            ref = gu.reference(name, optset, fp_mode, n, size, gkind)
            assert (ref["mag"] > 0).sum() > 200, "the case shows nothing"
            d32 = np.ascontiguousarray(ref["tree"].data, np.float16).astype(np.float32)
            n_rays = ref["w"] * ref["h"]
            rng = np.random.default_rng(5)
            for shuffled in (False, True):
                got = np.zeros(d32.shape, np.float32)
                for i, t in enumerate(ref["traces"]):
                    t.backward32(d32, ref["g"][i], rng.permutation(n_rays) if shuffled else np.arange(n_rays), got)
                ratio, zeros_same = gu.worst_ratio(got, ref)
                print(f"{name} {optset} {gkind} fp{fp_mode} shuffled={shuffled}: {ratio:.3f}")
                assert zeros_same
                worst = max(worst, ratio)
    print(f"k32 of the scheduling cases measured: {worst:.3f}")
    assert worst <= gu.K32, worst
    assert abs(worst - gu.SCHED_K32_MEASURED) < 0.01, worst


# ---- 4. the value domain: the edge-aware unit ------------------------------------------------------------------
CATALOGUES = ("finite", "full")
EDGE = pytest.mark.parametrize("name,fp_mode", gu.EDGE_RUNS, ids=gu.EDGE_IDS)


def _eval32(ref, shuffled, mutant=0):
    d32 = np.ascontiguousarray(ref["tree"].data, np.float16).astype(np.float32)
    n_rays = ref["w"] * ref["h"]
    order = np.random.default_rng(5).permutation(n_rays) if shuffled else np.arange(n_rays)
    got = np.zeros(d32.shape, np.float32)
    return ref["traces"][0].backward32(d32, ref["g"][0], order, got, mutant=mutant)


def test_edge_summation_constant():
    """test_summation_constant over the edge cases (tests/grad_util.py EDGE_CASES), both catalogues, against
    unit_edge and over the clean elements only: the largest |diff| / unit_edge is K32_EDGE, measured 28.996."""
    worst = 0.0
    for name, fp_mode in gu.EDGE_RUNS:
        for catalogue in CATALOGUES:
            ref = gu.edge_reference(name, catalogue, fp_mode)
            for shuffled in (False, True):
                ratio, n, zeros_same = gu.worst_edge_ratio(_eval32(ref, shuffled), ref)
                print(f"{name} fp{fp_mode} {catalogue} shuffled={shuffled}: {ratio:.3f} over {n} elements")
                assert zeros_same, (name, catalogue)
                worst = max(worst, ratio)
    print(f"k32_edge measured: {worst:.3f}")
    assert worst <= gu.K32_EDGE and gu.K32_EDGE - worst < 1.0, worst
    assert gu.K_EDGE == 4 * gu.K32_EDGE


@pytest.mark.parametrize("catalogue", CATALOGUES)
@EDGE
def test_edge_cap(name, fp_mode, catalogue):
    """Every edge case shows something: the slots a dirty ray touches are at most a third of the hit slots, at
    least 200 clean elements have M > 0, the clean slots hold special values, and the full catalogue has dirty
    slots at all."""
    ref = gu.edge_reference(name, catalogue, fp_mode)
    tree = ref["tree"]
    n_hit, n_dirty = int(ref["hit"].sum()), int(ref["dirty"].sum())
    n_pos = int((gu.clean_elements(ref) & (np.nan_to_num(ref["mag"], nan=0.0) > 0)).sum())
    print(f"{name} fp{fp_mode} {catalogue}: {n_dirty} of {n_hit} hit slots dirty ({n_dirty / n_hit:.3f}), "
          f"{ref['dirty_rays']} dirty rays, {n_pos} clean elements with M > 0")
    assert 3 * n_dirty <= n_hit
    assert n_pos >= 200
    rec = np.asarray(tree.data, np.float32).reshape(-1, tree.data_dim)[ref["clean"]]
    assert np.isfinite(rec).all(), "a clean slot holds a non-finite value"
    colours = rec[:, :-1]
    assert ((colours < 0) | (colours > 1)).any() if tree.format_name == "RGBA" else (np.abs(colours) >= 40).any()
    clean = gu.clean_elements(ref)
    assert np.isfinite(ref["grad"][clean]).all() and np.isfinite(gu.unit_edge(ref)[clean]).all()
    if catalogue == "full":
        assert n_dirty > 0 and ref["dirty_rays"] > 0
        assert not np.isfinite(ref["g"]).all()


@pytest.mark.parametrize("mutant", [1, 2, 3])
def test_the_edge_unit_sees_a_mutant(mutant):
    """grad_eval32 built with one deliberate mistake (tests/cpp/grad_restatement.c GRAD_MUTANT) exceeds K_EDGE on
    the clean elements of at least one edge case: the unit is not so loose that the mistake passes."""
    seen = []
    for name, fp_mode in gu.EDGE_RUNS:
        if fp_mode != 0:
            continue
        ref = gu.edge_reference(name, "finite", 0)
        ratio, _, _ = gu.worst_edge_ratio(_eval32(ref, False, mutant), ref)
        if ratio > gu.K_EDGE:
            seen.append(name)
        print(f"mutant {mutant} {name}: worst |diff| / unit_edge = {ratio:.3g} of {gu.K_EDGE}")
    print(f"mutant {mutant} exceeds K_EDGE on: {seen}")
    assert seen, f"no edge case sees mutant {mutant}"
    # the unmutated build on the same case stays within K32_EDGE
    ref = gu.edge_reference(seen[0], "finite", 0)
    assert gu.worst_edge_ratio(_eval32(ref, False), ref)[0] <= gu.K32_EDGE


def _fourth_order_difference(t, g, d64, idx, h):
    v = d64[idx]
    f = []
    for k in (-2, -1, 1, 2):
        d64[idx] = v + k * h
        f.append(t.forward64(d64)[0])
    d64[idx] = v
    return float(((f[0] - 8 * f[1] + 8 * f[2] - f[3]) * g).sum() / (12 * h))


@pytest.mark.parametrize("sign", [1, -1], ids=["u+20", "u-20"])
def test_formulas_are_the_derivative_at_a_saturated_colour(sign):
    """One record of the SH16 scene with |u| ~ 20 in one channel (coefficient 0 at +-70.9: c (1 - c) = 2e-9).
    grad_accum = (1, 1, 1, 0), so the contributions of the rays that cross the leaf -- one camera, nearly one
    direction -- do not cancel and the bound can be relative to the gradient itself: 1e-4 |grad| + 2e-13.  The
    fourth-order difference with h = 0.2 has a truncation error of (h B)^4 / 30 <= 5.3e-5 relative (|B_b| <= 1,
    the derivatives of a saturated sigmoid are all of its own size).  Its rounding error is absolute: the four
    frames enter with weights 1 + 8 + 8 + 1 over 12 h = 7.5, each pixel's colour is a sum of some 20 terms of size
    <= 1 (20 * 2^-53 each) and about ten pixels see the leaf: 7.5 * 20 * 1.1e-16 * 10 = 1.7e-13, against
    gradients of 1e-9 for the basis functions whose value is not small.  (c (1 - c) itself is 2e-9 of the
    unsaturated 0.25: a formula without the (1 - c), or with a flushed exp, is wrong by a factor.)"""
    tree = gu.tree_of("sh16")[0]
    trs, w, h, f = gu.views("sh16", 24, 1)
    t = gu.Trace(tree, trs[0], w, h, f, 0)
    g = gu.upstream("colour", 1, h, w)[0].astype(np.float64)
    d64 = gu.data64_of(tree).copy()
    dd, bd = tree.data_dim, tree.basis_dim
    mag0 = t.backward64(d64, g)[1]
    touched = np.flatnonzero(mag0.reshape(-1, dd)[:, 0] > 0)
    slot, ch = int(_draw(np.random.default_rng(17), touched.tolist(), "a touched slot")), 1
    d64.reshape(-1, dd)[slot, ch * bd] = sign * 20.0 / 0.28209479177387814
    grad = t.backward64(d64, g)[0]
    first = np.unravel_index(slot * dd + ch * bd, d64.shape)
    assert 0 < abs(grad[first]) < 1e-6 * mag0[first], "the record is not saturated"
    for b in (0, 2, 6, 12):
        idx = np.unravel_index(slot * dd + ch * bd + b, d64.shape)
        fd = _fourth_order_difference(t, g, d64, idx, 0.2)
        print(f"u = {sign * 20}: b = {b} grad {grad[idx]:.6e} difference {fd:.6e} "
              f"relative {abs(fd - grad[idx]) / abs(grad[idx]):.2e}")
        assert abs(fd - grad[idx]) <= 1e-4 * abs(grad[idx]) + 2e-13, (b, grad[idx], fd)


def test_formulas_are_the_derivative_at_a_negative_sigma():
    """The SH4 scene with a fifth of its leaf densities at -0.5, marched with sigma_thresh = -1: those samples are
    hits with att > 1.  Central differences on such a density and on a coefficient of its record, in the style of
    test_formulas_are_the_derivative."""
    import dataclasses
    base = gu.tree_of("sh4")[0]
    rng = np.random.default_rng(23)
    data = np.array(base.data, np.float16, copy=True)
    leaf = np.asarray(base.child) == 0
    data[..., -1][leaf & (rng.random(leaf.shape) < 0.2)] = np.float16(-0.5)
    tree = dataclasses.replace(base, data=data)
    trs, w, h, f = gu.views("sh4", 24, 1)
    t = gu.Trace(tree, trs[0], w, h, f, 0, sigma_thresh=-1.0)
    g = gu.upstream("normal", 1, h, w, seed=21)[0].astype(np.float64)
    d64 = gu.data64_of(tree)
    grad, mag, _ = t.backward64(d64, g)
    dd, bd = tree.data_dim, tree.basis_dim
    flat, flat_mag = d64.reshape(-1, dd), mag.reshape(-1, dd)
    cand = np.flatnonzero((flat[:, -1] < 0) & (flat_mag[:, -1] > 0))
    assert cand.size > 10, "no negative density is a hit sample"
    for slot in rng.choice(cand, 3, replace=False):
        for e, what in ((dd - 1, "sigma"), (int(rng.integers(3)) * bd + int(rng.integers(bd)), "coefficient")):
            idx = np.unravel_index(int(slot) * dd + e, d64.shape)
            cd = _central_difference(t, g, d64, idx)
            err, m = abs(cd - grad[idx]), mag[idx]
            print(f"negative sigma, {what}: grad {grad[idx]:.6e} central difference {cd:.6e} |diff| / M = {err / m:.2e}")
            assert m > 0 and err <= 1e-6 * m, (what, grad[idx], cd, m)
