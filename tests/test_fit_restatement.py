"""The yardstick of the vr_fit_rays tests (tests/fit_util.py), tied down without a GPU: the loss head's g is the
derivative of L = grad_scale / 2 * sum r^2 through trace_ray's out[] -- which proves g_3 = -bg sum g_ch and the
grad_scale convention -- and the FMA model's camera rays are the oracle's."""
import numpy as np
import pytest

from tests import common
from tests import fit_util as fu
from tests import grad_util as gu
from tests import rays_util as ru
from tests.test_grad_restatement import _draw, _sigma_slots_by_stop

BG, GRAD_SCALE = 0.625, 0.37     # (a background that is not 0 or 1: g_3 matters; any finite scale)


def _loss_rays(t, d64, target):
    out = t.forward64(d64)[0].reshape(-1, 4)
    return fu.loss64(out, target, BG, GRAD_SCALE)


def _central_difference(t, d64, idx, target):
    """tests/test_grad_restatement.py's, of L: ray by ray, so that a ray the element does not reach adds an exact 0."""
    v = d64[idx]
    h = 1e-5 * max(abs(v), 1.0)
    d64[idx] = v + h
    up = _loss_rays(t, d64, target)
    d64[idx] = v - h
    dn = _loss_rays(t, d64, target)
    d64[idx] = v
    return float((up - dn).sum() / (2 * h))


@pytest.mark.parametrize("name", ["sh4", "rgba"])
def test_the_heads_g_is_the_derivative_of_the_loss(name):
    """Central differences in float64 of L over forward64 against backward64 fed with the head's g, in a sigma only
    stopped rays reach, a sigma only unstopped rays reach and a colour entry; the tolerance is the one
    tests/test_grad_restatement.py::test_formulas_are_the_derivative applies (1e-6 M)."""
    tree = gu.tree_of(name)[0]
    trs, w, h, f = gu.views(name, 24, 1)
    t = gu.Trace(tree, trs[0], w, h, f, 0, background_brightness=BG)
    target = fu.targets(w * h, 31).astype(np.float64)
    d64 = gu.data64_of(tree)
    out = t.forward64(d64)[0].reshape(-1, 4)
    g = fu.head(out, target, BG, GRAD_SCALE, np.float64)["g"]
    assert (g[:, 3] != 0).any()
    grad, mag, _ = t.backward64(d64, g.reshape(h, w, 4))
    dd, bd = tree.data_dim, tree.basis_dim
    flat_mag = mag.reshape(-1, dd)
    rng = np.random.default_rng(5)
    only_stopped, only_open = _sigma_slots_by_stop(t)
    picks = []
    for slots, what in ((only_stopped, "sigma, stopped rays only"), (only_open, "sigma, unstopped rays only")):
        picks.append((_draw(rng, [s for s in slots if flat_mag[s, dd - 1] > 0], what), dd - 1, what))
    touched = np.nonzero(flat_mag[:, 0] > 0)[0].tolist()
    ch = int(rng.integers(3))
    picks.append((_draw(rng, touched, "colour"), ch * bd + int(rng.integers(bd)) if bd > 0 else ch, "colour entry"))
    for slot, e, what in picks:
        idx = np.unravel_index(slot * dd + e, d64.shape)
        cd = _central_difference(t, d64, idx, target)
        err, m = abs(cd - grad[idx]), mag[idx]
        print(f"{name} {what}: grad {grad[idx]:.6e} central difference {cd:.6e} |diff| / M = {err / m:.2e}")
        assert m > 0 and err <= 1e-6 * m, (what, grad[idx], cd, m)


def test_binary32_head_is_the_binary64_head_rounded():
    """The float32 head against the float64 one on the same inputs: every entry within a few roundings of its
    operands' size, and sq_err >= 0, +0 for a zero residual."""
    rng = np.random.default_rng(2)
    out = rng.random((500, 4), np.float32)
    out[::7, 3] = 1.0
    target = fu.targets(500, 3)
    a, b = fu.head(out, target, BG, GRAD_SCALE), fu.head(out, target, BG, GRAD_SCALE, np.float64)
    eps = 2.0 ** -24
    assert (np.abs(a["r"] - b["r"]) <= 3 * eps * 2.0).all()                    # (|pred|, |target| < 2)
    assert (np.abs(a["sq_err"] - b["sq_err"]) <= 12 * eps * np.maximum(b["sq_err"], 1e-30) + 1e-12).all()
    assert (np.abs(a["g"][:, :3] - b["g"][:, :3]) <= 4 * eps * 2.0 * GRAD_SCALE).all()
    assert (np.abs(a["g"][:, 3] - b["g"][:, 3]) <= 16 * eps * 2.0 * GRAD_SCALE * 3 * BG).all()
    pred = a["pred"]
    z = fu.head(out, pred, BG, GRAD_SCALE)
    assert (z["sq_err"].view(np.uint32) == 0).all() and not z["g"].any()


def test_fma_camera_rays_are_the_oracles():
    """fit_util.rays_of_camera(fp_mode = 1): every ray through the oracle as its own camera (tests/rays_util.py)
    gives the accumulators of the oracle's FMA frame bit for bit -- and the strict order does not, so the case
    shows something."""
    tree = gu.tree_of("sh4")[0]
    trs, w, h, f = gu.views("sh4", 24, 2)
    tr = trs[1]                                  # (a rotation without zeros: pose 0 is exact in either order)
    _, acc, _ = common.oracle_frame(tree, tr, w, h, f, 1)
    o, d = fu.rays_of_camera(tr, w, h, f, 1)
    _, got, _ = ru.oracle_rays(tree, o, d, 1)
    assert np.array_equal(got.view(np.uint32), acc.reshape(-1, 4).view(np.uint32))
    o0, d0 = fu.rays_of_camera(tr, w, h, f, 0)
    assert not np.array_equal(d0.view(np.uint32), d.view(np.uint32))
    assert np.array_equal(d0, ru.rays_of_camera(tr, w, h, f)[1])
