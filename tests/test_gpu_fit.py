"""vr_fit_rays on the GPU: the fused loss + backward of a ray list against what it fuses.

Rays: tests/rays_util.rays_of_camera over grad_util.views (tests/fit_util.py forms them in the FMA model's order for
fp_mode = 1, pinned against the oracle by tests/test_fit_restatement.py); targets: default_rng(seed).random((n, 3)).
Four checks per case, none with a tolerance of its own:
  accum      == render_rays(...)["accum"], bit for bit
  sq_err     == the numpy head (tests/fit_util.head) over that accum, bit for bit
  touched    == the bitmap of the marked render_backward_rays fed the numpy head's g, bit for bit
  grad_data  within K * unit of the float64 gradient for that g (grad_util.assert_parity: K and unit() as they stand),
             into a sentinel-filled buffer whose untouched elements keep their bits
Every run ends with status() == 0."""
import dataclasses
import functools

import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import fit_util as fu
from tests import grad_util as gu
from tests.fit_util import BG, assert_four, bits, dev, fit, options, unfused, zero_bits
from tests.grad_util import assert_parity, sentinel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def case_rays(ref, fp_mode):
    o, d = fu.camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"], fp_mode)
    return o, d, fu.targets(len(o), 100 + len(o))


# ---- 1. parity ---------------------------------------------------------------------------------------------------
PARITY = [(n, s, p, o, fp) for n, s, p in gu.PARITY_TREES for o in gu.OPTION_SETS for fp in (0, 1)]


@pytest.mark.parametrize("name,size,n_poses,optset,fp_mode", PARITY, ids=[f"{c[0]}-{c[3]}-fp{c[4]}" for c in PARITY])
def test_parity(torch_cuda, name, size, n_poses, optset, fp_mode):
    torch = torch_cuda
    ref = gu.reference(name, optset, fp_mode, n_poses, size)
    o, d, target = case_rays(ref, fp_mode)
    t = gu.upload(ref, name)
    try:
        _, _, fref = assert_four(torch, t, ref, o, d, target, fp_mode, f"fit {name} {optset} fp{fp_mode}")
    finally:
        t.free_device()
    assert (fref["mag"] > 0).sum() > 200, "the case shows nothing"


# ---- 2. segments -------------------------------------------------------------------------------------------------
# The fog tree's densest view leaves 0.31 of the light (sigma <= 0.4 over at most the volume's diagonal): no view of
# it reaches a kSegment restart, so the case is kept as the issue names it and a second one is added whose CPU trace
# shows the attenuation: the near SH9 scene without early stop, where most rays that hit end below 2^-40.
@pytest.mark.parametrize("name,size", [("fog", 40), ("sh9_near", 40)])
def test_segments(torch_cuda, name, size):
    torch = torch_cuda
    ref = gu.reference(name, (("stop_thresh", 0.0),), 0, 1, size)
    T = au.restate(ref["tree"], ref["trs"][0], ref["w"], ref["h"], ref["f"], 0, stop_thresh=0.0)[1]
    deep = int((T < 2.0 ** -20).sum())
    print(f"{name}: {deep} of {T.size} rays attenuate below 2^-20, min T = {float(T.min()):.3e}")
    if name != "fog":
        assert deep > 100, "no ray reaches a segment restart: the case shows nothing"
    o, d, target = case_rays(ref, 0)
    t = gu.upload(ref, name)
    try:
        assert_four(torch, t, ref, o, d, target, 0, f"segments {name}")
    finally:
        t.free_device()


# ---- 3. the shape of the list ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def list_reference():
    return gu.reference("sh16", "default", 0, 1, 96)        # 9216 rays


@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_list_sizes(torch_cuda, n):
    torch = torch_cuda
    ref = list_reference()
    o, d, target = case_rays(ref, 0)
    hitting = np.flatnonzero(ref["traces"][0].n_hits > 0)
    idx = np.random.default_rng(21 + n).choice(len(o), n, replace=False)
    if not np.isin(idx, hitting).any():        # (a list of one ray: one that has a hit sample)
        idx[0] = hitting[len(hitting) // 2]
    t = gu.upload(ref, "sh16")
    try:
        res, _, _ = assert_four(torch, t, ref, o[idx], d[idx], target[idx], 0, f"list of {n}", idx=idx)
        assert tuple(res["sq_err"].shape) == (n,) and tuple(res["accum"].shape) == (n, 4)
    finally:
        t.free_device()


def test_an_empty_list_writes_nothing(torch_cuda):
    torch = torch_cuda
    ref = list_reference()
    tree = ref["tree"]
    t = gu.upload(ref, "sh16")
    try:
        empty = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
        bytes0 = t.info()["device_bytes"]
        start = sentinel(tuple(tree.data.shape))
        buf, touched = dev(torch, start), zero_bits(torch, tree)
        res = t.fit_rays(empty, empty, options(ref), empty, grad_scale=1.0, grad_data=buf, touched=touched,
                         want=("sq_err", "accum"))
        torch.cuda.synchronize()
        assert res["grad_data"] is buf and t.status() == 0
        assert tuple(res["sq_err"].shape) == (0,) and tuple(res["accum"].shape) == (0, 4)
        assert t.info()["device_bytes"] == bytes0 + 4 * tree.capacity             # the file-order table, nothing else
        assert np.array_equal(bits(buf), bits(start)) and not bits(touched).any()
    finally:
        t.free_device()


def test_a_shuffled_list_and_a_split_list(torch_cuda):
    """Shuffled: the permuted sq_err / accum bits and the same bitmap.  Split into two calls on one buffer: the
    gradient accumulates to within K of the float64 gradient of the whole list, and each half's rows are the whole
    list's."""
    torch = torch_cuda
    ref = list_reference()
    o, d, target = case_rays(ref, 0)
    n = len(o)
    grad_scale = 2.0 / (3 * n)
    perm = np.random.default_rng(9).permutation(n)
    cut = 4097
    t = gu.upload(ref, "sh16")
    try:
        whole, touched = fit(torch, t, ref, o, d, target, 0, grad_scale)
        shuf, touched_s = fit(torch, t, ref, o[perm], d[perm], target[perm], 0, grad_scale)
        first, touched_2 = fit(torch, t, ref, o[:cut], d[:cut], target[:cut], 0, grad_scale)
        second, _ = fit(torch, t, ref, o[cut:], d[cut:], target[cut:], 0, grad_scale, grad_data=first["grad_data"],
                        touched=touched_2)
        torch.cuda.synchronize()
        assert t.status() == 0
        accum = whole["accum"].cpu().numpy()
        for key in ("sq_err", "accum"):
            assert np.array_equal(bits(shuf[key]), bits(whole[key])[perm]), key
            assert np.array_equal(np.concatenate([bits(first[key]), bits(second[key])]), bits(whole[key])), key
        assert np.array_equal(bits(touched_s), bits(touched)) and np.array_equal(bits(touched_2), bits(touched))
        fref = fu.reference_for(ref, fu.head(accum, target, BG, grad_scale)["g"])
        for what, r in (("whole", whole), ("shuffled", shuf), ("two calls", second)):
            assert_parity(r["grad_data"].cpu().numpy(), fref, what=what)
    finally:
        t.free_device()


# ---- 4. the outputs ----------------------------------------------------------------------------------------------
def test_each_output_is_optional(torch_cuda):
    """sq_err, accum and touched left out in turn: the others keep their bits, grad_data stays within K, and a
    sentinel-filled grad_data keeps its bits where no ray adds."""
    torch = torch_cuda
    ref = gu.reference("sh4", "default", 0, 1, 40)
    o, d, target = case_rays(ref, 0)
    grad_scale = 2.0 / (3 * len(o))
    start = sentinel(ref["grad"].shape)
    t = gu.upload(ref, "sh4")
    try:
        base, touched = fit(torch, t, ref, o, d, target, 0, grad_scale, start=start)
        runs = {
            "no sq_err": fit(torch, t, ref, o, d, target, 0, grad_scale, start=start, want=("accum",)),
            "no accum": fit(torch, t, ref, o, d, target, 0, grad_scale, start=start, want=("sq_err",)),
            "no touched": fit(torch, t, ref, o, d, target, 0, grad_scale, start=start, touched=None),
            "grad_data only": fit(torch, t, ref, o, d, target, 0, grad_scale, start=start, touched=None, want=()),
        }
        torch.cuda.synchronize()
        assert t.status() == 0
        fref = fu.reference_for(ref, fu.head(base["accum"].cpu().numpy(), target, BG, grad_scale)["g"])
        assert_parity(base["grad_data"].cpu().numpy(), fref, start=start, what="every output")
        assert bits(touched).any()
        for what, (res, tb) in runs.items():
            assert set(res) == {"grad_data"} | {k for k in ("sq_err", "accum") if k not in what and "only" not in what}
            for key in ("sq_err", "accum"):
                if key in res:
                    assert np.array_equal(bits(res[key]), bits(base[key])), (what, key)
            if tb is not None:
                assert np.array_equal(bits(tb), bits(touched)), what
            assert_parity(res["grad_data"].cpu().numpy(), fref, start=start, what=what)
    finally:
        t.free_device()


def test_zero_residual(torch_cuda):
    """target = the numpy head's pred: sq_err is +0 everywhere, grad_data keeps its values, and the slots are
    marked all the same."""
    torch = torch_cuda
    ref = gu.reference("sh4", "default", 0, 1, 40)
    o, d, _ = case_rays(ref, 0)
    start = sentinel(ref["grad"].shape)
    t = gu.upload(ref, "sh4")
    try:
        accum = t.render_rays(dev(torch, o), dev(torch, d), options(ref), want=("accum",))["accum"].cpu().numpy()
        target = fu.head(accum, np.zeros((len(o), 3), np.float32), BG, 1.0)["pred"]
        res, touched = fit(torch, t, ref, o, d, target, 0, 1.0, start=start)
        _, want, _, touched_b = unfused(torch, t, ref, o, d, target, 0, 1.0)
        torch.cuda.synchronize()
        assert t.status() == 0
        assert not want["g"].any() and (accum[:, 3] > 0).sum() > 100
        assert not bits(res["sq_err"]).any(), "sq_err is not +0 everywhere"
        assert np.array_equal(res["grad_data"].cpu().numpy(), start), "a zero residual changed grad_data"
        assert np.array_equal(bits(touched), bits(touched_b)) and bits(touched).any()
    finally:
        t.free_device()


# ---- 5. the optimiser --------------------------------------------------------------------------------------------
LR, LR_SIGMA = 0.5, 3.0      # (tests/test_gpu_step.py's: both exact in binary32; large enough to move binary16 values)


def test_optimizer_fit_and_step(torch_cuda, monkeypatch):
    """SparseTreeOptimizer.fit + step against render + the head in torch + backward + step, three SGD iterations on
    "sh4", each from the same start (the second optimiser is set to the first one's state before every iteration).
    The bound of one iteration.  Both gradients are runs of the backward formulas for one g (the torch head has the
    numpy head's bits: asserted), each within K * unit of the float64 gradient, so they differ by at most 2 K unit
    per element -- the bound tests/test_gpu_rays.py holds two backward runs to.  The step is bit-exact
    (tests/test_gpu_step.py): master' = master - rate * grad in binary32, two roundings, so the masters differ by at
    most rate * 2 K unit + 2^-23 (|master'| + rate |grad|).  The unit is that of the iteration's own tree: the trace
    and float64 magnitudes of binary16(master) as the iteration finds it.  grad_scale = 1 / 4 where the default
    2 / (3 n) would move no binary16 value in three steps; the default is looked at by itself at the end."""
    torch = torch_cuda
    from volrend_amd import api, optim
    base = gu.reference("sh4", "default", 0, 1, 40)
    tree0 = base["tree"]
    o, d, target = case_rays(base, 0)
    n = len(o)
    grad_scale = 0.25
    opts = options(base)
    od, dd_, td = dev(torch, o), dev(torch, d), dev(torch, target)
    rate = np.full(tree0.data_dim, LR, np.float64)
    rate[-1] = LR_SIGMA
    ta, tb = gu.upload(base, "sh4"), gu.upload(base, "sh4")
    fresh = None
    try:
        a = optim.SparseTreeOptimizer(ta, "sgd", lr=LR, lr_sigma=LR_SIGMA, options=opts)
        b = optim.SparseTreeOptimizer(tb, "sgd", lr=LR, lr_sigma=LR_SIGMA, options=opts)
        moved = 0
        for it in range(3):
            b.master.copy_(a.master)
            tb.update_data(a.master)
            held = ta.read_data().cpu().numpy()
            assert np.array_equal(held.view(np.uint16), tb.read_data().cpu().numpy().view(np.uint16))
            # path A
            sq_err = a.fit(od, dd_, td, grad_scale=grad_scale)
            torch.cuda.synchronize()
            marks_a = bits(a.touched).copy()
            # path B: the loss head in torch, operator by operator as the header orders it
            accum = b.render(od, dd_)
            na = 1.0 - accum[:, 3]
            r = (accum[:, :3] + (BG * na)[:, None]) - td
            g3 = grad_scale * r
            g = torch.cat([g3, -(BG * ((g3[:, 0] + g3[:, 1]) + g3[:, 2]))[:, None]], 1)
            b.backward(od, dd_, g)
            torch.cuda.synchronize()
            want = fu.head(accum.cpu().numpy(), target, BG, grad_scale)
            assert np.array_equal(bits(g), bits(want["g"])), "the torch head is not the numpy head"
            assert np.array_equal(bits(sq_err), bits(want["sq_err"]))
            assert np.array_equal(marks_a, bits(b.touched)) and marks_a.any()
            grad_b = b.grad.cpu().numpy().astype(np.float64)
            a.step()
            b.step()
            torch.cuda.synchronize()
            # the unit of this iteration
            now = dataclasses.replace(tree0, data=np.ascontiguousarray(held, np.float16))
            tr = gu.Trace(now, base["trs"][0], base["w"], base["h"], base["f"], 0, **base["opt"])
            _, mag, under = tr.backward64(gu.data64_of(now), want["g"].astype(np.float64).reshape(base["h"], base["w"], 4))
            unit = gu.unit(dict(mag=mag, under=under))
            ma, mb = a.master.cpu().numpy().astype(np.float64), b.master.cpu().numpy().astype(np.float64)
            bound = rate * 2 * gu.K * unit + 2.0 ** -23 * (np.abs(mb) + rate * np.abs(grad_b))
            worst = float((np.abs(ma - mb) / np.maximum(bound, 1e-300)).max())
            print(f"iteration {it}: worst |master fit - master unfused| / bound = {worst:.4f}")
            assert (np.abs(ma - mb) <= bound).all(), it
            for opt_, t_ in ((a, ta), (b, tb)):
                assert torch.equal(t_.read_data(dtype=torch.float16).view(torch.int16), opt_.master.half().view(torch.int16))
                assert not bool(opt_.grad.any()) and not bool(opt_.touched.any())
            moved += int((ta.read_data().cpu().numpy().view(np.uint16) != held.view(np.uint16)).sum())
        assert ta.status() == 0 and tb.status() == 0 and a.steps == 3 and moved > 100
        # the tree is a fresh upload of binary16(master)
        fresh = api.N3Tree.from_synth(dataclasses.replace(tree0, data=a.master.half().cpu().numpy()))
        mine = ta.render_rays(od, dd_, opts, want=("accum",))["accum"]
        theirs = fresh.render_rays(od, dd_, opts, want=("accum",))["accum"]
        assert np.array_equal(bits(mine), bits(theirs))
        assert np.array_equal(ta.read_data().cpu().numpy().view(np.uint16), fresh.read_data().cpu().numpy().view(np.uint16))
        # the default grad_scale is the mean's
        seen = {}
        real = api.fit_rays
        monkeypatch.setattr(api, "fit_rays", lambda *args, **kw: (seen.update(kw), real(*args, **kw))[1])
        sq_err = a.fit(od, dd_, td)
        torch.cuda.synchronize()
        assert seen["grad_scale"] == 2.0 / (3 * n) and tuple(sq_err.shape) == (n,) and bool(a.touched.any())
    finally:
        ta.free_device()
        tb.free_device()
        if fresh is not None:
            fresh.free_device()


# ---- 6. refusals that need the tree ------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["SG", "ASG", "basis_minmax"])
def test_refusals_on_a_real_tree(torch_cuda, what):
    torch = torch_cuda
    from volrend_amd import _abi, api
    if what == "basis_minmax":
        tree, opts = gu.tree_of("sh4")[0], api.RenderOptions(basis_minmax=(0, 2))
    else:
        tree, opts = common.small_scene(depth=4, basis_dim=9, fmt=what, seed=2), api.RenderOptions()
    t = api.N3Tree.from_synth(tree)
    try:
        z = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
        buf = dev(torch, sentinel(tuple(tree.data.shape)))
        with pytest.raises(_abi.VolrendError) as e:
            t.fit_rays(z, z, opts, z, grad_scale=1.0, grad_data=buf, want=())
        assert e.value.code == 5 and "vr_fit_rays" in str(e.value) and (what in str(e.value) or "SG / ASG" in str(e.value))
        torch.cuda.synchronize()
        assert np.array_equal(bits(buf), bits(sentinel(tuple(tree.data.shape)))) and t.status() == 0
    finally:
        t.free_device()
