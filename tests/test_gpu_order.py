"""vr_order_rays on the GPU against the restatement of its key (tests/order_util.py over the oracle's functions) and
the result rule: keys == the restatement's keys sorted, order == numpy's stable argsort of the unsorted keys, the
gathered arrays == input[order], all bit for bit; inputs unchanged; guard words around every output and behind the
workspace intact.  Then what the order is for: the ray-list calls give the same results on the ordered list."""
import dataclasses

import numpy as np
import pytest

from tests import fit_util as fu
from tests import grad_util as gu
from tests import order_util as ou
from tests import rays_util as ru
from tests import step_util as su

pytestmark = pytest.mark.gpu
GUARD = 16                                   # words in front of and behind every output
GW = ou.KEY_WAVES
SIZES = (0, 1, 63, 64, 65, 64 * GW - 1, 64 * GW + 1, 3000)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


@pytest.fixture(scope="module")
def trees(torch_cuda):
    """The scenes of tests/order_util.py on the device, uploaded once."""
    from volrend_amd import api
    up = {name: api.N3Tree.from_synth(ou.scene(name)[0], ndc=ou.scene(name)[1]) for name in ("plain", "ndc")}
    up["bbox"] = up["plain"]
    yield up
    for name in ("plain", "ndc"):
        up[name].free_device()


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    return t.cpu().numpy()


class Guarded:
    """An output of ``shape`` in the middle of a sentinel-filled buffer: GUARD words either side."""

    def __init__(self, torch, shape, dtype, fill):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n].view(*shape) if n else self.buf[GUARD:GUARD].view(*shape)
        self.n, self.fill = n, fill

    def intact(self):
        b = host(self.buf)
        return bool((b[:GUARD] == self.fill).all() and (b[GUARD + self.n:] == self.fill).all())


def run(torch, t, o, d, opts, bits, fp_mode, payloads=(), want=("order", "keys", "origins", "dirs")):
    """One guarded call per payload (none: one call) -> list of (result as numpy, inputs on the device)."""
    from volrend_amd import _abi
    n = len(o)
    outs = []
    for payload in (payloads or (None,)):
        od, dd = dev(torch, o), dev(torch, d)
        pd = None if payload is None else dev(torch, payload)
        g = {"order": Guarded(torch, (n,), torch.int32, -7), "keys": Guarded(torch, (n,), torch.int32, -9),
             "origins": Guarded(torch, (n, 3), torch.float32, -3.5), "dirs": Guarded(torch, (n, 3), torch.float32, -4.5)}
        if payload is not None:
            g["payload"] = Guarded(torch, payload.shape, torch.float32, -5.5)
        need = int(_abi.lib().vr_order_rays_workspace(n))
        ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        res = t.order_rays(od, dd, opts, bits=bits, payload=pd, want=want, out={k: v.view for k, v in g.items()},
                           workspace=ws[:need] if n else None, fp_mode=fp_mode)
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values()), "a guard word around an output was written"
        assert bool((ws[need:] == 0x5A).all()), "a byte behind the workspace was written"
        assert np.array_equal(host(od), o) and np.array_equal(host(dd), d), "an input was modified"
        assert payload is None or np.array_equal(host(pd).view(np.uint32), payload.view(np.uint32))
        for k, v in g.items():
            assert res[k] is v.view                          # what a caller passes is returned as passed
        outs.append({k: host(v.view) for k, v in g.items()})
    return outs


def check(out, keys_unsorted, o, d, payload=None, what=""):
    order, keys = ou.result_of(np.asarray(keys_unsorted))
    assert np.array_equal(out["keys"].view(np.uint32), keys), f"{what}: keys differ from the restatement's, sorted"
    assert np.array_equal(out["order"].view(np.uint32), order), f"{what}: order is not the stable argsort of the keys"
    assert np.array_equal(out["origins"].view(np.uint32), o[order].view(np.uint32)), f"{what}: origins"
    assert np.array_equal(out["dirs"].view(np.uint32), d[order].view(np.uint32)), f"{what}: dirs"
    if payload is not None:
        assert np.array_equal(out["payload"].view(np.uint32), payload[order].view(np.uint32)), f"{what}: payload"


# ---- 1. parity ---------------------------------------------------------------------------------------------------
CASES = [("plain", fp, b) for fp in (0, 1) for b in (1, 3, 5, 0)] + \
        [(s, fp, b) for s in ("ndc", "bbox") for fp in (0, 1) for b in (0, 5)]


@pytest.mark.parametrize("name,fp_mode,bits", CASES, ids=[f"{c[0]}-fp{c[1]}-bits{c[2]}" for c in CASES])
def test_parity(torch_cuda, trees, name, fp_mode, bits):
    torch = torch_cuda
    from volrend_amd import api
    opts = api.RenderOptions(**ou.scene(name)[2])
    seen_miss = seen_hit = 0
    for n in SIZES:
        o, d = ou.rays(name, n)
        ref = ou.reference(name, n, bits, fp_mode)
        rng = np.random.default_rng(n)
        # a 3-wide and an 8-wide payload whose words are all different (NaN patterns included: bit copies)
        p3 = rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
        p8 = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32).view(np.float32)
        for out, payload in zip(run(torch, trees[name], o, d, opts, bits, fp_mode, (p3, p8)), (p3, p8)):
            check(out, ref, o, d, payload, f"{name} n={n} fp{fp_mode} bits={bits} payload {payload.shape[1]}")
        seen_miss += int((ref == ou.MISS).sum())
        seen_hit += int((ref != ou.MISS).sum())
    assert seen_hit > 1000 and (name == "ndc" or seen_miss > 100), "the case shows nothing"
    assert trees[name].status() == 0


def test_above_the_merge_sort_limit(torch_cuda, trees):
    """The sort is rocPRIM's: a block sort up to 1,024 pairs, a merge sort up to 2^20, its onesweep radix sort above
    -- another set of kernels and another temporary-storage layout (the sizes of test_parity stay below).  One list
    just above the limit, the finest key; the call itself checks that the workspace rule covers what the sort asks."""
    torch = torch_cuda
    from volrend_amd import api
    n = (1 << 20) + 65
    o, d = ou.rays("plain", n)
    ref = ou.reference("plain", n, 5, 0)
    check(run(torch, trees["plain"], o, d, api.RenderOptions(), 5, 0)[0], ref, o, d, None, f"n={n}")


def test_outputs_that_are_not_wanted_and_allocation(torch_cuda, trees):
    """The defaults: the function allocates outputs and workspace; keys and payload only when asked for."""
    torch = torch_cuda
    from volrend_amd import api
    o, d = ou.rays("plain", 500)
    ref = ou.reference("plain", 500, 0, 0)
    res = trees["plain"].order_rays(dev(torch, o), dev(torch, d), api.RenderOptions())
    torch.cuda.synchronize()
    assert sorted(res) == ["dirs", "order", "origins", "workspace"]
    order = ou.result_of(np.asarray(ref))[0]
    assert np.array_equal(host(res["order"]).view(np.uint32), order)
    assert np.array_equal(host(res["origins"]), o[order]) and np.array_equal(host(res["dirs"]), d[order])
    res = trees["plain"].order_rays(dev(torch, o), dev(torch, d), api.RenderOptions(), want=("order",))
    torch.cuda.synchronize()
    assert sorted(res) == ["order", "workspace"] and np.array_equal(host(res["order"]).view(np.uint32), order)
    res = trees["plain"].order_rays(dev(torch, o[:0]), dev(torch, d[:0]), api.RenderOptions(), want=("order", "keys"))
    assert sorted(res) == ["keys", "order"] and res["order"].shape == (0,)


# ---- 2. degenerate lists -----------------------------------------------------------------------------------------
def test_degenerate_lists(torch_cuda, trees):
    torch = torch_cuda
    from volrend_amd import api
    tree = ou.scene("plain")[0]
    opts = api.RenderOptions()
    # every ray misses: 50 box diagonals out, pointing further away
    o, d = ou.rays("plain", 300)
    lo, hi = ru.world_box(tree)
    u = np.random.default_rng(2).standard_normal((300, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    far = np.ascontiguousarray((lo + hi) / 2 + 50.0 * np.linalg.norm(hi - lo) * u, np.float32)
    away = np.ascontiguousarray(u, np.float32)
    assert (ou.keys_of(tree, far, away, 3) == ou.MISS).all()
    out = run(torch, trees["plain"], far, away, opts, 3, 0)[0]
    assert np.array_equal(out["order"], np.arange(300)) and (out["keys"].view(np.uint32) == ou.MISS).all()
    assert np.array_equal(out["origins"], far) and np.array_equal(out["dirs"], away)
    # 300 copies of one ray
    one_o, one_d = np.repeat(o[5:6], 300, 0), np.repeat(d[5:6], 300, 0)
    k = ou.keys_of(tree, one_o, one_d, 5)
    assert k[0] != ou.MISS
    out = run(torch, trees["plain"], one_o, one_d, opts, 5, 0)[0]
    assert np.array_equal(out["order"], np.arange(300)) and (out["keys"].view(np.uint32) == k[0]).all()
    # bits = 1 on 3000 rays: at most 65 distinct keys, so long runs of ties -- the stability case
    o, d = ou.rays("plain", 3000)
    ref = np.asarray(ou.reference("plain", 3000, 1, 0))
    assert len(np.unique(ref)) <= 65 and np.bincount(np.unique(ref, return_inverse=True)[1]).max() > 100
    check(run(torch, trees["plain"], o, d, opts, 1, 0)[0], ref, o, d, None, "ties")


# ---- 3. order-independence, end to end ---------------------------------------------------------------------------
BG = 0.625


def bits_of(a):
    return np.ascontiguousarray(host(a) if hasattr(a, "cpu") else a).view(np.uint32)


@pytest.mark.parametrize("fp_mode", [0, 1])
def test_fit_rays_on_the_ordered_list(torch_cuda, fp_mode):
    """fit_rays on a shuffled batch, and on the same batch ordered with the targets as the payload: accum and
    sq_err scattered back through ``order``, and touched, are the unordered call's bit for bit; each grad_data is
    within K * unit of the float64 gradient (grad_util.assert_parity as it stands), so the two are within 2 K unit of
    each other -- the bound two backward runs of the same rays are held to."""
    torch = torch_cuda
    from volrend_amd import api
    ref = gu.reference("sh4", "default", fp_mode, 1, 40)
    o, d = fu.camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"], fp_mode)
    n = len(o)
    perm = np.random.default_rng(12).permutation(n)                 # the batch as an optimiser draws it
    o, d, target = np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm]), fu.targets(n, 100 + n)
    grad_scale = 2.0 / (3 * n)
    opts = api.RenderOptions(**dict(ref["opt"], background_brightness=BG))
    start = gu.sentinel(ref["grad"].shape)
    t = gu.upload(ref, "sh4")
    try:
        words = su.n_words(ref["tree"].capacity * ref["tree"].N ** 3)
        od, dd, td = dev(torch, o), dev(torch, d), dev(torch, target)
        ta = torch.zeros(words, dtype=torch.int32, device="cuda")
        a = t.fit_rays(od, dd, opts, td, grad_scale=grad_scale, grad_data=dev(torch, start), touched=ta,
                       want=("sq_err", "accum"), fp_mode=fp_mode)
        r = t.order_rays(od, dd, opts, payload=td, fp_mode=fp_mode)
        tb = torch.zeros(words, dtype=torch.int32, device="cuda")
        b = t.fit_rays(r["origins"], r["dirs"], opts, r["payload"], grad_scale=grad_scale, grad_data=dev(torch, start),
                       touched=tb, want=("sq_err", "accum"), fp_mode=fp_mode)
        torch.cuda.synchronize()
        assert t.status() == 0
        order = host(r["order"]).astype(np.int64)
        assert not np.array_equal(order, np.arange(n)) and np.array_equal(np.sort(order), np.arange(n))
        for name in ("accum", "sq_err"):
            back = np.empty_like(host(b[name]))
            back[order] = host(b[name])
            assert np.array_equal(bits_of(back), bits_of(a[name])), f"{name} depends on the order of the rays"
        assert np.array_equal(bits_of(ta), bits_of(tb)) and bits_of(ta).any(), "touched depends on the order"
        g = np.zeros((n, 4), np.float32)
        g[perm] = fu.head(host(a["accum"]), target, BG, grad_scale)["g"]
        fref = fu.reference_for(ref, g)
        ga, gb = host(a["grad_data"]), host(b["grad_data"])
        gu.assert_parity(ga, fref, start=start, what=f"unordered fp{fp_mode}")
        gu.assert_parity(gb, fref, start=start, what=f"ordered fp{fp_mode}")
        pos = fref["mag"] > 0
        worst = float((np.abs(ga.astype(np.float64) - gb)[pos] / gu.unit(fref)[pos]).max())
        print(f"fp{fp_mode}: worst |ordered - unordered| / unit = {worst:.3f} of {2 * gu.K}")
        assert worst <= 2 * gu.K
    finally:
        t.free_device()


# ---- 4. SparseTreeOptimizer(reorder=True) ------------------------------------------------------------------------
LR, LR_SIGMA = 0.5, 3.0      # (tests/test_gpu_step.py's: both exact in binary32; large enough to move binary16 values)


def disjoint_batch(ref, rng):
    """Rays of the view of ``ref`` of which no two share a leaf slot, and none meets a slot twice: every element of
    the gradient then receives at most ONE contribution, and no order of a float sum can matter.  Chosen greedily in
    a seeded random order from the record of the hits -> (ray indices, hits per slot over the batch)."""
    tr = ref["traces"][0]
    slots, ray = tr.all_slots()
    taken = np.zeros(int(np.prod(ref["grad"].shape[:-1])), bool)
    starts = np.concatenate([[0], np.cumsum(tr.n_hits)])
    picked = []
    for i in rng.permutation(tr.n_hits.size):
        s = slots[starts[i]:starts[i + 1]]
        if s.size and len(np.unique(s)) == s.size and not taken[s].any():
            taken[s] = True
            picked.append(int(i))
    picked = np.array(picked)
    hits = np.bincount(np.concatenate([slots[starts[i]:starts[i + 1]] for i in picked]), minlength=taken.size)
    assert (ray[starts[picked]] == picked).all()
    return picked, hits


def test_optimizer_with_reorder(torch_cuda):
    torch = torch_cuda
    from volrend_amd import api, optim
    ref = gu.reference("sh4", "default", 0, 1, 40)
    tree0 = ref["tree"]
    o_all, d_all = fu.camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"], 0)
    rng = np.random.default_rng(8)
    picked, hits = disjoint_batch(ref, rng)
    assert hits.max() == 1 and len(picked) >= 20, "shown on the CPU: no slot is hit twice by the batch"
    opts = api.RenderOptions(**dict(ref["opt"], background_brightness=BG))
    rate = np.full(tree0.data_dim, LR, np.float64)
    rate[-1] = LR_SIGMA
    ta, tb = gu.upload(ref, "sh4"), gu.upload(ref, "sh4")
    try:
        a = optim.SparseTreeOptimizer(ta, "sgd", lr=LR, lr_sigma=LR_SIGMA, options=opts, reorder=True)
        b = optim.SparseTreeOptimizer(tb, "sgd", lr=LR, lr_sigma=LR_SIGMA, options=opts, reorder=False)
        # (a) the batch without shared leaves: everything bit for bit
        o, d = np.ascontiguousarray(o_all[picked]), np.ascontiguousarray(d_all[picked])
        target = fu.targets(len(o), 55)
        od, dd, td = dev(torch, o), dev(torch, d), dev(torch, target)
        order = host(ta.order_rays(od, dd, opts, want=("order",))["order"])
        assert not np.array_equal(order, np.arange(len(o))), "the batch is already in order: the case shows nothing"
        sa, sb = a.fit(od, dd, td, grad_scale=0.25), b.fit(od, dd, td, grad_scale=0.25)
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(sa), bits_of(sb)), "sq_err is not handed back in the caller's order"
        assert np.array_equal(bits_of(a.touched), bits_of(b.touched)) and bits_of(a.touched).any()
        assert np.array_equal(bits_of(a.grad), bits_of(b.grad)), "one contribution per element, yet the sums differ"
        assert np.array_equal(bits_of(a.render(od, dd)), bits_of(b.render(od, dd)))
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(a.master), bits_of(b.master))
        held = host(ta.read_data())
        assert np.array_equal(held.view(np.uint16), host(tb.read_data()).view(np.uint16))
        assert (held.view(np.uint16) != np.ascontiguousarray(tree0.data, np.float16).view(np.uint16)).any()
        # (b) the whole view, shuffled: the bound of one iteration (tests/test_gpu_fit.py::test_optimizer_fit_and_step)
        perm = rng.permutation(len(o_all))
        o, d, target = np.ascontiguousarray(o_all[perm]), np.ascontiguousarray(d_all[perm]), fu.targets(len(o_all), 56)
        od, dd, td = dev(torch, o), dev(torch, d), dev(torch, target)
        accum = host(b.render(od, dd))
        sa, sb = a.fit(od, dd, td, grad_scale=0.25), b.fit(od, dd, td, grad_scale=0.25)
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(sa), bits_of(sb)) and np.array_equal(bits_of(a.touched), bits_of(b.touched))
        grad_b = host(b.grad).astype(np.float64)
        a.step()
        b.step()
        torch.cuda.synchronize()
        now = dataclasses.replace(tree0, data=np.ascontiguousarray(held, np.float16))
        tr = gu.Trace(now, ref["trs"][0], ref["w"], ref["h"], ref["f"], 0, **ref["opt"])
        g = np.zeros((len(o_all), 4), np.float32)
        g[perm] = fu.head(accum, target, BG, 0.25)["g"]
        _, mag, under = tr.backward64(gu.data64_of(now), g.astype(np.float64).reshape(ref["h"], ref["w"], 4))
        unit = gu.unit(dict(mag=mag, under=under))
        ma, mb = host(a.master).astype(np.float64), host(b.master).astype(np.float64)
        bound = rate * 2 * gu.K * unit + 2.0 ** -23 * (np.abs(mb) + rate * np.abs(grad_b))
        worst = float((np.abs(ma - mb) / np.maximum(bound, 1e-300)).max())
        print(f"worst |master reorder - master plain| / bound = {worst:.4f}")
        assert (np.abs(ma - mb) <= bound).all()
        assert ta.status() == 0 and tb.status() == 0
    finally:
        ta.free_device()
        tb.free_device()


def test_tree_rays_with_reorder(torch_cuda):
    """TreeRays(reorder=True): the forward's accumulators are the unordered module's bit for bit, in the caller's
    order; the gradients agree within 2 K unit."""
    torch = torch_cuda
    from volrend_amd import api, optim
    ref = gu.reference("sh4", "default", 0, 1, 40)
    o, d = fu.camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"], 0)
    perm = np.random.default_rng(3).permutation(len(o))
    od, dd = dev(torch, o[perm]), dev(torch, d[perm])
    g = gu.upstream("normal", 1, ref["h"], ref["w"]).reshape(-1, 4)       # (in the view's order; the batch: [perm])
    gd = dev(torch, g[perm])
    opts = api.RenderOptions(**ref["opt"])
    ta, tb = gu.upload(ref, "sh4"), gu.upload(ref, "sh4")
    try:
        grads = []
        for t, reorder in ((ta, True), (tb, False)):
            m = optim.TreeRays(t, opts, reorder=reorder)
            out = m(od, dd)
            out.backward(gd)
            torch.cuda.synchronize()
            grads.append((host(out.detach()), host(m.data.grad)))
        assert np.array_equal(bits_of(grads[0][0]), bits_of(grads[1][0]))
        fref = fu.reference_for(ref, g)
        for got, what in ((grads[0][1], "reorder"), (grads[1][1], "plain")):
            gu.assert_parity(got, fref, what=what)
    finally:
        ta.free_device()
        tb.free_device()
