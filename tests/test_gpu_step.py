"""The sparse optimiser step on the GPU: the marked backward calls (vr_render_backward_touched,
vr_render_backward_rays_touched), vr_tree_step and volrend_amd.optim.SparseTreeOptimizer.

Everything about the step is bit-exact: the expected side is the numpy binary32 restatement (tests/step_util.py),
the dense vr_tree_update_data or a FRESH upload of the expected data.  The marks are compared with hits > 0 of
vr_accumulate_weights_rays, an independently tested call; the marked gradient passes the check and the bound of
tests/test_gpu_grad.py (no new tolerance).  Scenes: tests/update_util.py; rays: the scene's two poses through
tests/rays_util.rays_of_camera.  The step's value domain (section 8) runs the catalogue of tests/step_util.py, whose
strength tests/test_step_host.py shows on the CPU; every record shape and the bitmap patterns:
tests/test_gpu_step_shapes.py."""
import functools

import numpy as np
import pytest

from tests import grad_util as gu
from tests import query_util as qu
from tests import rays_util as ru
from tests import step_util as su
from tests import update_util as uu
from tests.grad_util import assert_parity
from tests.update_util import dev, upload

pytestmark = pytest.mark.gpu
LR, LR_SIGMA = 0.5, 3.0      # (both exact in binary32; large enough to move binary16 values)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def n_slots(tree):
    return tree.capacity * tree.N ** 3


@functools.lru_cache(maxsize=None)
def rays_of(name):
    """-> (origins [n, 3], dirs [n, 3], grad_accum [n, 4]) of the scene's two poses, frame after frame."""
    c = uu.case(name)
    parts = [ru.rays_of_camera(tr, c["w"], c["h"], c["f"]) for tr in c["trs"]]
    g = gu.upstream("normal", len(c["trs"]), c["h"], c["w"])
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), g.reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def reference(name, fp_mode):
    """The float64 gradient of the scene's two poses, as grad_util.reference forms it -> its dict."""
    c = uu.case(name)
    if name in ("sh16", "sh25", "sh9_near", "rgba", "basis1"):
        ref = gu.reference(name, "default", fp_mode, 2, 48)      # (the views of update_util.case)
        assert ref["w"] == c["w"] and all(np.array_equal(a, b) for a, b in zip(ref["trs"], c["trs"]))
        return ref
    tree = c["tree"]
    g = gu.upstream("normal", len(c["trs"]), c["h"], c["w"])
    d64 = gu.data64_of(tree)
    grad, mag, under = (np.zeros(d64.shape, np.float64) for _ in range(3))
    for i, tr in enumerate(c["trs"]):
        gu.Trace(tree, tr, c["w"], c["h"], c["f"], fp_mode, ndc=c["ndc"]).backward64(d64, g[i].astype(np.float64), grad,
                                                                                     mag, under)
    return dict(tree=tree, ndc=c["ndc"], trs=c["trs"], w=c["w"], h=c["h"], f=c["f"], g=g, grad=grad, mag=mag,
                under=under, opt={})


def zero_bits(torch, tree):
    return torch.zeros(su.n_words(n_slots(tree)), dtype=torch.int32, device="cuda")


def host_bits(x):
    return x.cpu().numpy().view(np.uint32)


def marked_rays(torch, t, name, fp_mode=0, touched=None, grad_data=None):
    """The marked ray-list call over the scene's rays -> (grad_data, touched), device tensors."""
    from volrend_amd import api
    o, d, g = rays_of(name)
    touched = zero_bits(torch, uu.case(name)["tree"]) if touched is None else touched
    grad = t.render_backward_rays(dev(torch, o), dev(torch, d), api.RenderOptions(), dev(torch, g), grad_data=grad_data,
                                  fp_mode=fp_mode, touched=touched)
    return grad, touched


# ---- 1. the marks are the hit set --------------------------------------------------------------------------------
# (edge_*: the full-catalogue value-domain trees of tests/grad_util.py -- NaN and +-inf in records.  A mark depends
# on sigma > sigma_thresh alone: NaN sigma never marks, +inf sigma does, dirty or clean makes no difference.)
MARK_CASES = [("sh16", 0), ("sh16", 1), ("sh25", 0), ("sh9_near", 0), ("rgba", 0), ("basis1", 0), ("n3", 0), ("chain", 0),
              ("edge_sh16", 0), ("edge_rgba", 0)]


def cpu_hit_set(name):
    """The slots with a hit sample in the scene's two poses, marched by the restatement (strict model), and the
    float32 sigma of every slot."""
    c = uu.case(name)
    tree = c["tree"]
    hit = np.zeros(n_slots(tree), bool)
    for tr in c["trs"]:
        hit[gu.Trace(tree, tr, c["w"], c["h"], c["f"], 0).all_slots()[0]] = True
    return hit, np.asarray(tree.data, np.float32).reshape(-1, tree.data_dim)[:, -1]


@pytest.mark.parametrize("name,fp_mode", MARK_CASES, ids=[f"{n}-fp{f}" for n, f in MARK_CASES])
def test_marks_are_the_hit_set(torch_cuda, name, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    c = uu.case(name)
    tree = c["tree"]
    o, d, g = rays_of(name)
    edge = name.startswith("edge_")
    ref = None if edge else reference(name, fp_mode)     # (the gradient of the edge trees: tests/test_gpu_grad.py)
    slots = n_slots(tree)
    # bits set beforehand, on slots of internal nodes (no sample ever falls into one): the call ORs
    interior = np.flatnonzero(np.asarray(tree.child).reshape(-1) != 0)
    preset = np.zeros(slots, bool)
    preset[interior[:: max(1, interior.size // 7)]] = True
    assert preset.any()
    t = upload(name)
    try:
        touched = dev(torch, su.pack_bits(preset).view(np.int32))
        grad, touched = marked_rays(torch, t, name, fp_mode, touched=touched)
        hits = t.accumulate_weights_rays(dev(torch, o), dev(torch, d), api.RenderOptions(), want=("hits",),
                                         fp_mode=fp_mode)["hits"]
        cam = api.Camera(c["w"], c["h"], c["f"], c["f"])
        touched_f = zero_bits(torch, tree)
        grad_f = t.render_backward(cam, c["trs"], api.RenderOptions(), dev(torch, g.reshape(len(c["trs"]), c["h"], c["w"], 4)),
                                   fp_mode=fp_mode, touched=touched_f)
        hits_f = t.accumulate_weights(cam, c["trs"], api.RenderOptions(), want=("hits",), fp_mode=fp_mode)["hits"]
        torch.cuda.synchronize()
        assert t.status() == 0
        words, words_f = host_bits(touched), host_bits(touched_f)
        grad, grad_f = grad.cpu().numpy(), grad_f.cpu().numpy()
        hit = hits.cpu().numpy().reshape(-1) != 0
        hit_f = hits_f.cpu().numpy().reshape(-1) != 0
    finally:
        t.free_device()
    assert words.size == su.n_words(slots)
    marks, marks_f = su.unpack_bits(words, slots), su.unpack_bits(words_f, slots)
    assert hit.sum() > 50 and not (hit & preset).any(), "the case shows nothing"
    assert np.array_equal(marks, hit | preset), f"{int((marks != (hit | preset)).sum())} slots differ from hits > 0"
    assert np.array_equal(su.unpack_bits(words, words.size * 32)[slots:], np.zeros(words.size * 32 - slots, bool))
    assert np.array_equal(marks_f, hit_f), "frame call: marks differ from hits > 0"
    if fp_mode == 0:   # (rays_of_camera forms the directions in the strict model's order: the frame's bits)
        assert np.array_equal(marks_f, hit), "the frame call marks other slots than the ray list of its cameras"
    dd = tree.data_dim
    for what, gd, mk in (("rays", grad, marks), ("frames", grad_f, marks_f)):
        touched_elems = (gd.reshape(-1, dd) != 0).any(1)
        assert not (touched_elems & ~mk).any(), f"{what}: a non-zero gradient in an unmarked slot"
    if edge:
        cpu_hit, sigma = cpu_hit_set(name)
        assert np.array_equal(marks_f, cpu_hit), f"{int((marks_f != cpu_hit).sum())} marks differ from the hit set"
        assert np.isnan(sigma).any() and not marks_f[np.isnan(sigma)].any(), "a NaN sigma was marked"
        assert marks_f[sigma == np.inf].any(), "no +inf sigma was marked: the case shows nothing"
        assert not np.isfinite(grad_f).all(), "no non-finite record was met: the case shows nothing"
        return
    assert_parity(grad_f, ref, what=f"marked frames {name} fp{fp_mode}")
    if fp_mode == 0:
        assert_parity(grad, ref, what=f"marked rays {name}")


# ---- 2. / 3. SGD is the restatement; sparse equals dense ---------------------------------------------------------
SENTINEL = np.float32(-123.456)


@functools.lru_cache(maxsize=None)
def sgd_run(name):
    """One marked backward and one SGD step on the scene, and the dense path on a second upload -> numpy arrays."""
    import torch
    tree = uu.case(name)["tree"]
    slots, dd = n_slots(tree), tree.data_dim
    t, t2 = upload(name), upload(name)
    try:
        master = t.read_data(dtype=torch.float32)
        grad, touched = marked_rays(torch, t, name)
        torch.cuda.synchronize()
        out = dict(master0=master.cpu().numpy(), g=grad.cpu().numpy(), old16=t.read_data().cpu().numpy())
        mask = su.unpack_bits(host_bits(touched), slots)
        # the slots the step must not read or write carry a sentinel in grad
        grad.view(-1, dd)[dev(torch, ~mask)] = float(SENTINEL)
        t.step(master, grad, touched, kind="sgd", lr=LR, lr_sigma=LR_SIGMA)
        read = t.read_data()
        # the dense path: master - lr * g over the whole array, vr_tree_update_data(F32) on a second upload
        rate = np.full(dd, LR, np.float32)
        rate[-1] = LR_SIGMA
        dense = out["master0"] - rate * out["g"]
        t2.update_data(dev(torch, dense))
        read2 = t2.read_data()
        torch.cuda.synchronize()
        assert t.status() == 0
        out.update(mask=mask, master=master.cpu().numpy(), grad=grad.cpu().numpy(), words=host_bits(touched),
                   read=read.cpu().numpy(), read_dense=read2.cpu().numpy(), dense=dense)
    finally:
        t.free_device()
        t2.free_device()
    return out


@pytest.mark.parametrize("name", ["sh16", "rgba", "n3", "mixed"])
def test_sgd_is_the_restatement(torch_cuda, name):
    tree = uu.case(name)["tree"]
    r = sgd_run(name)
    mask, dd = r["mask"], tree.data_dim
    assert 50 < mask.sum() < mask.size
    assert np.array_equal(r["master0"].view(np.uint32), uu.stored(tree, tree.data).astype(np.float32).view(np.uint32))
    want = su.restate("sgd", r["master0"], r["g"], mask, lr=LR, lr_sigma=LR_SIGMA)
    assert np.array_equal(r["master"].view(np.uint32), want["master"].view(np.uint32))
    assert not np.array_equal(r["master"], r["master0"]), "the step moved nothing"
    flat0, flat1 = r["master0"].reshape(-1, dd), r["master"].reshape(-1, dd)
    assert np.array_equal(flat1[~mask].view(np.uint32), flat0[~mask].view(np.uint32))
    g = r["grad"].reshape(-1, dd)
    assert (g[mask].view(np.uint32) == 0).all(), "grad is not +0 in a touched slot"
    assert (g[~mask] == SENTINEL).all(), "grad of an untouched slot was written"
    assert not r["words"].any(), "the bitmap is not zero after the step"
    expected = uu.stored(tree, su.mixture(r["old16"], want["master"], mask))
    assert np.array_equal(r["read"].view(np.uint16), expected.view(np.uint16))
    assert not np.array_equal(r["read"].view(np.uint16), r["old16"].view(np.uint16))


@pytest.mark.parametrize("name", ["sh16", "rgba", "n3", "mixed"])
def test_sparse_equals_dense(torch_cuda, name):
    r = sgd_run(name)
    assert np.array_equal(r["read"].view(np.uint16), r["read_dense"].view(np.uint16))
    with np.errstate(over="ignore"):
        want = uu.stored(uu.case(name)["tree"], r["dense"].astype(np.float16))
    assert np.array_equal(r["read_dense"].view(np.uint16), want.view(np.uint16))


# ---- 4. the tree is a fresh upload's -----------------------------------------------------------------------------
def observe(torch, t, name, pts):
    """What has to equal a fresh upload's, as numpy: colour and accumulators of the scene's rays, the leaf weights of
    the same rays, sigma and depth at `pts` (through the lookup structure where the tree has one)."""
    from volrend_amd import api
    o, d, _ = rays_of(name)
    out = dict(t.render_rays(dev(torch, o), dev(torch, d), api.RenderOptions(), want=("rgba", "accum")))
    w = t.accumulate_weights_rays(dev(torch, o), dev(torch, d), api.RenderOptions(), want=("max_weight", "hits"))
    out.update(w)
    q = t.query(dev(torch, pts), want=("sigma", "depth"), space="tree")
    out.update({f"query_{k}": v for k, v in q.items()})
    out["read"] = t.read_data().view(torch.int16)
    torch.cuda.synchronize()
    assert t.status() == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def made_up_step(name):
    """A caller-made gradient and bitmap that take data set 1 to (nearly) data set 2 in every slot whose sigma lies on
    different sides of sigma_thresh in the two sets, and in three quarters of the others -> (master0, grad, mask,
    expected float16 data, the restatement's arrays).  Asserts, for every lookup structure an upload may pick, that
    in each kind of leaf (update_util.leaf_kinds) of which the tree has four, one rises above the threshold and
    one falls to or below it."""
    tree = uu.case(name)["tree"]
    v1, v2 = uu.variant(name, 1), uu.variant(name, 2)
    master0 = uu.stored(tree, v1).astype(np.float32)
    on1 = v1[..., -1].astype(np.float32).reshape(-1) > uu.SIGMA_THRESH
    on2 = v2[..., -1].astype(np.float32).reshape(-1) > uu.SIGMA_THRESH
    mask = (on1 != on2) | (np.arange(n_slots(tree)) % 4 != 3)
    assert 0 < (~mask).sum() and (on1 != on2).sum() > 8
    grad = np.where(mask.reshape(v1.shape[:-1])[..., None], master0 - v2.astype(np.float32), np.float32(9.0))
    want = su.restate("sgd", master0, grad, mask, lr=1.0)
    expected = su.mixture(v1, want["master"], mask)
    for top, brick in ((0, 0), (1, 1), (2, 1), (2, 3), (3, 3), (4, 3), (5, 3), (6, 3)):
        f = uu.flips(tree, top, brick, v1, expected)
        assert f and all(up > 0 and down > 0 for up, down in f.values()), (name, top, brick, f)
    return master0, grad.astype(np.float32), mask, expected, want


@pytest.mark.parametrize("name", ["mixed", "blocked", "sh16", "chain", "sh9", "sh25", "sg21", "sg22"])
def test_the_tree_is_a_fresh_uploads(torch_cuda, name):
    torch = torch_cuda
    tree = uu.case(name)["tree"]
    v1 = uu.variant(name, 1)
    master0, grad, mask, expected, want = made_up_step(name)
    t = upload(name, v1)
    fresh = None
    try:
        info = t.info()
        flips = uu.flips(tree, info["top_levels"], info["brick_levels"], v1, expected)
        print(name, "flips (up, down) per kind:", flips)
        assert flips and all(up > 0 and down > 0 for up, down in flips.values()), flips
        if name in ("mixed", "blocked"):
            assert sorted(flips) == [uu.TOP, uu.BRICK, uu.WORD]
        # the centres of the leaves whose sigma crosses the threshold
        corners, sizes, depths, slots = qu.leaf_boxes(tree)
        s0 = v1.reshape(-1, tree.data_dim)[slots, -1].astype(np.float32) > uu.SIGMA_THRESH
        s1 = expected.reshape(-1, tree.data_dim)[slots, -1].astype(np.float32) > uu.SIGMA_THRESH
        crossed = np.flatnonzero(s0 != s1)[:4096]
        pts = (corners[crossed] + 0.5 * sizes[crossed, None]).astype(np.float32)
        m, g, bits = dev(torch, master0), dev(torch, grad), dev(torch, su.pack_bits(mask).view(np.int32))
        t.step(m, g, bits, kind="sgd", lr=1.0)
        got = observe(torch, t, name, pts)
        assert np.array_equal(m.cpu().numpy().view(np.uint32), want["master"].view(np.uint32))
        fresh = upload(name, expected)
        ref = observe(torch, fresh, name, pts)
    finally:
        t.free_device()
        if fresh is not None:
            fresh.free_device()
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        bad = got[k].view(np.uint8) != ref[k].view(np.uint8)
        assert not bad.any(), f"{name}: {k} differs from the fresh upload in {int(bad.sum())} of {bad.size} bytes"
    assert np.array_equal(got["read"].view(np.uint16), uu.stored(tree, expected).view(np.uint16))
    # where binary32 resolves the leaf, the query returns the leaf's new sigma
    shallow = depths[crossed] <= 16
    assert shallow.sum() >= 4
    want_sigma = expected.reshape(-1, tree.data_dim)[slots[crossed], -1].astype(np.float32)
    assert np.array_equal(got["query_sigma"][shallow].view(np.uint32), want_sigma[shallow].view(np.uint32))
    assert (got["hits"] != 0).sum() > 50


# ---- 5. Adam -----------------------------------------------------------------------------------------------------
def test_adam_three_steps(torch_cuda):
    """Steps 1..3 with a different touched set each: slots touched once keep their moments afterwards."""
    torch = torch_cuda
    name = "sh16"
    tree = uu.case(name)["tree"]
    slots, dd = n_slots(tree), tree.data_dim
    rng = np.random.default_rng(11)
    masks = [np.arange(slots) % 3 == 0, np.arange(slots) % 5 < 2, rng.random(slots) < 0.3]
    once = (masks[0].astype(int) + masks[1] + masks[2]) == 1
    assert (once & masks[0]).sum() > 10 and (masks[0] & masks[1] & masks[2]).sum() > 10
    kw = dict(lr=0.05, lr_sigma=0.5, betas=(0.9, 0.999), eps=1e-8)
    t = upload(name)
    try:
        master = t.read_data(dtype=torch.float32)
        m, v = torch.zeros_like(master), torch.zeros_like(master)
        want = dict(master=master.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy())
        old16 = t.read_data().cpu().numpy()
        touched_ever = np.zeros(slots, bool)
        for step, mask in enumerate(masks, 1):
            g = (rng.standard_normal(tree.data.shape) * 10.0 ** rng.uniform(-3, 0, tree.data.shape)).astype(np.float32)
            want = su.restate("adam", want["master"], g, mask, m=want["m"], v=want["v"], step=step, **kw)
            touched_ever |= mask
            grad, bits = dev(torch, g), dev(torch, su.pack_bits(mask).view(np.int32))
            t.step(master, grad, bits, kind="adam", m=m, v=v, step=step, **kw)
            read = t.read_data()
            torch.cuda.synchronize()
            for key, x in (("master", master), ("m", m), ("v", v)):
                assert np.array_equal(x.cpu().numpy().view(np.uint32), want[key].view(np.uint32)), (step, key)
            assert not host_bits(bits).any() and not grad.view(-1, dd)[dev(torch, mask)].any()
            expected = uu.stored(tree, su.mixture(old16, want["master"], touched_ever))
            assert np.array_equal(read.cpu().numpy().view(np.uint16), expected.view(np.uint16)), step
        assert t.status() == 0
    finally:
        t.free_device()
    assert not want["m"].reshape(-1, dd)[~touched_ever].any() and want["v"].reshape(-1, dd)[touched_ever].any()


# ---- 6. edges ----------------------------------------------------------------------------------------------------
def test_an_empty_bitmap_changes_nothing(torch_cuda):
    torch = torch_cuda
    name = "mixed"
    tree = uu.case(name)["tree"]
    rng = np.random.default_rng(2)
    t = upload(name)
    try:
        before = t.read_data().cpu().numpy()
        arrays = {k: rng.standard_normal(tree.data.shape).astype(np.float32) for k in ("master", "grad", "m", "v")}
        arrays["v"] = np.abs(arrays["v"])
        on_dev = {k: dev(torch, a) for k, a in arrays.items()}
        bits = zero_bits(torch, tree)
        for kind in ("sgd", "adam"):
            t.step(on_dev["master"], on_dev["grad"], bits, kind=kind, lr=0.1, m=on_dev["m"], v=on_dev["v"])
        after = t.read_data().cpu().numpy()
        torch.cuda.synchronize()
        for k, a in arrays.items():
            assert np.array_equal(on_dev[k].cpu().numpy().view(np.uint32), a.view(np.uint32)), k
        assert np.array_equal(before.view(np.uint16), after.view(np.uint16)) and not host_bits(bits).any()
    finally:
        t.free_device()


def test_bits_beyond_the_last_slot_are_cleared_and_ignored(torch_cuda):
    torch = torch_cuda
    name = "n3"
    tree = uu.case(name)["tree"]
    slots, dd = n_slots(tree), tree.data_dim
    assert slots % 32 != 0, "the last word is not partial"
    words = np.zeros(su.n_words(slots), np.uint32)
    words[-1] = 0xFFFFFFFF                      # the last slots of the tree, and bits that stand for no slot
    mask = su.unpack_bits(words, slots)
    assert 0 < mask.sum() < 32
    rng = np.random.default_rng(4)
    g = rng.standard_normal(tree.data.shape).astype(np.float32)
    t = upload(name)
    try:
        master = t.read_data(dtype=torch.float32)
        m0, old16 = master.cpu().numpy(), t.read_data().cpu().numpy()
        # (the arrays end where the tree ends: a step that followed a bit beyond it would write outside them)
        grad, bits = dev(torch, g), dev(torch, words.view(np.int32))
        t.step(master, grad, bits, kind="sgd", lr=LR, lr_sigma=LR_SIGMA)
        read = t.read_data().cpu().numpy()
        torch.cuda.synchronize()
        want = su.restate("sgd", m0, g, mask, lr=LR, lr_sigma=LR_SIGMA)
        assert np.array_equal(master.cpu().numpy().view(np.uint32), want["master"].view(np.uint32))
        assert np.array_equal(grad.cpu().numpy().view(np.uint32), want["grad"].view(np.uint32))
        assert not host_bits(bits).any()
        assert np.array_equal(read.view(np.uint16), uu.stored(tree, su.mixture(old16, want["master"], mask)).view(np.uint16))
    finally:
        t.free_device()


def test_a_bit_on_an_internal_slot(torch_cuda):
    """Its coefficients are stored, its sigma is ignored: what the dense update of the same array gives."""
    torch = torch_cuda
    name = "mixed"
    tree = uu.case(name)["tree"]
    slots = n_slots(tree)
    interior = np.asarray(tree.child).reshape(-1) != 0
    mask = interior.copy()
    mask[np.flatnonzero(~interior)[::9]] = True
    assert interior.sum() > 10
    rng = np.random.default_rng(6)
    g = rng.standard_normal(tree.data.shape).astype(np.float32)
    t, t2 = upload(name), upload(name)
    try:
        master = t.read_data(dtype=torch.float32)
        m0 = master.cpu().numpy()
        t.step(master, dev(torch, g), dev(torch, su.pack_bits(mask).view(np.int32)), kind="sgd", lr=LR, lr_sigma=LR_SIGMA)
        want = su.restate("sgd", m0, g, mask, lr=LR, lr_sigma=LR_SIGMA)
        t2.update_data(dev(torch, want["master"]))
        a, b = t.read_data().cpu().numpy(), t2.read_data().cpu().numpy()
        torch.cuda.synchronize()
        assert np.array_equal(master.cpu().numpy().view(np.uint32), want["master"].view(np.uint32))
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
        flat = a.reshape(slots, -1)
        assert (flat[interior, -1].view(np.uint16) == 0).all()
        assert np.array_equal(flat[interior, :-1].view(np.uint16),
                              want["master"].reshape(slots, -1)[interior, :-1].astype(np.float16).view(np.uint16))
    finally:
        t.free_device()
        t2.free_device()


def test_clone_and_quantised_upload_step_alike(torch_cuda, tmp_path):
    torch = torch_cuda
    from tests import common
    from volrend_amd import api
    name = "basis1"     # (what test_gpu_update.py uploads quantised)
    tree = uu.case(name)["tree"]
    path = str(tmp_path / "quantised.npz")
    common.write_quantised_npz(tree, path, n_retain=1, compressed=False)
    rng = np.random.default_rng(8)
    g = rng.standard_normal(tree.data.shape).astype(np.float32)
    mask = rng.random(n_slots(tree)) < 0.4
    plain = upload(name)
    trees = {"plain": plain}
    try:
        trees["clone"] = plain.clone_to(torch.cuda.current_device())
        trees["quantised"] = api.N3Tree(path)
        pts = qu.point_set(tree, 256, seed=3)
        got = {}
        for what, t in trees.items():
            master = t.read_data(dtype=torch.float32)
            bytes0 = t.info()["device_bytes"]
            t.step(master, dev(torch, g), dev(torch, su.pack_bits(mask).view(np.int32)), kind="sgd", lr=LR, lr_sigma=LR_SIGMA)
            got[what] = observe(torch, t, name, pts)
            got[what]["master"] = master.cpu().numpy()
            # the first step keeps one more table: 4 bytes per node, file node -> device node
            assert t.info()["device_bytes"] == bytes0 + 4 * tree.capacity, what
    finally:
        for t in trees.values():
            t.free_device()
    for what in ("clone", "quantised"):
        for k, v in got["plain"].items():
            assert np.array_equal(got[what][k].view(np.uint8), v.view(np.uint8)), (what, k)
    want = su.restate("sgd", uu.stored(tree, tree.data).astype(np.float32), g, mask, lr=LR, lr_sigma=LR_SIGMA)
    assert np.array_equal(got["plain"]["master"].view(np.uint32), want["master"].view(np.uint32))


# ---- 7. SparseTreeOptimizer --------------------------------------------------------------------------------------
def test_sparse_tree_optimizer(torch_cuda):
    torch = torch_cuda
    from volrend_amd import optim
    name = "sh16"
    o, d, _ = rays_of(name)
    t = upload(name)
    try:
        opt = optim.SparseTreeOptimizer(t, "sgd", lr=LR, lr_sigma=LR_SIGMA)
        od, dd_ = dev(torch, o), dev(torch, d)
        renders = []
        for it in range(2):
            accum = opt.render(od, dd_)
            renders.append(accum.cpu().numpy())
            opt.backward(od, dd_, 2.0 * (accum - 0.5))     # d/d accum of sum((accum - 0.5)^2)
            assert bool(opt.touched.any()) and bool(opt.grad.any())
            master0 = opt.master.clone()
            opt.step()
            torch.cuda.synchronize()
            assert torch.equal(t.read_data(dtype=torch.float16).view(torch.int16), opt.master.half().view(torch.int16))
            assert not bool(opt.grad.any()) and not bool(opt.touched.any())
            assert not torch.equal(master0, opt.master), it
        assert t.status() == 0 and opt.steps == 2
        assert not np.array_equal(renders[0], renders[1]), "the second render equals the first"
    finally:
        t.free_device()


def test_sparse_tree_optimizer_adam(torch_cuda):
    """Three iterations of render -> backward -> step on SH9 (two slots per wave instruction, eight idle lanes): the
    optimiser's arrays are the restatement of the gradients and marks it read, the tree is binary16(master) in every
    slot ever touched."""
    torch = torch_cuda
    from volrend_amd import optim
    name = "sh9"
    tree = uu.case(name)["tree"]
    slots = n_slots(tree)
    o, d, _ = rays_of(name)
    kw = dict(lr=0.02, lr_sigma=0.3, betas=(0.9, 0.999), eps=1e-8)
    t = upload(name)
    try:
        opt = optim.SparseTreeOptimizer(t, "adam", **kw)
        od, dd_ = dev(torch, o), dev(torch, d)
        old16 = t.read_data().cpu().numpy()
        want = dict(master=opt.master.cpu().numpy(), m=opt.m.cpu().numpy(), v=opt.v.cpu().numpy())
        assert not want["m"].any() and not want["v"].any()
        ever = np.zeros(slots, bool)
        for it in (1, 2, 3):
            accum = opt.render(od, dd_)
            opt.backward(od, dd_, 2.0 * (accum - 0.5))
            torch.cuda.synchronize()
            g, mask = opt.grad.cpu().numpy(), su.unpack_bits(host_bits(opt.touched), slots)
            assert mask.sum() > 50 and g.any()
            want = su.restate("adam", want["master"], g, mask, m=want["m"], v=want["v"], step=it, **kw)
            ever |= mask
            opt.step()
            read = t.read_data()
            torch.cuda.synchronize()
            for key, x in (("master", opt.master), ("m", opt.m), ("v", opt.v)):
                assert np.array_equal(x.cpu().numpy().view(np.uint32), want[key].view(np.uint32)), (it, key)
            assert not bool(opt.grad.any()) and not bool(opt.touched.any())
            expected = uu.stored(tree, su.mixture(old16, want["master"], ever))
            assert np.array_equal(read.cpu().numpy().view(np.uint16), expected.view(np.uint16)), it
        assert t.status() == 0 and opt.steps == 3
        assert not np.array_equal(expected.view(np.uint16), old16.view(np.uint16))
    finally:
        t.free_device()


# ---- 8. the value domain -----------------------------------------------------------------------------------------
def frame(torch, t, name, pose=0):
    """One frame of the scene through the camera path (ray generation with the block cull at its default)."""
    from volrend_amd import api
    c = uu.case(name)
    cam = api.Camera(c["w"], c["h"], c["f"], c["f"])
    cam.transform = c["trs"][pose]
    img = torch.zeros((c["h"], c["w"], 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((c["h"], c["w"], 4), dtype=torch.float32, device="cuda")
    api.launch_renderer(t, cam, api.RenderOptions(), img, None, torch.cuda.current_stream(), True, accum=acc)
    torch.cuda.synchronize()
    return img.cpu().numpy(), acc.cpu().numpy()


@pytest.mark.parametrize("call_name", list(su.CALLS))
@pytest.mark.parametrize("name", su.CATALOGUE_SCENES)
def test_value_domain(torch_cuda, name, call_name):
    """One call over the catalogue of step_util.catalogue (what it holds and what it shows: tests/test_step_host.py):
    subnormal, overflowing and non-finite gradients and moments, eps = 0, extreme betas, step counts and rates,
    master on binary16 ties, subnormals and overflow.  Everything that is not NaN is bit-exact against the
    restatement; NaN stands in exactly the same elements, in binary32 and in the binary16 the tree holds, and leaks
    into no other element.  Then the tree is a fresh upload's of that data, byte for byte in every output -- the
    fresh upload takes the tree's own NaN bits, since the header leaves a NaN's sign and payload open -- and for SH16
    its frame is the oracle's: sigma has become NaN, +-inf, negative, -0 and subnormal in marked leaves and has
    crossed sigma_thresh both ways, so lookup refresh and block-cull occupancy have to follow."""
    torch = torch_cuda
    from tests import common
    c, call = su.catalogue(name), su.CALLS[call_name]
    tree = uu.case(name)["tree"]
    mask = c["mask"]
    want, expected16 = su.catalogue_expected(name, call_name)
    found = su.sigma_outcomes(name, expected16)
    need = su.SIGMA_OUTCOMES if su.passes_through(call) else ("rises", "falls", "nan")
    assert all(found[k] > 0 for k in need), found
    corners, sizes, _, slots = qu.leaf_boxes(tree)
    cat_leaves = np.isin(slots, np.concatenate(list(c["sigma"].values())))
    pts = (corners[cat_leaves] + 0.5 * sizes[cat_leaves, None]).astype(np.float32)
    assert len(pts) == len(su.entries()) * su.SIGMA_COPIES
    t = upload(name, c["old16"])
    fresh = None
    try:
        before = frame(torch, t, name)[0]
        got = su.device_call(torch, t, call["kind"], c, mask, su.pack_bits(mask), **su.call_kw(call))
        stored16 = uu.stored(tree, expected16)
        su.assert_call(got, want, mask, stored16, f"{name} {call_name}", nan_ok=True)
        assert np.isnan(want["master"]).any() and np.isinf(want["master"]).any()
        obs = observe(torch, t, name, pts)
        obs["frame_rgba"], obs["frame_accum"] = frame(torch, t, name)
        assert t.status() == 0
        nan16 = np.isnan(stored16)
        fresh = upload(name, np.where(nan16, got["read"], stored16))
        ref = observe(torch, fresh, name, pts)
        ref["frame_rgba"], ref["frame_accum"] = frame(torch, fresh, name)
    finally:
        t.free_device()
        if fresh is not None:
            fresh.free_device()
    for k in ref:
        assert obs[k].dtype == ref[k].dtype and obs[k].shape == ref[k].shape, k
        bad = obs[k].view(np.uint8) != ref[k].view(np.uint8)
        assert not bad.any(), (f"{name} {call_name}: {k} differs from the fresh upload in {int(bad.sum())} of "
                               f"{bad.size} bytes")
    assert (obs["hits"] != 0).sum() > 50
    assert not np.array_equal(obs["frame_rgba"], before), "the step changed nothing in the frame"
    if name == "sh16":
        sc = uu.case(name)
        rgba_o, acc_o, cnt = common.oracle_frame(uu.with_data(tree, expected16), sc["trs"][0], sc["w"], sc["h"], sc["f"],
                                                 0)
        assert cnt["hit_samples"] > 0
        common.assert_same_values(obs["frame_rgba"], obs["frame_accum"], rgba_o, acc_o,
                                  f"{name} {call_name} against the oracle")
