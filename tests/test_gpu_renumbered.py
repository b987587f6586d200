"""-m gpu: every call that speaks the file's node numbering, on trees whose numbering is not breadth-first and whose
arrays hold nodes the root does not reach (common.renumbered: backward links, a pruned subtree left in the middle of
the array, zero slack and linked, bright slack behind it), under default tuning and under forced lookup shapes.

The expected side is an independent reference -- the oracle, the C restatements of the march, the float64 gradient,
the numpy restatements of the step, the geometry, refine and collapse -- evaluated on the renumbered tree itself or, for
the gradient, on the pruned original and carried through new_of.  Everything is bit-exact but the gradient sums,
which keep grad_util.K.  The bright orphans (sigma 200, coefficients 3.0) change a pixel, a weight or a gradient of any
kernel that reaches them; sentinel buffers show a store into their slots."""
import dataclasses
import functools

import numpy as np
import pytest

from tests import collapse_util as cu
from tests import common
from tests import fit_util as fu
from tests import geometry_util as gg
from tests import grad_util as gu
from tests import query_util as qu
from tests import refine_util as ru
from tests import renumber_util as rn
from tests import step_util as su
from tests import update_util as uu
from tests import weights_util as wu
from tests.common import ob

pytestmark = pytest.mark.gpu
FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
SCENES = sorted(rn.SCENES)
ALONE = [("sh9", (k,)) for k in common.RENUMBER_KINDS]
COMBINED = [(s, rn.COMBINED) for s in SCENES]


def ids(cases):
    return [f"{s}-{'+'.join(k)}" for s, k in cases]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def frames(torch, t, fp_mode=0):
    """Both poses of rn.views() -> (rgba uint8 [2, h, w, 4], accum float32 [2, h, w, 4])."""
    from volrend_amd import api
    trs, w, h, f = rn.views()
    img = torch.zeros((len(trs), h, w, 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((len(trs), h, w, 4), dtype=torch.float32, device="cuda")
    cam = api.Camera(w, h, f, f)
    for i, tr in enumerate(trs):
        cam.transform = np.asarray(tr, np.float32)
        api.launch_renderer(t, cam, api.RenderOptions(), img[i], None, torch.cuda.current_stream(), True, accum=acc[i],
                            fp_mode=fp_mode)
    torch.cuda.synchronize()
    return img.cpu().numpy(), acc.cpu().numpy()


def oracle_frames(tree, fp_mode=0, **opt_kw):
    trs, w, h, f = rn.views()
    out = [common.oracle_frame(tree, tr, w, h, f, fp_mode, **opt_kw) for tr in trs]
    assert all(o[2]["hit_samples"] > 0 for o in out)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def assert_frames(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: RGBA8 differs in {int((got[0] != want[0]).any(-1).sum())} pixels"
    assert got[1].tobytes() == want[1].tobytes(), f"{what}: accumulators differ"


def weights(torch, t, tree, fp_mode=0):
    """Leaf weights of both poses into sentinel buffers -> (max_weight, hits) as numpy."""
    trs, w, h, f = rn.views()
    mw, hc = wu.accumulate(torch, t, w, h, f, trs, fp_mode, tree=tree)
    torch.cuda.synchronize()
    return wu.host(mw), wu.host(hc)


def bits16(x):
    import torch
    return x.view(torch.int16).cpu().numpy().view(np.uint16)


def slot_mask(nodes, N3):
    return np.repeat(np.asarray(nodes, bool), N3)


# ---- 1. render ------------------------------------------------------------------------------------------
@FP
@pytest.mark.parametrize("scene,kinds", ALONE + COMBINED, ids=ids(ALONE + COMBINED))
def test_frames_are_the_oracles(torch_cuda, scene, kinds, fp_mode):
    c = rn.case(scene, kinds)
    t = rn.upload(c)
    try:
        got = frames(torch_cuda, t, fp_mode)
        assert t.status() == 0
    finally:
        t.free_device()
    assert_frames(got, oracle_frames(c["tree"], fp_mode), f"{scene} {kinds} fp{fp_mode}")


@pytest.mark.parametrize("scene", rn.LOOKUP_SCENES)
def test_orphans_stay_out_of_the_occupancy_and_the_lead_in(torch_cuda, scene):
    """The block cull and the lead-in march see the pruned original: no block less culled, no ray more entered, no
    sample more marched for the bright nodes the root does not reach."""
    c = rn.case(scene, rn.COMBINED)
    stats = []
    for tree in (c["tree"], c["orig"]):
        t = rn.upload(c, tree)
        try:
            t.set_tuning(head_march=1, block_cull=1, head_min_lanes=1, head_max=1 << 20)
            t.cull_stats(reset=True)
            t.head_stats(reset=True)
            got = frames(torch_cuda, t)
            assert t.status() == 0
            stats.append((t.cull_stats(), t.head_stats()))
        finally:
            t.free_device()
        assert_frames(got, oracle_frames(tree), scene)
    assert stats[0] == stats[1], stats
    assert stats[0][0]["culled"] > 0 and stats[0][1]["samples"] > 0, stats[0]


# ---- 2. leaf weights ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight_reference(scene, fp_mode):
    c = rn.case(scene, rn.COMBINED)
    trs, w, h, f = rn.views()
    mw, hc, _ = wu.restate(c["tree"], trs, w, h, f, fp_mode)
    return mw, hc


@FP
@pytest.mark.parametrize("scene", SCENES)
def test_leaf_weights_of_frames_and_of_a_ray_list(torch_cuda, scene, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    want_mw, want_hc = weight_reference(scene, fp_mode)
    assert (want_hc > 0).sum() >= 100
    exp_mw, exp_hc = wu.expected(want_mw, want_hc)
    trs, w, h, f = rn.views()
    o, d = fu.camera_rays(trs, w, h, f, fp_mode)
    t = rn.upload(c)
    try:
        got_mw, got_hc = weights(torch, t, tree, fp_mode)
        mw, hc = wu.buffers(torch, tree)
        t.accumulate_weights_rays(fu.dev(torch, o), fu.dev(torch, d), api.RenderOptions(), max_weight=mw, hits=hc, want=(),
                                  fp_mode=fp_mode)
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    for what, a, b in (("frames", got_mw, got_hc), ("ray list", wu.host(mw), wu.host(hc))):
        wu.assert_same_slots(a, b, exp_mw, exp_hc, f"{scene} {what}")
        assert (wu.bits(a[c["orphan"]]) == wu.bits(wu.SENT_W)).all(), f"{what}: a weight of an orphan slot was written"
        assert (b[c["orphan"]].view(np.uint32) == wu.SENT_H).all(), f"{what}: a count of an orphan slot was written"


# ---- 3. backward, marked backward, fit --------------------------------------------------------------------
GRAD_SCENES = ["sh9", "mixed", "rgba", "n3"]


def carried(c, ref):
    """grad_util.reference's dict of the pruned original in the numbering of the renumbered tree: rows moved by
    new_of, rows of orphans zero (M == 0 there: assert_parity asks for the sentinel's bits)."""
    tree, new_of = c["tree"], c["new_of"]
    assert ref["tree"].child.tobytes() == c["orig"].child.tobytes() and ref["tree"].data.tobytes() == c["orig"].data.tobytes()
    moved = {k: rn.carry(ref[k], new_of, tree.capacity) for k in ("grad", "mag", "under")}
    assert not any(moved[k][c["orphan"]].any() for k in moved)
    return dict(ref, tree=tree, **moved)


def carried_marks(c, ref, rays=None):
    hit = rn.carry_slots(gu.hit_slots(ref, rays), c["new_of"], c["tree"].capacity, c["tree"].N ** 3, False)
    assert hit.sum() >= 100 and not hit[slot_mask(c["orphan"], c["tree"].N ** 3)].any()
    return gu.mark_words(hit)


@FP
@pytest.mark.parametrize("scene", GRAD_SCENES)
def test_backward_and_its_marks(torch_cuda, scene, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    ref0 = gu.reference("renum_" + scene, "default", fp_mode, 2, rn.SIZE)
    ref = carried(c, ref0)
    assert (ref["mag"] > 0).sum() > 200, "the case shows nothing"
    start = gu.sentinel(ref["grad"].shape)
    cam = api.Camera(ref["w"], ref["h"], ref["f"], ref["f"])
    g = fu.dev(torch, ref["g"])
    t = rn.upload(c)
    try:
        plain = t.render_backward(cam, ref["trs"], api.RenderOptions(), g, grad_data=fu.dev(torch, start), fp_mode=fp_mode)
        touched = fu.zero_bits(torch, tree)
        marked = t.render_backward(cam, ref["trs"], api.RenderOptions(), g, grad_data=fu.dev(torch, start),
                                   fp_mode=fp_mode, touched=touched)
        torch.cuda.synchronize()
        assert t.status() == 0
        plain, marked, touched = plain.cpu().numpy(), marked.cpu().numpy(), touched.cpu().numpy().view(np.uint32)
    finally:
        t.free_device()
    gu.assert_parity(plain, ref, start=start, what=f"{scene} fp{fp_mode} backward")
    gu.assert_parity(marked, ref, start=start, what=f"{scene} fp{fp_mode} marked backward")
    assert np.array_equal(touched, carried_marks(c, ref0)), "touched is not the set of hit slots"
    orphan = slot_mask(c["orphan"], tree.N ** 3)
    for got in (plain, marked):
        same = (got.view(np.uint32) == start.view(np.uint32)).reshape(orphan.size, -1)
        assert same[orphan].all(), "an element of an orphan slot was written"


@FP
@pytest.mark.parametrize("scene", GRAD_SCENES)
def test_fit_rays(torch_cuda, scene, fp_mode):
    """The fused loss and backward over the rays of both frames: accum is the oracle's frame, sq_err the numpy head on
    it, the gradient the float64 one for the head's g, the marks the hit slots."""
    torch = torch_cuda
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    ref0 = gu.reference("renum_" + scene, "default", fp_mode, 2, rn.SIZE)
    o, d = fu.camera_rays(ref0["trs"], ref0["w"], ref0["h"], ref0["f"], fp_mode)
    n = len(o)
    target, grad_scale = fu.targets(n, 40 + len(scene)), 2.0 / (3 * n)
    accum = oracle_frames(tree, fp_mode, background_brightness=fu.BG)[1].reshape(n, 4)
    want = fu.head(accum, target, fu.BG, grad_scale)
    ref = carried(c, fu.reference_for(ref0, want["g"]))
    start = gu.sentinel(ref["grad"].shape)
    t = rn.upload(c)
    try:
        res, touched = fu.fit(torch, t, ref, o, d, target, fp_mode, grad_scale, start=start)
        torch.cuda.synchronize()
        assert t.status() == 0
        res = {k: v.cpu().numpy() for k, v in res.items()}
        touched = touched.cpu().numpy().view(np.uint32)
    finally:
        t.free_device()
    assert fu.bits(res["accum"]).tobytes() == fu.bits(accum).tobytes(), "accum is not the oracle's frame"
    assert fu.bits(res["sq_err"]).tobytes() == fu.bits(want["sq_err"]).tobytes(), "sq_err is not the numpy head's"
    gu.assert_parity(res["grad_data"], ref, start=start, what=f"{scene} fp{fp_mode} fit")
    assert np.array_equal(touched, carried_marks(c, ref0))
    orphan = slot_mask(c["orphan"], tree.N ** 3)
    same = (res["grad_data"].view(np.uint32) == start.view(np.uint32)).reshape(orphan.size, -1)
    assert same[orphan].all(), "an element of an orphan slot was written"


# ---- 4. read-back, update, step ---------------------------------------------------------------------------
def read_both(torch, t):
    h, f = t.read_data(), t.read_data(dtype=torch.float32)
    torch.cuda.synchronize()
    return bits16(h), f.cpu().numpy()


def leaf_of_a_link_that_leaves(tree):
    """bool [capacity, N^3]: the slots whose link points outside [1, capacity)."""
    rows = common.rows_of(tree)
    target = np.arange(tree.capacity)[:, None] + rows
    return (rows != 0) & ((target < 1) | (target >= tree.capacity))


@pytest.mark.parametrize("scene", SCENES)
def test_read_back_is_the_file(torch_cuda, scene):
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    want = uu.stored(tree, tree.data)
    out = leaf_of_a_link_that_leaves(tree).reshape(tree.child.shape)
    assert out.sum() == 1 and (want[out][:, -1] == common.BRIGHT_SIGMA).all()     # a leaf to the upload: its sigma
    orphan = c["orphan"]
    assert want[orphan].any() and (want[orphan][..., -1] == 0).sum() >= 2         # values, and internal slots among them
    t = rn.upload(c)
    try:
        h, f = read_both(torch_cuda, t)
    finally:
        t.free_device()
    assert h.shape == f.shape == tree.data.shape
    assert np.array_equal(h, want.view(np.uint16))
    assert np.array_equal(f.view(np.uint32), want.astype(np.float32).view(np.uint32))


def data_sets(scene):
    tree = rn.case(scene, rn.COMBINED)["tree"]
    return tuple(uu.variant_of(tree, which, 5000 * which + len(scene)) for which in (1, 2))


def observe(torch, t, c, tree):
    """Every output an update has to carry, as numpy: frames and leaf weights in both FP modes, a grid query, the
    read-back."""
    out = {}
    for fp in (0, 1):
        out[f"rgba{fp}"], out[f"accum{fp}"] = frames(torch, t, fp)
        out[f"max_weight{fp}"], out[f"hits{fp}"] = weights(torch, t, tree, fp)
    res = 32
    q = t.query_grid((0, 0, 0), (1, 1, 1), (res, res, res), want=("sigma", "depth", "coeffs"), space="tree")
    out.update({f"grid_{k}": v.cpu().numpy() for k, v in q.items()})
    out["read"], out["read32"] = read_both(torch, t)
    assert t.status() == 0
    return out


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = got[k].view(np.uint8) != want[k].view(np.uint8)
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} bytes"


UPDATE_DTYPE = {"sh9": "f16", "mixed": "f32", "blocked": "f16", "rgba": "f32", "n3": "f16"}


@pytest.mark.parametrize("scene", SCENES)
def test_update_equals_a_fresh_upload(torch_cuda, scene):
    torch = torch_cuda
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    v1, v2 = data_sets(scene)
    orphan = c["orphan"]
    assert (v1[orphan].view(np.uint16) != v2[orphan].view(np.uint16)).mean() > 0.9       # other orphan values
    fresh = rn.upload(c, uu.with_data(tree, v2))
    try:
        want = observe(torch, fresh, c, tree)
    finally:
        fresh.free_device()
    t = rn.upload(c, uu.with_data(tree, v1))
    try:
        if scene in rn.LOOKUP_SCENES:
            info = t.info()
            f = uu.flips(tree, info["top_levels"], info["brick_levels"], v1, v2)
            assert uu.TOP in f and uu.BRICK in f and all(up > 0 and down > 0 for up, down in f.values()), f
        first = frames(torch, t)
        t.update_data(uu.dev(torch, v2, torch.float32 if UPDATE_DTYPE[scene] == "f32" else None))
        got = observe(torch, t, c, tree)
    finally:
        t.free_device()
    assert_same(got, want, f"{scene} {UPDATE_DTYPE[scene]}")
    assert np.array_equal(got["read"], uu.stored(tree, v2).view(np.uint16))
    assert not np.array_equal(first[0], got["rgba0"]), "the two data sets render the same frames"
    for fp in (0, 1):
        assert_frames((got[f"rgba{fp}"], got[f"accum{fp}"]), oracle_frames(uu.with_data(tree, v2), fp), f"{scene} fp{fp}")


def step_case(scene):
    """-> dict(old16, master, grad, m, v, mask): the arrays of a step on the combined tree of `scene`.  The mask sets
    half the reachable leaves, some internal slots, slots of the slack nodes and slots of the pruned subtree."""
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    N3, shape = tree.N ** 3, tree.data.shape
    rng = np.random.default_rng(4200 + len(scene))
    rows = common.rows_of(tree)
    orphan = slot_mask(c["orphan"], N3)
    internal = rows.reshape(-1) != 0
    mask = (rng.random(orphan.size) < 0.5) & ~internal & ~orphan
    mask[np.flatnonzero(internal & ~orphan)[::29]] = True
    slack = slot_mask(np.arange(tree.capacity) >= tree.capacity - 5, N3)
    mask[np.flatnonzero(slack)[::3]] = True                          # leaves, the linking slots, the link that leaves
    mask[np.flatnonzero(orphan & ~slack)[::2]] = True                # the pruned subtree, leaves and links
    groups = {"leaves": ~internal & ~orphan, "internal": internal & ~orphan, "slack": slack, "pruned": orphan & ~slack,
              "orphan links": orphan & internal}
    assert all((mask & g).sum() >= 2 and (~mask & g).sum() >= 2 for g in groups.values()), \
        {k: int((mask & g).sum()) for k, g in groups.items()}
    old16 = data_sets(scene)[0]
    return dict(old16=old16, master=uu.stored(tree, old16).astype(np.float32), mask=mask,
                grad=(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 0, shape)).astype(np.float32),
                m=(rng.standard_normal(shape) * 0.1).astype(np.float32),
                v=((rng.standard_normal(shape) * 0.1) ** 2).astype(np.float32))


@pytest.mark.parametrize("call", ["sgd", "adam"])
@pytest.mark.parametrize("scene", SCENES)
def test_step(torch_cuda, scene, call):
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    s = step_case(scene)
    kw = dict(lr=1e-2, lr_sigma=0.5) if call == "sgd" else dict(lr=1e-2, lr_sigma=0.5, betas=(0.9, 0.999), eps=1e-8, step=3)
    adam = call == "adam"
    want = su.restate(call, s["master"], s["grad"], s["mask"], m=s["m"] if adam else None, v=s["v"] if adam else None, **kw)
    expected16 = uu.stored(tree, su.mixture(s["old16"], want["master"], s["mask"]))
    assert (expected16.view(np.uint16) != uu.stored(tree, s["old16"]).view(np.uint16)).reshape(s["mask"].size, -1)[
        s["mask"]].any(1).mean() > 0.9, "the step changes too few marked slots"
    t = rn.upload(c, uu.with_data(tree, s["old16"]))
    try:
        got = su.device_call(torch_cuda, t, call, s, s["mask"], su.pack_bits(s["mask"]), **kw)
        assert t.status() == 0
        after = frames(torch_cuda, t)
    finally:
        t.free_device()
    su.assert_call(got, want, s["mask"], expected16, f"{scene} {call}")
    assert_frames(after, oracle_frames(uu.with_data(tree, expected16)), f"{scene} {call}: the stepped tree")


# ---- 5. queries, geometry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
def test_point_queries(torch_cuda, scene):
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    pts = qu.point_set(tree, 20_000, 700 + len(scene))
    th = ob.TreeHandle(tree)
    ans = qu.oracle_answers(tree, th, pts, "tree")
    assert (ans["sigma"] > 0).mean() >= 0.25
    assert not c["orphan"][ans["leaf"] // tree.N ** 3].any()
    t = rn.upload(c)
    try:
        qu.check_against_oracle(torch_cuda, t, tree, th, pts, "tree", scene, ans)
        qu.check_against_oracle(torch_cuda, t, tree, th, qu.to_world(tree, pts), "world", scene)
    finally:
        t.free_device()


@pytest.mark.parametrize("scene", SCENES)
def test_geometry_and_the_way_back_from_a_slot(torch_cuda, scene):
    """vr_tree_geometry of the raw kinds against its restatement and the top-down walk; on the power-of-two scenes
    the centre of every reachable leaf's cell, queried in tree space, is answered with that leaf's own record."""
    torch = torch_cuda
    c = rn.case(scene, rn.RAW)
    tree = gg.distinct_records(c["tree"])
    rows = common.rows_of(tree).astype(np.int32)
    N3 = rows.shape[1]
    parent, depth, origin = gg.restate(rows)
    down = gg.walk_down(rows)
    assert np.array_equal(depth >= 0, ~c["orphan"]) and set(down) == set(np.flatnonzero(~c["orphan"]).tolist())
    assert ((depth < 0) & (parent >= 0)).sum() >= 7                   # the pruned subtree: linked, without a depth
    t = rn.upload(c, tree)
    try:
        geo = t.geometry()
        got = {k: v.cpu().numpy() for k, v in geo.items()}
        assert np.array_equal(got["parent_slot"], parent) and np.array_equal(got["node_depth"], depth)
        assert np.array_equal(got["node_origin"].view(np.uint32)[depth >= 0], origin[depth >= 0])
        for m, (p, d, o) in down.items():
            assert (got["parent_slot"][m], got["node_depth"][m]) == (p, d) and tuple(got["node_origin"][m].view(np.uint32)) == o
        leaves = gg.reachable_leaves(rows, depth)
        res = t.slot_points(fu.dev(torch, leaves), geometry=geo)
        q = t.query(res["points"].reshape(-1, 3), want=("depth", "sigma", "coeffs"), space="tree")
        torch.cuda.synchronize()
        want_pts = gg.points(depth, origin, tree.N, leaves)
        assert res["points"].cpu().numpy().tobytes() == want_pts[0].tobytes()
        assert np.array_equal(res["depth"].cpu().numpy(), want_pts[1])
        if scene in rn.POWER_OF_TWO:
            records = tree.data.reshape(-1, tree.data_dim)
            assert np.array_equal(q["depth"].cpu().numpy(), depth[leaves // N3])
            assert q["sigma"].cpu().numpy().tobytes() == records[leaves, -1].astype(np.float32).tobytes()
            assert q["coeffs"].cpu().numpy().tobytes() == records[leaves, :-1].astype(np.float32).tobytes()
    finally:
        t.free_device()


# ---- 6. quantised upload, clone ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["sh9", "mixed", "n3"])
def test_quantised_upload(torch_cuda, scene, tmp_path):
    from volrend_amd import _tree, api
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    path = str(tmp_path / "renumbered.npz")
    common.write_quantised_npz(tree, path, n_retain=1, compressed=False)
    z = np.load(path)
    a = _tree._quant_arrays(z, z["child"])
    decoded = _tree._decode_arrays(a["quant_colors"], a["quant_map"], a["sigma"], a["data_retained"], tree.data_dim)
    decoded = decoded.reshape(tree.data.shape)
    assert decoded.tobytes() == tree.data.tobytes()                  # (the codebooks are exact)
    if c["tuning"]:
        api.set_tuning(**c["tuning"])
    try:
        t = api.N3Tree(path)
    finally:
        if c["tuning"]:
            api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    try:
        assert t.data_ is None and t.quant_ is not None              # decoded on the device
        h, _ = read_both(torch_cuda, t)
        got = frames(torch_cuda, t)
        assert t.status() == 0
    finally:
        t.free_device()
    assert np.array_equal(h, uu.stored(tree, decoded).view(np.uint16))
    assert_frames(got, oracle_frames(tree), f"{scene} quantised")


@pytest.mark.parametrize("scene", ["sh9", "blocked", "n3"])
def test_clone(torch_cuda, scene):
    torch = torch_cuda
    c = rn.case(scene, rn.COMBINED)
    tree = c["tree"]
    t = rn.upload(c)
    clone = None
    try:
        clone = t.clone_to(torch.cuda.current_device())
        want = (frames(torch, t), weights(torch, t, tree), read_both(torch, t))
        got = (frames(torch, clone), weights(torch, clone, tree), read_both(torch, clone))
        assert t.status() == 0 and clone.status() == 0
    finally:
        t.free_device()
        if clone is not None:
            clone.free_device()
    for g, w in zip(got, want):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g, w))
    assert_frames(got[0], oracle_frames(tree), f"{scene} clone")
    assert np.array_equal(got[2][0], uu.stored(tree, tree.data).view(np.uint16))


# ---- 7. refine, collapse, save ----------------------------------------------------------------------------
def collapsed_tree(tree, want):
    """The SynthTree of a collapse restatement (values under MEAN)."""
    cap, N, dd = want["n_keep"], tree.N, tree.data_dim
    return dataclasses.replace(tree, child=want["child_out"].reshape(cap, N, N, N),
                               data=want["dsts"][0].view(np.float16).reshape(cap, N, N, N, dd))


@pytest.mark.parametrize("scene", ["sh9", "n3"])
def test_refine(torch_cuda, scene):
    torch = torch_cuda
    c = rn.case(scene, rn.RAW)
    tree = c["tree"]
    rows = common.rows_of(tree).astype(np.int32)
    dd = tree.data_dim
    sel = ru.selections(rows, seed=3)["random30"]
    assert sel[slot_mask(c["orphan"], rows.shape[1])].any()                        # orphan leaves are refined too
    comp = ru.companions(rows.size, dd, seed=11)
    data = uu.stored(tree, tree.data).reshape(-1, dd).view(np.uint16)
    want_child, want_slots, want_dsts = ru.restate(rows, sel, [(data, ru.COPY), comp[1], comp[2]])
    t = rn.upload(c)
    new = None
    try:
        res = t.refine(fu.dev(torch, sel), [(fu.dev(torch, comp[1][0].view(np.int32)), "copy"),
                                            (fu.dev(torch, comp[2][0].view(np.int32)), "zero")])
        new = res["tree"]
        assert res["n_new"] == want_slots.size > 0
        assert np.array_equal(new.child_.reshape(-1, rows.shape[1]), want_child)
        assert np.array_equal(res["src_slot"].cpu().numpy(), want_slots)
        shape = (want_child.shape[0], tree.N, tree.N, tree.N)
        refined = dataclasses.replace(tree, child=want_child.reshape(shape),
                                      data=want_dsts[0].view(np.float16).reshape(shape + (dd,)))
        # (a refined slot is an internal slot of the new tree: its sigma reads back as +0)
        assert np.array_equal(bits16(new.read_data()), uu.stored(refined, refined.data).view(np.uint16))
        for g, w in zip(res["companions"], want_dsts[1:]):
            assert np.array_equal(g.cpu().numpy().view(np.uint32).reshape(w.shape), w)
        got = frames(torch, new)
        assert new.status() == 0
    finally:
        t.free_device()
        if new is not None:
            new.free_device()
    assert_frames(got, oracle_frames(ru.refined_synth(tree, sel)[0]), f"{scene} refined")


@pytest.mark.parametrize("scene", ["sh9", "n3"])
def test_collapse(torch_cuda, scene):
    torch = torch_cuda
    c = rn.case(scene, rn.RAW)
    tree = c["tree"]
    rows = common.rows_of(tree).astype(np.int32)
    dd, N3 = tree.data_dim, rows.shape[1]
    sel = cu.selections(rows, seed=4)["random50"]
    keep = cu.bit_companions(rows.size, dd, seed=12)[1]                 # binary32 bits, KEEP
    mean = cu.mean_companions(rows.size, dd, seed=12)[1]                # binary32 values, MEAN
    data = uu.stored(tree, tree.data).reshape(-1, dd).view(np.uint16)
    want = cu.restate(rows, sel, [(data, cu.MEAN), keep, mean])
    assert (want["child_out"] < 0).any() and 0 < want["n_keep"] < tree.capacity
    assert want["collapsed"][c["orphan"]].any() and want["collapsed"][~c["orphan"]].any()
    t = rn.upload(c)
    new = None
    try:
        res = t.collapse(fu.dev(torch, sel), [(fu.dev(torch, keep[0].view(np.int32)), "keep"),
                                              (fu.dev(torch, mean[0].view(np.float32)), "mean")], values="mean")
        new = res["tree"]
        assert res["n_keep"] == want["n_keep"]
        assert np.array_equal(new.child_.reshape(-1, N3), want["child_out"])
        for key in ("node_map", "src_node", "into_slot"):
            assert np.array_equal(res[key].cpu().numpy(), want[key]), key
        got_arrays = [bits16(new.read_data()).reshape(-1, dd)] + [g.cpu().numpy().view(np.uint32).reshape(-1, dd)
                                                                  for g in res["companions"]]
        got = frames(torch, new)
        assert new.status() == 0
    finally:
        t.free_device()
        if new is not None:
            new.free_device()
    stored_new = uu.stored(collapsed_tree(tree, want), want["dsts"][0].view(np.float16).reshape(-1, tree.N, tree.N, tree.N, dd))
    cu.assert_array(got_arrays[0], stored_new.reshape(-1, dd).view(np.uint16), cu.MEAN, want["into_slot"], "data")
    cu.assert_array(got_arrays[1], want["dsts"][1].view(np.uint32), cu.KEEP, want["into_slot"], "keep")
    cu.assert_array(got_arrays[2], want["dsts"][2].view(np.uint32), cu.MEAN, want["into_slot"], "mean")
    assert_frames(got, oracle_frames(collapsed_tree(tree, want)), f"{scene} collapsed")


@pytest.mark.parametrize("scene", ["sh9", "n3"])
def test_save_writes_one_parent_depth(torch_cuda, scene, tmp_path):
    """save() of the tree on the device (vr_tree_geometry) and off it (the host walk) write the same parent_depth."""
    from volrend_amd import api
    tree = rn.case(scene, rn.RAW)["tree"]
    a, b = str(tmp_path / "loaded.npz"), str(tmp_path / "unloaded.npz")
    t = api.N3Tree.from_synth(tree)
    try:
        t.save(a)
    finally:
        t.free_device()
    api.N3Tree.from_synth(tree, upload=False).save(b)
    za, zb = np.load(a), np.load(b)
    parent, depth, _ = gg.restate(common.rows_of(tree))
    want = np.stack([parent, depth], axis=1)
    want[0] = 0
    assert np.array_equal(za["parent_depth"], want) and np.array_equal(zb["parent_depth"], want)
    assert sorted(za.files) == sorted(zb.files) and all(za[k].tobytes() == zb[k].tobytes() for k in za.files)
