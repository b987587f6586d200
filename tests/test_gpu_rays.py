"""Ray lists on the GPU: vr_render_rays, vr_accumulate_weights_rays, vr_render_backward_rays, vr_reserve_rays
and volrend_amd.optim.

The yardsticks are the existing ones, untouched (tests/rays_util.py, pinned by tests/test_rays_restatement.py):
  arbitrary rays, colour       every ray through the oracle as its own 2 x 2 camera: RGBA8 and accumulators bit
                               for bit, both FP models, no ray left out;
  camera-derived rays          whole frames of the oracle / the leaf-weight restatement / the float64 gradient of
                               the same views: strict model any pose, FMA model signed-permutation poses (whose
                               matrix product is exact fused or not; odd image sizes, so 95 x 95 where the strict
                               cases use 96 x 96).
Every run ends with status() == 0."""
import functools

import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import grad_util as gu
from tests import rays_util as ru
from tests import weights_util as wu
from tests.grad_util import assert_contained, assert_parity, sentinel, upload_edge
from tests.weights_util import SENT_W, expected

pytestmark = pytest.mark.gpu
FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
SIZES = [1, 63, 64, 65, 1000, 1025, 8200, None]          # None = every ray of the three frames
SIZE_IDS = [str(n) if n else "3frames" for n in SIZES]
PERM_POSES = [ru.permutation_pose(),
              ru.permutation_pose((2, 0, 1), (1, 1, 1), (0.2, 3.4, 0.1)),
              ru.permutation_pose((0, 1, 2), (1, -1, -1), (0.1, -0.2, -3.4))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def tree_named(name):
    """-> (tree, ndc): the trees of grad_util.tree_of, plus one SG tree."""
    if name == "sg":
        return common.small_scene(depth=4, basis_dim=9, fmt="SG", seed=2), None
    tree, _, ndc = gu.tree_of(name)
    return tree, ndc


def upload(name):
    from volrend_amd import api
    tree, ndc = tree_named(name)
    blocked = name == "blocked"
    if blocked:
        api.set_tuning(top_levels=2, brick_levels=3, brick_blocked=1)
    try:
        t = api.N3Tree.from_synth(tree, ndc=ndc)
    finally:
        if blocked:
            api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    if blocked:
        assert t.info()["brick_blocked"] == 1
    return t


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the references are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def views(fp_mode, n_poses=3):
    """-> (transforms, size, focal): orbit poses at 96 x 96 (strict), permutation poses at 95 x 95 (FMA)."""
    if fp_mode == 0:
        return gu.poses(n_poses, size=96), 96, common.camera_for(size=96)[3]
    return PERM_POSES[:n_poses], 95, 112.0


def camera_rays(trs, w, h, fx, fy=None):
    """The rays of every pixel of every view, frame after frame in scanline order."""
    parts = [ru.rays_of_camera(tr, w, h, fx, fy) for tr in trs]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ---- 1. colour, arbitrary rays == the oracle -----------------------------------------------------------------
ARBITRARY_OPTIONS = {
    "default": {},
    "no_early_stop": dict(stop_thresh=0.0),
    "basis_minmax": dict(basis_minmax=(1, 3)),
    "rot_dirs": dict(rot_dirs=(0.3, -0.2, 0.9)),
}


@functools.lru_cache(maxsize=None)
def arbitrary_reference(name, optset, fp_mode):
    tree, ndc = tree_named(name)
    o, d = ru.arbitrary_rays(tree, 600, seed=sum(map(ord, name)))
    rgba, accum, hit = ru.oracle_rays(tree, o, d, fp_mode, ndc=ndc, **ARBITRARY_OPTIONS[optset])
    for a in (o, d, rgba, accum):
        a.setflags(write=False)
    return o, d, rgba, accum, hit


@FP
@pytest.mark.parametrize("name", ["sh16", "sh9_near", "sh25", "rgba", "n4", "blocked", "sg"])
def test_arbitrary_rays_equal_the_oracle(torch_cuda, name, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    t = upload(name)
    try:
        for optset, kw in ARBITRARY_OPTIONS.items():
            o, d, rgba, accum, hit = arbitrary_reference(name, optset, fp_mode)
            got = t.render_rays(dev(torch, o), dev(torch, d), api.RenderOptions(**kw), want=("rgba", "accum"),
                                fp_mode=fp_mode)
            torch.cuda.synchronize()
            assert t.status() == 0
            g_rgba, g_accum = got["rgba"].cpu().numpy(), got["accum"].cpu().numpy()
            bad = (bits(g_accum) != bits(accum)).any(1)
            print(f"{name} {optset} fp{fp_mode}: {int(bad.sum())} of {bad.size} accumulators differ; "
                  f"{int((accum[:, 3] > 0).sum())} rays with alpha > 0, {bad.size - hit} miss the box")
            assert not bad.any(), (optset, np.flatnonzero(bad)[:8])
            assert np.array_equal(g_rgba, rgba), optset
            assert (accum[:, 3] > 0).sum() > len(o) // 10 and hit < len(o), "the case shows nothing"
    finally:
        t.free_device()


# ---- 2. colour, camera-derived rays == the oracle's frames ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_reference(fp_mode):
    """Three views of the SH16 scene through the oracle -> (origins, dirs, rgba [n, 4], accum [n, 4])."""
    tree = gu.tree_of("sh16")[0]
    trs, size, f = views(fp_mode)
    o, d = camera_rays(trs, size, size, f)
    frames = [common.oracle_frame(tree, tr, size, size, f, fp_mode) for tr in trs]
    rgba = np.concatenate([fr[0].reshape(-1, 4) for fr in frames])
    accum = np.concatenate([fr[1].reshape(-1, 4) for fr in frames])
    for a in (o, d, rgba, accum):
        a.setflags(write=False)
    return o, d, rgba, accum


def shuffled_list(total, n, seed, duplicates=True):
    """Indices of a list of n rays out of `total`: shuffled, the last eighth duplicates of earlier entries."""
    rng = np.random.default_rng(seed)
    n = total if n is None else n
    n_dup = n // 8 if duplicates else 0
    idx = rng.permutation(total)[:n - n_dup]
    idx = np.concatenate([idx, rng.choice(idx, n_dup)]) if n_dup else idx
    return idx[rng.permutation(n)] if duplicates else idx


@FP
@pytest.mark.parametrize("n", SIZES, ids=SIZE_IDS)
def test_camera_rays_equal_the_oracles_frames(torch_cuda, n, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    o, d, rgba, accum = frames_reference(fp_mode)
    idx = shuffled_list(len(o), n, seed=11 + (n or 0))
    t = upload("sh16")
    try:
        od, dd = dev(torch, o[idx]), dev(torch, d[idx])
        for want in (("accum",), ("rgba",), ("rgba", "accum")):
            got = t.render_rays(od, dd, api.RenderOptions(), want=want, fp_mode=fp_mode)
            torch.cuda.synchronize()
            assert t.status() == 0 and sorted(got) == sorted(want)
            if "accum" in want:
                bad = (bits(got["accum"].cpu().numpy()) != bits(accum[idx])).any(1)
                assert not bad.any(), (want, int(bad.sum()), bad.size)
            if "rgba" in want:
                assert np.array_equal(got["rgba"].cpu().numpy(), rgba[idx]), want
    finally:
        t.free_device()
    assert (accum[:, 3] > 0).sum() > len(o) // 10 and (accum[:, 3] == 0).any()


# ---- 3. leaf weights -----------------------------------------------------------------------------------------
def weight_views(name, fp_mode):
    """-> (tree, ndc, transforms, w, h, focal)."""
    tree, ndc = tree_named(name)
    if ndc is not None:    # (the NDC pose is the identity rotation: exact in both models)
        return tree, ndc, [au.NDC_TRANSFORM], 47, 35, 40.0
    if fp_mode == 0:
        return tree, None, gu.poses(2, size=48), 48, 48, common.camera_for(size=48)[3]
    return tree, None, PERM_POSES[:2], 47, 47, 56.0


@functools.lru_cache(maxsize=None)
def weights_reference(name, fp_mode):
    tree, ndc, trs, w, h, f = weight_views(name, fp_mode)
    mw, hc, _ = wu.restate(tree, trs, w, h, f, fp_mode, ndc=ndc)
    o, d = camera_rays(trs, w, h, f)
    for a in (mw, hc, o, d):
        a.setflags(write=False)
    return tree, o, d, mw, hc


@FP
@pytest.mark.parametrize("name", ["sh16", "n4", "ndc"])
def test_weights_of_a_doubled_list(torch_cuda, name, fp_mode):
    """Every ray twice, shuffled, into sentinel buffers: max_weight bit-equal, hits exactly twice the views'."""
    torch = torch_cuda
    from volrend_amd import api
    tree, o, d, want_mw, want_hits = weights_reference(name, fp_mode)
    idx = np.random.default_rng(5).permutation(np.concatenate([np.arange(len(o))] * 2))
    t = upload(name)
    try:
        mw = torch.full(wu.slots_shape(tree), float(SENT_W), dtype=torch.float32, device="cuda")
        hc = torch.full(wu.slots_shape(tree), -16, dtype=torch.int32, device="cuda")          # SENT_H
        t.accumulate_weights_rays(dev(torch, o[idx]), dev(torch, d[idx]), api.RenderOptions(), max_weight=mw,
                                  hits=hc, want=(), fp_mode=fp_mode)
        torch.cuda.synchronize()
        assert t.status() == 0
        exp_mw, exp_hits = expected(want_mw, (2 * want_hits).astype(np.uint32))
        wu.assert_same_slots(mw.cpu().numpy(), hc.cpu().numpy(), exp_mw, exp_hits, f"{name} fp{fp_mode}")
    finally:
        t.free_device()
    assert (want_hits == 0).any() and (want_mw > 0).any(), "the case shows nothing"


@FP
def test_weights_split_over_two_streams(torch_cuda, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    tree, o, d, want_mw, want_hits = weights_reference("sh16", fp_mode)
    idx = np.random.default_rng(6).permutation(len(o))
    cut = 1000                                  # (not a multiple of 64)
    t = upload("sh16")
    try:
        t.reserve_rays(len(o), 2)
        od, dd = dev(torch, o[idx]), dev(torch, d[idx])
        one = t.accumulate_weights_rays(od, dd, api.RenderOptions(), want=("max_weight", "hits"), fp_mode=fp_mode)
        mw = torch.zeros(wu.slots_shape(tree), dtype=torch.float32, device="cuda")
        hc = torch.zeros(wu.slots_shape(tree), dtype=torch.int32, device="cuda")
        parts = [(od[:cut].contiguous(), dd[:cut].contiguous()), (od[cut:].contiguous(), dd[cut:].contiguous())]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for s, (po, pd) in zip(streams, parts):
            with torch.cuda.stream(s):
                t.accumulate_weights_rays(po, pd, api.RenderOptions(), max_weight=mw, hits=hc, want=(),
                                          fp_mode=fp_mode, stream=s)
        torch.cuda.synchronize()
        assert t.status() == 0
        wu.assert_same_slots(one["max_weight"].cpu().numpy(), one["hits"].cpu().numpy(), want_mw, want_hits, "one call")
        wu.assert_same_slots(mw.cpu().numpy(), hc.cpu().numpy(), want_mw, want_hits, "two streams")
    finally:
        t.free_device()


# ---- 4. backward ---------------------------------------------------------------------------------------------
def backward_list(torch, t, ref, fp_mode, idx, start=None, stream=None, grad_data=None):
    """vr_render_backward_rays over rays `idx` of the views of `ref`, grad_accum permuted alike."""
    from volrend_amd import api
    o, d = camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"])
    g = np.asarray(ref["g"]).reshape(-1, 4)
    if grad_data is None and start is not None:
        grad_data = dev(torch, start.copy())
    return t.render_backward_rays(dev(torch, o[idx]), dev(torch, d[idx]), api.RenderOptions(**ref["opt"]),
                                  dev(torch, g[idx]), grad_data=grad_data, fp_mode=fp_mode, stream=stream)


@pytest.mark.parametrize("name,size,n,optset,gkind", gu.PARITY_CASES,
                         ids=[f"{c[0]}-{c[3]}-{c[4]}" for c in gu.PARITY_CASES])
def test_backward_of_shuffled_camera_lists(torch_cuda, name, size, n, optset, gkind):
    """Strict model (the views are orbit poses).  Into a sentinel: untouched elements keep its bits."""
    torch = torch_cuda
    ref = gu.reference(name, optset, 0, n, size, gkind)
    idx = np.random.default_rng(9).permutation(len(ref["trs"]) * ref["w"] * ref["h"])
    start = sentinel(ref["grad"].shape)
    t = upload(name)
    try:
        got = backward_list(torch, t, ref, 0, idx, start=start)
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert (ref["mag"] > 0).sum() > 200, "the case shows nothing"
    assert_parity(got, ref, start=start, what=f"rays {name} {optset} {gkind}")


@pytest.mark.parametrize("name", ["sh16", "sh4_negative_thresh", "rgba"])
def test_backward_of_shuffled_lists_contains_non_finite_rays(torch_cuda, name):
    """The full-catalogue edge cases of tests/grad_util.py as shuffled lists: dirty and clean rays share a wave,
    and for SH4 and RGBA one packed scatter instruction.  The assertions of
    tests/test_gpu_grad.py::test_non_finite_rays_are_contained."""
    torch = torch_cuda
    ref = gu.edge_reference(name, "full", 0)
    idx = np.random.default_rng(9).permutation(ref["w"] * ref["h"])
    start = sentinel(ref["grad"].shape)
    t = upload_edge(ref)
    try:
        got = backward_list(torch, t, ref, 0, idx, start=start)
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert_contained(got, ref, start, what=f"rays full {name}")


def fma_reference(name):
    """The float64 gradient of views whose rays are exact in the FMA model -> a dict like grad_util.reference's."""
    if name == "ndc":
        return gu.reference("ndc", "default", 1, 1, 0)       # (the NDC pose is the identity rotation)
    return perm_reference()


@functools.lru_cache(maxsize=None)
def perm_reference():
    tree = gu.tree_of("sh16")[0]
    trs, w, h, f = PERM_POSES[:2], 41, 41, 48.0
    g = gu.upstream("normal", len(trs), h, w)
    d64 = gu.data64_of(tree)
    grad, mag, under = (np.zeros(d64.shape, np.float64) for _ in range(3))
    for i, tr in enumerate(trs):
        gu.Trace(tree, tr, w, h, f, 1).backward64(d64, g[i].astype(np.float64), grad, mag, under)
    return dict(tree=tree, ndc=None, trs=trs, w=w, h=h, f=f, g=g, grad=grad, mag=mag, under=under, opt={})


@pytest.mark.parametrize("name", ["sh16", "ndc"])
def test_backward_fma_model(torch_cuda, name):
    torch = torch_cuda
    ref = fma_reference(name)
    idx = np.random.default_rng(10).permutation(len(ref["trs"]) * ref["w"] * ref["h"])
    start = sentinel(ref["grad"].shape)
    t = upload(name)
    try:
        got = backward_list(torch, t, ref, 1, idx, start=start)
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert (ref["mag"] > 0).sum() > 200, "the case shows nothing"
    assert_parity(got, ref, start=start, what=f"rays {name} fma")


@pytest.mark.parametrize("n", SIZES, ids=SIZE_IDS)
def test_backward_list_sizes(torch_cuda, n):
    """A shuffled sub-list of the rays of three 96 x 96 views: the float64 reference is that of the frames with
    the gradient of every other pixel set to zero."""
    torch = torch_cuda
    full = gu.reference("sh16", "default", 0, 3, 96)
    total = 3 * 96 * 96
    hitting = np.flatnonzero(np.concatenate([tr.n_hits for tr in full["traces"]]) > 0)
    idx = shuffled_list(total, n, seed=21 + (n or 0), duplicates=False)
    if not np.isin(idx, hitting).any():        # (a list of one ray: one that has a hit sample)
        idx[0] = hitting[len(hitting) // 2]
    g = np.zeros((total, 4), np.float32)
    g[idx] = np.asarray(full["g"]).reshape(-1, 4)[idx]
    g = g.reshape(3, 96, 96, 4)
    d64 = gu.data64_of(full["tree"])
    grad, mag, under = (np.zeros(d64.shape, np.float64) for _ in range(3))
    for i, tr in enumerate(full["traces"]):
        tr.backward64(d64, g[i].astype(np.float64), grad, mag, under)
    ref = dict(full, g=g, grad=grad, mag=mag, under=under)
    start = sentinel(grad.shape)
    t = upload("sh16")
    try:
        got = backward_list(torch, t, ref, 0, idx, start=start)
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert (mag > 0).any(), "the case shows nothing"
    assert_parity(got, ref, start=start, what=f"list of {len(idx)} rays")


@FP
def test_backward_one_call_three_calls_two_streams(torch_cuda, fp_mode):
    """One list == three lists into one buffer == a split over two streams, within 2 K units; each within K."""
    torch = torch_cuda
    ref = gu.reference("sh16", "default", 0, 3, 24) if fp_mode == 0 else perm_reference()
    total = len(ref["trs"]) * ref["w"] * ref["h"]
    idx = np.random.default_rng(12).permutation(total)
    cuts = [0, 500, 1111, total]
    t = upload("sh16")
    try:
        t.reserve_rays(total, 2)
        one = backward_list(torch, t, ref, fp_mode, idx)
        three = None
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            three = backward_list(torch, t, ref, fp_mode, idx[lo:hi], grad_data=three)
        split = torch.zeros_like(one)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for s, (lo, hi) in zip(streams, ((0, cuts[2]), (cuts[2], total))):
            with torch.cuda.stream(s):
                backward_list(torch, t, ref, fp_mode, idx[lo:hi], grad_data=split, stream=s)
        torch.cuda.synchronize()
        assert t.status() == 0
        one, three, split = (x.cpu().numpy() for x in (one, three, split))
    finally:
        t.free_device()
    unit, pos = gu.unit(ref), ref["mag"] > 0
    for what, other in (("three calls", three), ("two streams", split)):
        assert_parity(other, ref, what=what)
        diff = np.abs(one.astype(np.float64) - other.astype(np.float64))
        assert (diff[pos] <= 2 * gu.K * unit[pos]).all() and (diff[~pos] == 0).all(), what
    assert_parity(one, ref, what="one call")


# ---- 5. n == 0, vr_reserve_rays ------------------------------------------------------------------------------
def test_empty_lists_launch_nothing(torch_cuda):
    torch = torch_cuda
    from volrend_amd import api
    tree = gu.tree_of("sh4")[0]
    t = upload("sh4")
    try:
        empty = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
        bytes0 = t.info()["device_bytes"]
        got = t.render_rays(empty, empty, api.RenderOptions(), want=("rgba", "accum"))
        assert tuple(got["rgba"].shape) == (0, 4) and tuple(got["accum"].shape) == (0, 4)
        assert t.info()["device_bytes"] == bytes0                                 # the colour call uploads nothing
        start = sentinel(tuple(tree.data.shape))
        buf = dev(torch, start.copy())
        out = t.render_backward_rays(empty, empty, api.RenderOptions(), torch.zeros((0, 4), device="cuda"),
                                     grad_data=buf)
        torch.cuda.synchronize()
        assert out is buf and t.status() == 0
        assert t.info()["device_bytes"] == bytes0 + 4 * tree.capacity             # the file-order table, nothing else
        mw = torch.full(wu.slots_shape(tree), 0.25, dtype=torch.float32, device="cuda")
        t.accumulate_weights_rays(empty, empty, api.RenderOptions(), max_weight=mw, want=())
        torch.cuda.synchronize()
        assert t.info()["device_bytes"] == bytes0 + 4 * tree.capacity
        assert np.array_equal(bits(buf.cpu().numpy()), bits(start)) and bool((mw == 0.25).all())
    finally:
        t.free_device()


def test_reserve_rays_covers_later_calls(torch_cuda):
    """After reserve_rays(n, 2) ray calls of n rays on two streams change neither device_bytes nor -- beyond what
    the runtime takes for itself -- the device's free memory.  n = 2^20: the two ray buffers are 2 x 84 MB, which a
    call that had to allocate would show; the same calls on a tree without the reservation do show them.  The
    16 MiB allowed are the runtime's own (queues and pools of new streams: 2 MiB was seen)."""
    torch = torch_cuda
    from volrend_amd import api
    tree = gu.tree_of("sh16")[0]
    n = 1 << 20
    gen = torch.Generator(device="cuda").manual_seed(4)
    od = torch.randn((n, 3), device="cuda", generator=gen)
    od = (od / od.norm(dim=1, keepdim=True) * 4.0).contiguous()
    dd = (-od + 0.5 * torch.randn((n, 3), device="cuda", generator=gen)).contiguous()
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    g = torch.ones((n, 4), dtype=torch.float32, device="cuda")
    gd = torch.zeros(tuple(tree.data.shape), dtype=torch.float32, device="cuda")
    mw = torch.zeros(wu.slots_shape(tree), dtype=torch.float32, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def calls(t):
        """-> (growth of device_bytes, drop of the device's free memory) over the calls."""
        torch.cuda.synchronize()
        bytes0, free0 = t.info()["device_bytes"], torch.cuda.mem_get_info()[0]
        for s in streams:
            with torch.cuda.stream(s):
                t.render_rays(od, dd, api.RenderOptions(), want=(), accum=out, stream=s)   # (no rgba: slot scratch)
                t.accumulate_weights_rays(od, dd, api.RenderOptions(), max_weight=mw, want=(), stream=s)
                t.render_backward_rays(od, dd, api.RenderOptions(), g, grad_data=gd, stream=s)
        torch.cuda.synchronize()
        assert t.status() == 0
        return t.info()["device_bytes"] - bytes0, free0 - torch.cuda.mem_get_info()[0]

    for reserve in (True, False):
        t = upload("sh16")
        try:
            t.accumulate_weights_rays(od[:0], dd[:0], api.RenderOptions())            # the file-order table
            if reserve:
                t.reserve_rays(n, 2)
            grown, dropped = calls(t)
            print(f"reserve={reserve}: device_bytes +{grown}, free memory -{dropped}")
            assert grown == 0
            if reserve:
                assert dropped < (16 << 20), "a ray call allocated after reserve_rays"
                assert bool((out[:, 3] > 0).any())
            else:
                assert dropped > (64 << 20), "the control shows nothing"
        finally:
            t.free_device()


# ---- 6. frames still equal frames ----------------------------------------------------------------------------
def test_frames_before_and_after_ray_launches(torch_cuda):
    """One stream, hence one launch slot: a frame render, ray launches of all three kinds (larger and smaller
    than the frame), the frame render again -- the same bytes, equal to the oracle's."""
    torch = torch_cuda
    from volrend_amd import api
    tree = gu.tree_of("sh16")[0]
    o, d, _, _ = frames_reference(0)
    tr, w, h, f = common.camera_for(size=64)
    want_rgba, want_accum, _ = common.oracle_frame(tree, tr, w, h, f, 0)
    t = upload("sh16")
    try:
        cam = api.Camera(w, h, f, f)
        cam.transform = np.asarray(tr, np.float32)

        def frame():
            img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            api.launch_renderer(t, cam, api.RenderOptions(), img, offscreen=True, accum=acc)
            torch.cuda.synchronize()
            return img.cpu().numpy(), acc.cpu().numpy()

        before = frame()
        for n in (len(o), 100):
            od, dd = dev(torch, o[:n]), dev(torch, d[:n])
            t.render_rays(od, dd, api.RenderOptions(), want=("accum",))
            t.render_rays(od, dd, api.RenderOptions(), want=("rgba", "accum"))
            t.accumulate_weights_rays(od, dd, api.RenderOptions())
            t.render_backward_rays(od, dd, api.RenderOptions(), torch.ones((n, 4), device="cuda"))
        after = frame()
        assert t.status() == 0
    finally:
        t.free_device()
    for got in (before, after):
        assert np.array_equal(got[0], want_rgba) and np.array_equal(bits(got[1]), bits(want_accum))


def test_bench_tools_pixel_rays_are_the_frames_rays(torch_cuda):
    """tools/benchlib.py pixel_rays, from which the ray benchmarks draw their batches: the rays of all pixels of
    three 64 x 48 frames (W != H, so that a swap of % W and // W, or of W and H, shows) render the bytes of the
    batch launch of the same poses, strict model, offscreen; and a seeded pick of 1,000 (frame, pixel) pairs gives
    the rows of the full list at those indices."""
    import os
    import sys
    torch = torch_cuda
    from volrend_amd import api
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import benchlib as bl
    w, h = 64, 48
    trs = [common.camera_for(pose_idx=i, size=w)[0] for i in range(3)]
    focal = common.camera_for(size=w)[3]
    m = dev(torch, np.stack(trs).astype(np.float32))
    every = torch.arange(3 * h * w, device="cuda")
    o, d = bl.pixel_rays(torch, m, w, h, focal, every // (h * w), every % (h * w))
    assert o.dtype == d.dtype == torch.float32 and tuple(o.shape) == tuple(d.shape) == (3 * h * w, 3)
    assert o.is_contiguous() and d.is_contiguous()
    t = api.N3Tree.from_synth(common.small_scene())
    try:
        imgs = torch.zeros((3, h, w, 4), dtype=torch.uint8, device="cuda")
        api.launch_renderer_batch(t, api.Camera(w, h, focal, focal), trs, api.RenderOptions(), list(imgs), None, True)
        got = t.render_rays(o, d, api.RenderOptions(), want=("rgba",))["rgba"]
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    assert bool((imgs[..., :3] != imgs[0, 0, 0, :3]).any()), "the scene must be in view"
    assert torch.equal(got, imgs.view(-1, 4))
    pick = torch.randint(0, 3 * h * w, (1000,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    po, pd = bl.pixel_rays(torch, m, w, h, focal, pick // (h * w), pick % (h * w))
    assert torch.equal(po, o[pick]) and torch.equal(pd, d[pick])


# ---- 7. optim ------------------------------------------------------------------------------------------------
def test_optim_forward_and_gradient(torch_cuda):
    torch = torch_cuda
    from volrend_amd import api, optim
    ref = gu.reference("sh4", "default", 0, 1, 40)
    o, d = camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"])
    od, dd = dev(torch, o), dev(torch, d)
    t = upload("sh4")
    try:
        plain = t.render_rays(od, dd, api.RenderOptions())["accum"].cpu().numpy()
        model = optim.TreeRays(t)
        assert model.data.dtype == torch.float32 and tuple(model.data.shape) == ref["grad"].shape
        leaf = np.asarray(ref["tree"].child) == 0
        assert np.array_equal(model.data.detach().cpu().numpy()[leaf], np.asarray(ref["tree"].data, np.float32)[leaf])
        accum = model(od, dd)
        G = dev(torch, np.asarray(ref["g"]).reshape(-1, 4))
        (G * accum).sum().backward()
        torch.cuda.synchronize()
        assert t.status() == 0
        assert np.array_equal(bits(accum.detach().cpu().numpy()), bits(plain))      # forward: render_rays' bits
        got = model.data.grad.cpu().numpy()
    finally:
        t.free_device()
    assert_parity(got, ref, what="optim: d (G * accum).sum() / d data")


def test_optim_sgd_lowers_the_loss(torch_cuda):
    """30 plain SGD steps towards the accumulators of a perturbed copy of a depth-4 SH4 tree end strictly below
    the starting loss (half the sum of squares).  The rate: a coefficient's gradient sums, over the 10-100 rays
    that cross its leaf, a residual of ~0.05 times a sensitivity w c (1 - c) B of ~0.04: 0.02-0.2, so at 0.5 a
    step is 0.01-0.1 -- far above half a binary16 ulp of a coefficient (2.4e-4 at 0.5-1): steps survive the
    rounding into the tree.  The curvature of such an element is at most ~1 (a density seen by 100 rays with
    sensitivity 0.1), so 0.5 is stable."""
    torch = torch_cuda
    import dataclasses
    from volrend_amd import api, optim
    tree = gu.tree_of("sh4")[0]
    rng = np.random.default_rng(31)
    noisy = np.asarray(tree.data, np.float32) * (1 + 0.3 * rng.standard_normal(tree.data.shape)).astype(np.float32)
    noisy[np.asarray(tree.child) != 0] = 0
    target_tree = dataclasses.replace(tree, data=noisy.astype(np.float16))
    trs, w, h, f = gu.views("sh4", 40, 1)
    o, d = camera_rays(trs, w, h, f)
    od, dd = dev(torch, o), dev(torch, d)
    tt = api.N3Tree.from_synth(target_tree)
    t = upload("sh4")
    try:
        target = tt.render_rays(od, dd, api.RenderOptions())["accum"]
        model = optim.TreeRays(t)
        opt = torch.optim.SGD(model.parameters(), lr=0.5)
        curve = []
        for _ in range(31):
            opt.zero_grad()
            loss = 0.5 * ((model(od, dd) - target) ** 2).sum()
            curve.append(float(loss.detach()))
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
        tt.free_device()
    print("loss:", " ".join(f"{x:.3e}" for x in curve))
    assert curve[0] > 0 and np.isfinite(curve).all()
    assert curve[-1] < curve[0], "30 SGD steps did not lower the loss"
