"""-m gpu: the scheduling knobs are scheduling only -- for the backward march, the fused fit, the ray-list
launches and the non-temporal record stream as for the colour frames of tests/test_gpu_chunks.py.

Every case is judged against the yardsticks the other modules use, never against a default-knob GPU run: the
oracle bit for bit (colour, accumulators, AOV planes), the leaf-weight restatement bit for bit, the float64
gradient formulas under grad_util.assert_parity with K as it stands (tests/grad_util.py SCHED_CASES: the
summation constant of these cases is measured on the CPU), fit_util.assert_four for the fused call.  Knobs are
set per tree; every tree is freed; status() == 0 everywhere.

A  the backward march refills: backward_kernel keeps its own written-out retire / refill frame with far more
   per-ray state than weights_kernel.  With one wave per CU and at least 2 * 64 * CUs rays entering the volume
   some wave takes a second chunk and some lane a second ray whatever the launch order (the grid is at most
   CUs * waves_per_cu waves, a chunk at least 64 rays): asserted per case from the CPU trace.
B  the 16-wave flavours of list ray generation, which plan_launch picks only above 1 280 000 rays: lists of
   1 .. 8200 rays with raygen_waves forced, outputs in exactly sized buffers with a poisoned guard band.
C  records_nt = 1 (the second copy of the record DMA issue loop, production path of every large tree) against
   records_nt = 0 and the oracle: every staged basis, both FP models, colour batch / AOV / ray list.
D  colour ray lists under chunk, refill and drain knobs, across rows of the 2^15-wide pseudo-frame.

CPU references: cached per module (functools.lru_cache over the tests' helpers); all of them together take
about 5 s of CPU time."""
import functools

import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import fit_util as fu
from tests import grad_util as gu
from tests import rays_util as ru
from tests import weights_util as wu
from tests.fit_util import bits, dev
from tests.grad_util import assert_parity, sentinel
from tests.rays_util import Guarded

pytestmark = pytest.mark.gpu
FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])

FIRST = dict(waves_per_cu=1, refill_min=1)
HARSHEST = dict(waves_per_cu=1, refill_min=1, march_max=1, chunk_max=64, raygen_waves=4)
REFILL_KNOBS = [FIRST,
                dict(waves_per_cu=1, refill_min=64, march_max=1),
                dict(waves_per_cu=1, refill_min=20, chunk_max=64, xcd_queues=0),
                HARSHEST,
                dict(waves_per_cu=1, raygen_waves=16, frame_group=1)]


def knob_id(k):
    return "-".join(f"{a}{b}" for a, b in k.items())


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def pigeonhole_bound(torch, waves_per_cu=1):
    """Entering rays from which on some wave takes a second chunk: the grid is at most CUs * waves_per_cu waves
    (persistent_grid) and grab_chunk hands out at least 64 rays."""
    return 2 * 64 * torch.cuda.get_device_properties(0).multi_processor_count * waves_per_cu


def refill_reference(torch, name, optset="default", fp_mode=0, gkind="normal"):
    """grad_util.reference of enough orbit poses at 96 x 96 for the pigeonhole bound: 8 on a 256-CU device (the
    shape of tests/test_gpu_weights.py::test_refill_chunks_and_knobs_change_nothing), more in steps of 8 where
    the device has more CUs."""
    bound = pigeonhole_bound(torch)
    for n_poses in range(gu.SCHED_POSES, 65, 8):
        ref = gu.reference(name, optset, fp_mode, n_poses, gu.SCHED_SIZE, gkind)
        n_enter, n_hit_free = gu.entering(ref)
        if n_enter >= bound:
            break
    print(f"{name} {optset} {gkind} fp{fp_mode}: {n_poses} poses, {n_enter} rays enter (bound {bound}), "
          f"{n_hit_free} of them without a hit sample, M > 0 in {int((ref['mag'] > 0).sum())} elements")
    assert n_enter >= bound, "no wave is certain to take a second chunk: the case shows nothing"
    assert (ref["mag"] > 0).sum() > 200, "the case shows nothing"
    return ref


@functools.lru_cache(maxsize=None)
def marks_of(name, optset, fp_mode, n_poses, size):
    return gu.mark_words(gu.hit_slots(gu.reference(name, optset, fp_mode, n_poses, size)))


def want_marks(ref, name, optset, fp_mode):
    """The bitmap of the slots the restatement hits (it does not depend on grad_accum)."""
    return marks_of(name, optset, fp_mode, len(ref["trs"]), ref["w"])


def shuffled(n, seed, drop=0):
    return np.random.default_rng(seed).permutation(n)[:n - drop]


# ---- A. refill of the backward march ---------------------------------------------------------------------------
def backward_frames(torch, name, knobs, optset="default", gkind="normal", fp_mode=0):
    """vr_render_backward, unmarked and marked (two kernels), on one tree under ``knobs``: each within K of the
    float64 formulas into a sentinel whose untouched elements keep their bits; the marks are exactly the slots
    the restatement hits."""
    from volrend_amd import api
    ref = refill_reference(torch, name, optset, fp_mode, gkind)
    marks = want_marks(ref, name, optset, fp_mode)
    start = sentinel(ref["grad"].shape)
    cam, opts = api.Camera(ref["w"], ref["h"], ref["f"], ref["f"]), api.RenderOptions(**ref["opt"])
    t = gu.upload(ref, name)
    try:
        t.set_tuning(**knobs)
        g = dev(torch, ref["g"])
        plain = t.render_backward(cam, ref["trs"], opts, g, grad_data=dev(torch, start), fp_mode=fp_mode)
        touched = fu.zero_bits(torch, ref["tree"])
        marked = t.render_backward(cam, ref["trs"], opts, g, grad_data=dev(torch, start), fp_mode=fp_mode,
                                   touched=touched)
        torch.cuda.synchronize()
        assert t.status() == 0
        plain, marked, touched = plain.cpu().numpy(), marked.cpu().numpy(), bits(touched)
    finally:
        t.free_device()
    what = f"{name} {optset} {gkind} fp{fp_mode} {knob_id(knobs)}"
    assert_parity(plain, ref, start=start, what=what)
    assert_parity(marked, ref, start=start, what=what + " marked")
    assert marks.any() and np.array_equal(touched, marks), f"{what}: touched is not the set of slots the rays hit"
    return ref


@pytest.mark.parametrize("knobs", REFILL_KNOBS, ids=knob_id)
def test_backward_frames_under_every_knob_set(torch_cuda, knobs):
    """SH16 (one scatter run of 49 lanes).  grad_accum is non-zero in every pixel, and thousands of rays enter
    without a hit sample, each in a lane whose ray before it may have had hits, been stopped and formed a tail."""
    ref = backward_frames(torch_cuda, "sh16", knobs)
    assert gu.entering(ref)[1] >= 1000 and bool(np.asarray(ref["g"]).all(-1).all())


@pytest.mark.parametrize("name", ["sh9_near", "sh25", "rgba", "basis1", "n4"])
def test_backward_frames_harshest_set_per_scatter_shape(torch_cuda, name):
    """SH9: two packed runs; SH25: two instructions; RGBA: 16 packed runs; one basis function; N = 4: the float
    descent.  (SH16 is the tree of test_backward_frames_under_every_knob_set.)"""
    backward_frames(torch_cuda, name, HARSHEST)


def test_backward_frames_segments_restart_in_a_refilled_lane(torch_cuda):
    """stop_thresh = 0 on the near SH9 scene: rays attenuate below 2^-20 of their segment's light (kSegment), so
    lanes that have already marched another ray go through sum / emit segments: t_ck, light_ck and phase must
    not survive the refill."""
    ref = gu.reference("sh9_near", gu.NO_STOP, 0, gu.SCHED_POSES, gu.SCHED_SIZE)
    deep = sum(int((au.restate(ref["tree"], tr, ref["w"], ref["h"], ref["f"], 0, stop_thresh=0.0)[1] < 2.0 ** -20).sum())
               for tr in ref["trs"])
    print(f"{deep} rays attenuate below 2^-20")
    assert deep > 100, "no ray reaches a segment restart: the case shows nothing"
    backward_frames(torch_cuda, "sh9_near", HARSHEST, optset=gu.NO_STOP)


def test_backward_frames_rays_without_a_hit_carry_a_gradient(torch_cuda):
    """grad_accum = (0, 0, 0, 1): only g_3 is non-zero, the entry a ray's tail is made of, in every pixel -- those
    of the rays that enter without a hit sample included."""
    ref = backward_frames(torch_cuda, "sh16", HARSHEST, gkind="alpha")
    assert gu.entering(ref)[1] >= 1000 and bool((np.asarray(ref["g"])[..., 3] != 0).all())


LIST_KNOBS = pytest.mark.parametrize("knobs", [HARSHEST, FIRST], ids=knob_id)


def list_of(ref, fp_mode, seed):
    """The shuffled rays of the views of ``ref`` -> (idx, origins, dirs)."""
    o, d = fu.camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"], fp_mode)
    idx = shuffled(len(o), seed)
    return idx, o[idx], d[idx]


@LIST_KNOBS
def test_backward_rays_refill(torch_cuda, knobs):
    torch = torch_cuda
    from volrend_amd import api
    ref = refill_reference(torch, "sh16")
    marks = want_marks(ref, "sh16", "default", 0)
    idx, o, d = list_of(ref, 0, 31)
    g = np.asarray(ref["g"]).reshape(-1, 4)[idx]
    start = sentinel(ref["grad"].shape)
    t = gu.upload(ref, "sh16")
    try:
        t.set_tuning(**knobs)
        od, dd, gd, opts = dev(torch, o), dev(torch, d), dev(torch, g), api.RenderOptions(**ref["opt"])
        plain = t.render_backward_rays(od, dd, opts, gd, grad_data=dev(torch, start))
        touched = fu.zero_bits(torch, ref["tree"])
        marked = t.render_backward_rays(od, dd, opts, gd, grad_data=dev(torch, start), touched=touched)
        torch.cuda.synchronize()
        assert t.status() == 0
        plain, marked, touched = plain.cpu().numpy(), marked.cpu().numpy(), bits(touched)
    finally:
        t.free_device()
    assert_parity(plain, ref, start=start, what=f"rays {knob_id(knobs)}")
    assert_parity(marked, ref, start=start, what=f"rays {knob_id(knobs)} marked")
    assert np.array_equal(touched, marks), "touched is not the set of slots the rays hit"


@LIST_KNOBS
def test_weights_rays_refill(torch_cuda, knobs):
    torch = torch_cuda
    from volrend_amd import api
    ref = refill_reference(torch, "sh16")
    n_poses = len(ref["trs"])
    tree, trs, w, h, f, want_mw, want_hits, _ = wu.reference("sh16", "default", 0, n_poses, gu.SCHED_SIZE)
    assert tree is ref["tree"] or np.array_equal(tree.data, ref["tree"].data)
    assert all(np.array_equal(a, b) for a, b in zip(trs, ref["trs"]))
    _, o, d = list_of(ref, 0, 32)
    t = api.N3Tree.from_synth(tree)
    try:
        t.set_tuning(**knobs)
        mw, hc = wu.buffers(torch, tree)
        t.accumulate_weights_rays(dev(torch, o), dev(torch, d), api.RenderOptions(), max_weight=mw, hits=hc, want=())
        torch.cuda.synchronize()
        assert t.status() == 0
        wu.assert_same_slots(wu.host(mw), wu.host(hc), *wu.expected(want_mw, want_hits), knob_id(knobs))
    finally:
        t.free_device()
    assert (want_hits == 0).any() and (want_mw > 0).any(), "the case shows nothing"


@functools.lru_cache(maxsize=None)
def oracle_accum(name, optset, fp_mode, n_poses, size):
    """The oracle's frames of the views of grad_util.reference -> (rgba uint8 [n, 4], accum float32 [n, 4])."""
    ref = gu.reference(name, optset, fp_mode, n_poses, size)
    frames = [common.oracle_frame(ref["tree"], tr, ref["w"], ref["h"], ref["f"], fp_mode, ndc=ref["ndc"], **ref["opt"])
              for tr in ref["trs"]]
    rgba = np.concatenate([fr[0].reshape(-1, 4) for fr in frames])
    accum = np.concatenate([fr[1].reshape(-1, 4) for fr in frames])
    rgba.setflags(write=False)
    accum.setflags(write=False)
    return rgba, accum


@FP
@LIST_KNOBS
def test_fit_rays_refill(torch_cuda, knobs, fp_mode):
    """assert_four under the knobs (the unfused sequence it compares with runs under them too), and accum against
    the oracle's frames: the rays of the FMA model are formed as its matrix product forms them."""
    torch = torch_cuda
    ref = refill_reference(torch, "sh16", fp_mode=fp_mode)
    idx, o, d = list_of(ref, fp_mode, 33 + fp_mode)
    target = fu.targets(len(o), 100 + len(o))
    t = gu.upload(ref, "sh16")
    try:
        t.set_tuning(**knobs)
        res, _, fref = fu.assert_four(torch, t, ref, o, d, target, fp_mode, f"fit fp{fp_mode} {knob_id(knobs)}", idx=idx)
        accum = res["accum"].cpu().numpy()
    finally:
        t.free_device()
    assert (fref["mag"] > 0).sum() > 200, "the case shows nothing"
    want = oracle_accum("sh16", "default", fp_mode, len(ref["trs"]), ref["w"])[1][idx]
    bad = (bits(accum) != bits(want)).any(1)
    assert not bad.any(), f"accum differs from the oracle in {int(bad.sum())} of {bad.size} rays"


# ---- B. sixteen-wave list ray generation -----------------------------------------------------------------------
# n: 1 .. 1025 leave trailing waves of a 16-wave workgroup without a ray (id >= n), and give one full plus one
# nearly empty workgroup; 8200 rays are nine groups of 16 blocks over eight queues, or over one.
GEN_CASES = [(n, q) for n in (1, 63, 1023, 1024, 1025, 8200) for q in (1,)] + [(8200, 0)]
GEN = pytest.mark.parametrize("n,xcd_queues", GEN_CASES, ids=[f"{n}-q{q}" for n, q in GEN_CASES])
GEN_WAVES = pytest.mark.parametrize("raygen_waves", [16, 4])


@functools.lru_cache(maxsize=None)
def strip_reference(name, n, fp_mode):
    """A list of n rays that is also a frame (rays_util.strip_camera), judged by every yardstick of that frame
    -> grad_util.reference's dict plus o, d (scanline order), rgba, accum [n, 4] (the oracle), mw, hits (the
    leaf-weight restatement)."""
    tree, _, ndc = gu.tree_of(name)
    tr, w, h, f = ru.strip_camera(n, fp_mode)
    trace = gu.Trace(tree, tr, w, h, f, fp_mode)
    g = gu.upstream("normal", 1, h, w, seed=3)
    grad, mag, under = trace.backward64(gu.data64_of(tree), g[0].astype(np.float64))
    o, d = fu.rays_of_camera(tr, w, h, f, fp_mode)
    rgba, accum, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode)
    mw, hits, _ = wu.restate(tree, [tr], w, h, f, fp_mode)
    out = dict(tree=tree, ndc=ndc, trs=[tr], w=w, h=h, f=f, g=g, grad=grad, mag=mag, under=under, opt={},
               traces=[trace], o=o, d=d, rgba=rgba.reshape(-1, 4), accum=accum.reshape(-1, 4), mw=mw, hits=hits)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@FP
@GEN_WAVES
@GEN
def test_list_raygen_colour(torch_cuda, n, xcd_queues, raygen_waves, fp_mode):
    """vr_render_rays, one SH and one RGBA tree: the oracle's RGBA8 and accumulators bit for bit."""
    torch = torch_cuda
    from volrend_amd import api
    for name in ("sh16", "rgba"):
        ref = strip_reference(name, n, fp_mode)
        idx = shuffled(n, 40 + n)
        t = gu.upload(ref, name)
        try:
            t.set_tuning(raygen_waves=raygen_waves, xcd_queues=xcd_queues)
            rgba, accum = Guarded(torch, (n, 4), np.uint8), Guarded(torch, (n, 4), np.float32)
            t.render_rays(dev(torch, ref["o"][idx]), dev(torch, ref["d"][idx]), api.RenderOptions(), want=(),
                          rgba=rgba.tensor, accum=accum.tensor, fp_mode=fp_mode)
            torch.cuda.synchronize()
            assert t.status() == 0
            rgba, accum = rgba.host(), accum.host()
        finally:
            t.free_device()
        bad = (bits(accum) != bits(ref["accum"][idx])).any(1)
        assert not bad.any(), (name, int(bad.sum()), n, np.flatnonzero(bad)[:8])
        assert np.array_equal(rgba, ref["rgba"][idx]), name
        assert (ref["accum"][:, 3] > 0).any(), "the case shows nothing"


@GEN_WAVES
@GEN
def test_list_raygen_march(torch_cuda, n, xcd_queues, raygen_waves):
    """The list forms of vr_accumulate_weights (restatement bits), vr_render_backward_rays (float64 parity, marks)
    and vr_fit_rays (assert_four), every output guarded."""
    torch = torch_cuda
    from volrend_amd import api
    ref = strip_reference("sh16", n, 0)
    tree = ref["tree"]
    assert ref["traces"][0].n_hits.sum() > 0 and (ref["mag"] > 0).any(), "the case shows nothing"
    idx = shuffled(n, 50 + n)
    o, d = ref["o"][idx], ref["d"][idx]
    start = sentinel(ref["grad"].shape)
    marks = gu.mark_words(gu.hit_slots(ref))
    t = gu.upload(ref, "sh16")
    try:
        t.set_tuning(raygen_waves=raygen_waves, xcd_queues=xcd_queues)
        od, dd, opts = dev(torch, o), dev(torch, d), api.RenderOptions()
        mw = Guarded(torch, wu.slots_shape(tree), np.float32, wu.SENT_W)
        hc = Guarded(torch, wu.slots_shape(tree), np.int32, -16)                            # SENT_H
        t.accumulate_weights_rays(od, dd, opts, max_weight=mw.tensor, hits=hc.tensor, want=())
        grad, touched = Guarded(torch, start.shape, np.float32, start), Guarded(torch, marks.shape, np.int32, 0)
        t.render_backward_rays(od, dd, opts, dev(torch, np.asarray(ref["g"]).reshape(-1, 4)[idx]),
                               grad_data=grad.tensor, touched=touched.tensor)
        torch.cuda.synchronize()
        assert t.status() == 0
        wu.assert_same_slots(mw.host(), hc.host(), *wu.expected(ref["mw"], ref["hits"]), "weights")
        assert_parity(grad.host(), ref, start=start, what=f"backward of {n} rays, {raygen_waves} waves")
        assert np.array_equal(bits(touched.host()), marks), "touched is not the set of slots the rays hit"
        fu.assert_four(torch, t, ref, o, d, fu.targets(n, 100 + n), 0, f"fit of {n} rays, {raygen_waves} waves", idx=idx,
                       guarded=Guarded)
    finally:
        t.free_device()


# ---- C. the non-temporal record stream ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fog25():
    return common.fog_tree(basis_dim=25, depth=4, seed=3)


def nt_tree(name):
    """-> (tree, camera radius): the SH trees of grad_util's catalogue (SH4 / 9 / 16 / 25: every basis whose records
    are staged), its tree for the blocked brick order, and an SH25 fog tree -- every sample a hit, so the ring is
    always full and the two passes of an SH25 record alternate."""
    if name == "fog25":
        return fog25(), 4.0
    tree, radius, _ = gu.tree_of(name)
    return tree, radius


@functools.lru_cache(maxsize=None)
def nt_reference(name, fp_mode):
    """Three orbit poses at 40 x 40 -> (tree, trs, w, h, f, rgba [3, h, w, 4], accum, D, T [3, h, w], o, d)."""
    tree, radius = nt_tree(name)
    trs = gu.poses(3, size=40, radius=radius)
    w = h = 40
    f = common.camera_for(size=40)[3]
    frames = [common.oracle_frame(tree, tr, w, h, f, fp_mode) for tr in trs]
    planes = [au.restate(tree, tr, w, h, f, fp_mode) for tr in trs]
    o, d = fu.camera_rays(trs, w, h, f, fp_mode)
    out = (tree, trs, w, h, f, np.stack([fr[0] for fr in frames]), np.stack([fr[1] for fr in frames]),
           np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes]), o, d)
    for a in out[5:]:
        a.setflags(write=False)
    return out


@FP
@pytest.mark.parametrize("name", ["sh4", "sh9_near", "sh16", "sh25", "blocked", "fog25"])
def test_records_nt(torch_cuda, name, fp_mode):
    """A 3-frame colour batch, vr_render_aov with both planes and vr_render_rays with records_nt = 1 and with
    records_nt = 0: each the oracle's bits (and so each other's).  (The library reports the knob nowhere:
    vr_tree_info has no field for it, so the forced value is not read back.)"""
    torch = torch_cuda
    from volrend_amd import api
    tree, trs, w, h, f, rgba, accum, D, T, o, d = nt_reference(name, fp_mode)
    assert (accum[..., 3] > 0).sum() > 300 and (D > 0).any(), "the case shows nothing"
    t = gu.upload(dict(tree=tree, ndc=None), name)
    try:
        od, dd = dev(torch, o), dev(torch, d)
        for nt in (1, 0):
            t.set_tuning(records_nt=nt)
            r = au.render_both(torch, t, w, h, f, trs, fp_mode, "tree")
            rays = t.render_rays(od, dd, api.RenderOptions(), want=("rgba", "accum"), fp_mode=fp_mode)
            torch.cuda.synchronize()
            assert t.status() == 0
            for k in ("0", "1"):                   # vr_render_batch, vr_render_aov
                assert np.array_equal(r["img" + k], rgba), (nt, k)
                au.assert_same_bits(r["acc" + k], accum, f"records_nt={nt} accum of launch kind {k}")
            au.assert_same_bits(r["depth"], D, f"records_nt={nt} depth")
            au.assert_same_bits(r["trans"], T, f"records_nt={nt} transmittance")
            assert np.array_equal(rays["rgba"].cpu().numpy(), rgba.reshape(-1, 4)), nt
            au.assert_same_bits(rays["accum"].cpu().numpy(), accum.reshape(-1, 4), f"records_nt={nt} ray list")
    finally:
        t.free_device()


# ---- D. colour lists under chunk and refill knobs ----------------------------------------------------------------
COLOUR_KNOBS = [dict(waves_per_cu=1, refill_min=1, chunk_max=64), dict(waves_per_cu=1, refill_min=64, march_max=1),
                dict(waves_per_cu=1, drain_flush=0), dict(waves_per_cu=1, drain_flush=64, xcd_queues=0)]


@pytest.mark.parametrize("knobs", COLOUR_KNOBS, ids=knob_id)
def test_colour_list_under_chunk_and_refill_knobs(torch_cuda, knobs):
    """The shuffled rays of the poses of section A but 37: more than 2^15 + 64, no multiple of 64, so the list
    crosses rows of the 2^15-wide pseudo-frame and ends in a ragged wave."""
    torch = torch_cuda
    from volrend_amd import api
    ref = refill_reference(torch, "sh16")
    n_poses = len(ref["trs"])
    o, d = fu.camera_rays(ref["trs"], ref["w"], ref["h"], ref["f"], 0)
    idx = shuffled(len(o), 61, drop=37)
    n = len(idx)
    entered = np.concatenate([tr.entered for tr in ref["traces"]])[idx]
    assert n > 2 ** 15 + 64 and n % 64 != 0 and int(entered.sum()) >= pigeonhole_bound(torch)
    rgba, accum = oracle_accum("sh16", "default", 0, n_poses, ref["w"])
    t = gu.upload(ref, "sh16")
    try:
        t.set_tuning(**knobs)
        got = t.render_rays(dev(torch, o[idx]), dev(torch, d[idx]), api.RenderOptions(), want=("rgba", "accum"))
        torch.cuda.synchronize()
        assert t.status() == 0
        g_rgba, g_accum = got["rgba"].cpu().numpy(), got["accum"].cpu().numpy()
    finally:
        t.free_device()
    bad = (bits(g_accum) != bits(accum[idx])).any(1)
    assert not bad.any(), (knobs, int(bad.sum()), np.flatnonzero(bad)[:8])
    assert np.array_equal(g_rgba, rgba[idx]), knobs
    assert (accum[:, 3] > 0).sum() > n // 10 and (accum[:, 3] == 0).any()
