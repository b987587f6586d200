"""-m gpu: the ray hand-out of render_kernel, colour and AOV flavours, is scheduling only.

A wave takes its rays from the queue of its XCD in guided chunks of at most `chunk_max` rays (tuning key;
0 = the host's rule for the kind of launch, vr_launch_plan.cpp plan_launch) and refills its idle lanes from the
chunk in hand.  Whatever the cap, the refill threshold, the number of waves and of queues: every frame of a
batch equals the oracle byte for byte, the status word stays 0, the AOV planes equal those of the
chunk_max=4096 launch, launches whose queues hold less than a chunk -- or nothing -- end, and the sample
guard still trips."""
import itertools

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

SIZES = [(40, 24), (63, 41)]    # 15 blocks (fewer than 16: the single-queue split edge); ragged edges
N_FRAMES = [1, 3, 17]           # 17 exceeds one 16-wave ray-generation workgroup
TUNINGS = [dict(chunk_max=c, refill_min=r, waves_per_cu=wv, xcd_queues=q)
           for c, r, wv, q in itertools.product([0, 64, 128, 4096], [1, 20, 64], [1, 0], [0, 1])]
FOCAL = 70.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def poses(n):
    return [common.camera_for(pose_idx=i, n_poses=17, size=64)[0] for i in range(n)]


_scenes = {}


def scene(fmt="SH", basis_dim=16):
    """(tree, {(w, h): the oracle's 17 frames}) -- computed once per module, never written to."""
    key = (fmt, basis_dim)
    if key not in _scenes:
        _scenes[key] = (common.small_scene(depth=5, basis_dim=basis_dim, fmt=fmt), {})
    return _scenes[key]


def oracle_frames(fmt, basis_dim, w, h, n):
    tree, cache = scene(fmt, basis_dim)
    got = cache.setdefault((w, h), [])
    trs = poses(n)
    while len(got) < n:
        got.append(common.oracle_frame(tree, trs[len(got)], w, h, FOCAL, 0)[0])
    return tree, trs, got[:n]


def render(torch, t, w, h, trs, **kw):
    from volrend_amd import api
    imgs = torch.zeros((len(trs), h, w, 4), dtype=torch.uint8, device="cuda")
    api.launch_renderer_batch(t, api.Camera(w, h, FOCAL, FOCAL), trs, api.RenderOptions(), list(imgs), None, True, **kw)
    torch.cuda.synchronize()
    return imgs.cpu().numpy()


@pytest.mark.parametrize("n_frames", N_FRAMES)
@pytest.mark.parametrize("w,h", SIZES)
def test_every_chunking_renders_the_oracles_frames(torch_cuda, w, h, n_frames):
    from volrend_amd import api
    tree, trs, want = oracle_frames("SH", 16, w, h, n_frames)
    assert any((f[..., :3] != f[0, 0, :3]).any() for f in want), "the scene must be in view"
    t = api.N3Tree.from_synth(tree)
    try:
        for tn in TUNINGS:
            t.set_tuning(**tn)
            got = render(torch_cuda, t, w, h, trs)
            assert t.status() == 0, tn
            for i in range(n_frames):
                assert np.array_equal(got[i], want[i]), (tn, "frame", i)
    finally:
        t.free_device()


@pytest.mark.parametrize("fmt,basis_dim,tn", [("SH", 9, dict(chunk_max=64, refill_min=20)),
                                              ("RGBA", 0, dict(chunk_max=128, refill_min=1, xcd_queues=0))],
                         ids=["SH9", "RGBA"])
def test_other_formats(torch_cuda, fmt, basis_dim, tn):
    from volrend_amd import api
    w, h = SIZES[1]
    tree, trs, want = oracle_frames(fmt, basis_dim, w, h, 3)
    t = api.N3Tree.from_synth(tree)
    try:
        for tune in (dict(chunk_max=0), tn):
            t.set_tuning(**tune)
            got = render(torch_cuda, t, w, h, trs)
            assert t.status() == 0
            for i in range(3):
                assert np.array_equal(got[i], want[i]), (tune, "frame", i)
    finally:
        t.free_device()


@pytest.mark.parametrize("n_frames", [3, 17])
def test_aov_planes_do_not_depend_on_the_chunking(torch_cuda, n_frames):
    torch = torch_cuda
    from volrend_amd import api
    w, h = SIZES[1]
    tree, trs, want = oracle_frames("SH", 16, w, h, n_frames)
    t = api.N3Tree.from_synth(tree)

    def planes(**tn):
        t.set_tuning(**tn)
        d = torch.full((n_frames, h, w), 0x7FC12345, dtype=torch.int32, device="cuda")
        tr = torch.full((n_frames, h, w), 0x7FC12345, dtype=torch.int32, device="cuda")
        aov = [api.AovPlanes(d[i], tr[i], 0) for i in range(n_frames)]
        img = render(torch, t, w, h, trs, aov=aov, depth_units="tree")
        assert t.status() == 0, tn
        return img, d.cpu().numpy(), tr.cpu().numpy()

    try:
        img0, d0, t0 = planes(chunk_max=4096, refill_min=20)
        for i in range(n_frames):
            assert np.array_equal(img0[i], want[i]), ("frame", i)
        assert (d0 != 0x7FC12345).all() and (t0 != 0x7FC12345).all(), "a pixel's planes were never written"
        for tn in (dict(chunk_max=0), dict(chunk_max=64, refill_min=1), dict(chunk_max=128, refill_min=64, xcd_queues=0),
                   dict(chunk_max=64, waves_per_cu=1)):
            img, d, tr = planes(**tn)
            assert np.array_equal(img, img0) and np.array_equal(d, d0) and np.array_equal(tr, t0), tn
    finally:
        t.free_device()


@pytest.mark.parametrize("position,look_at,expect_hits", [((3.0, -3.0, 0.5), (3.0, 3.0, 0.5), True),
                                                          ((4.0, 4.0, 4.0), (8.0, 8.0, 8.0), False)],
                         ids=["mostly_past_the_box", "every_ray_misses"])
def test_sparse_queues(torch_cuda, position, look_at, expect_hits):
    """Queues that hold fewer rays than one chunk, some none; and a launch without a single ray in the
    volume (every grab comes back empty: the kernel must end, the frame is background)."""
    from volrend_amd import api
    tree, _ = scene("SH", 16)
    tr, w, h, f = common.camera_at(position, look_at, size=40, focal=28.0)
    want, _, cnt = common.oracle_frame(tree, tr, w, h, f, 0)
    assert (cnt["hit_samples"] > 0) == expect_hits and (cnt["rays_hit_box"] > 0) == expect_hits
    if expect_hits:  # few rays enter: fewer than a chunk per queue
        bg = want[(want == want[0, 0]).all(axis=-1)]
        assert 0 < (h * w - len(bg)) and len(bg) > h * w // 2, "the camera must look mostly past the box"
    else:
        assert (want == want[0, 0]).all()
    t = api.N3Tree.from_synth(tree)
    cam = api.Camera(w, h, f, f)
    import torch
    try:
        for tn in (dict(chunk_max=0), dict(chunk_max=64, refill_min=1), dict(chunk_max=4096, refill_min=64),
                   dict(chunk_max=128, xcd_queues=0, waves_per_cu=1)):
            t.set_tuning(**tn)
            for n in (1, 3):
                imgs = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
                api.launch_renderer_batch(t, cam, [tr] * n, api.RenderOptions(), list(imgs), None, True)
                torch.cuda.synchronize()
                assert t.status() == 0
                for i in range(n):
                    assert np.array_equal(imgs[i].cpu().numpy(), want), (tn, n, i)
    finally:
        t.free_device()


def test_sample_guard_with_small_chunks(torch_cuda):
    """max_iter = 2 with 64-ray chunks: the guard cuts what still marches, sets the status bit, and the
    launch ends (tests/test_gpu_status.py, at the default chunking)."""
    from volrend_amd import api
    w, h = SIZES[1]
    tree, trs, want = oracle_frames("SH", 16, w, h, 3)
    t = api.N3Tree.from_synth(tree)
    try:
        t.set_tuning(chunk_max=64, max_iter=2)
        got = render(torch_cuda, t, w, h, trs)
        assert t.status() & 1, "rays were cut by the guard but the status word says nothing"
        assert any(not np.array_equal(got[i], want[i]) for i in range(3)), "cut rays cannot give the right picture"
        assert t.status(reset=True) & 1 and t.status() == 0
        t.set_tuning(max_iter=1 << 22)
        got = render(torch_cuda, t, w, h, trs)
        assert t.status() == 0 and all(np.array_equal(got[i], want[i]) for i in range(3))
    finally:
        t.free_device()
