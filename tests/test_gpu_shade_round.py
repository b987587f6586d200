"""The shade round of render_kernel with the owner's basis values fetched one group ahead of their use.

A shade round evaluates up to 64 queued colour items, one per lane: the records arrive by LDS-DMA, the owner's
basis values through ds_bpermute.  vr_dev_shade.h SumsAhead requests b0 and the first group's values in front of the
wait for the records, and every later group's in front of the previous group's arithmetic.  Order and pipelining only:
every frame equals the CPU oracle byte for byte, RGBA8 and the fp32 accumulators, for every record format that is
staged (SH4 / SH9 / SH16 one pass; SH25 two passes with the basis gathered up front, unchanged) in both FP models.

Shapes: a depth-5 synthetic tree per format, three poses in one batch, under waves_per_cu = 1, march_max = 1 (a round
can fire after every march step) and drain_flush = 1 and 64 (partial rounds: only for the last marching ray, or for
any blocked ray once the queues are dry).  stop_thresh = 0: rays cross the whole object, so they queue many items.
  sparse  8 x 8 (one wave per frame at most) from far away: so few rays meet density that 64 items can never wait
          (4 per ray at most) -- every round is a partial one, of whatever the rays in flight have queued, and it
          fires when a ray is blocked or nobody can march: a ray with >= 4 hit samples then owns 4 items.
  dense   16 x 16 (four blocks) from close by: most rays hit on most steps, so rounds of exactly 64 fire while
          the queues feed the waves, and partial ones of shrinking size while they drain.
What the cases rest on is checked on the CPU (oracle.binding.render_maps), without a GPU: rays with >= 8 hit
samples in every case, and for the sparse ones at most 15 rays with a hit in the whole batch."""
import functools

import numpy as np
import pytest

from oracle import binding as ob
from tests import common

BASES = [4, 9, 16, 25]
FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
SHAPES = {"sparse": (8, 14.0), "dense": (16, 2.5)}   # image size, camera radius
POSES = (0, 3, 5)                                     # of the 8-pose orbit
OPT = dict(stop_thresh=0.0)
KNOBS = [dict(waves_per_cu=1, march_max=1, drain_flush=d) for d in (1, 64)]


@functools.lru_cache(maxsize=None)
def tree_of(basis_dim):
    return common.small_scene(depth=5, basis_dim=basis_dim, seed=40 + basis_dim)


def cameras(shape):
    size, radius = SHAPES[shape]
    cams = [common.camera_for(pose_idx=i, n_poses=8, size=size, radius=radius) for i in POSES]
    return [c[0] for c in cams], size, cams[0][3]


@functools.lru_cache(maxsize=None)
def hit_maps(basis_dim, shape, fp_mode):
    """Hit samples per pixel of the three frames, uint32 [3, size, size]."""
    trs, size, f = cameras(shape)
    th = ob.TreeHandle(tree_of(basis_dim))
    return np.stack([ob.render_maps(th, ob.make_camera(tr, size, size, f), ob.default_options(**OPT), fp_mode)[1]
                     for tr in trs])


@functools.lru_cache(maxsize=None)
def oracle_frames(basis_dim, shape, fp_mode):
    """-> (rgba uint8 [3, size, size, 4], accum float32 [3, size, size, 4]); read-only."""
    trs, size, f = cameras(shape)
    frames = [common.oracle_frame(tree_of(basis_dim), tr, size, size, f, fp_mode, **OPT) for tr in trs]
    out = np.stack([fr[0] for fr in frames]), np.stack([fr[1] for fr in frames])
    for a in out:
        a.setflags(write=False)
    return out


@FP
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("basis_dim", BASES)
def test_cases_queue_what_they_are_meant_to(basis_dim, shape, fp_mode):
    """No GPU.  Rays with >= 8 hit samples in every case (none of them exercises nothing); sparse: at most 15 rays
    of the batch have a hit, so fewer than 64 items can wait at any time (4 per ray), no round before the first
    blocked ray pops anything, and the first round finds a ray that owns 4; dense: frames whose rays nearly all
    hit, several times 64 items each."""
    hits = hit_maps(basis_dim, shape, fp_mode)
    with_hit, deep = int((hits > 0).sum()), int((hits >= 8).sum())
    print(f"SH{basis_dim} {shape} fp{fp_mode}: {with_hit} rays with a hit, {deep} with >= 8, {int(hits.sum())} items")
    assert deep >= 1
    if shape == "sparse":
        assert with_hit <= 15
    else:
        assert (hits > 0).reshape(3, -1).sum(1).min() >= 128 and hits.reshape(3, -1).sum(1).min() >= 4 * 64


@pytest.mark.gpu
@FP
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("basis_dim", BASES)
def test_shade_rounds_give_the_oracles_bits(basis_dim, shape, fp_mode):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from volrend_amd import api
    trs, size, f = cameras(shape)
    want_rgba, want_acc = oracle_frames(basis_dim, shape, fp_mode)
    assert (want_acc[..., 3] > 0).any(), "the object must be in view"
    t = api.N3Tree.from_synth(tree_of(basis_dim))
    try:
        for knobs in KNOBS:
            t.set_tuning(**knobs)
            imgs = torch.zeros((3, size, size, 4), dtype=torch.uint8, device="cuda")
            accs = torch.zeros((3, size, size, 4), dtype=torch.float32, device="cuda")
            api.launch_renderer_batch(t, api.Camera(size, size, f, f), trs, api.RenderOptions(**OPT), list(imgs), None,
                                      True, accums=list(accs), fp_mode=fp_mode)
            torch.cuda.synchronize()
            assert t.status() == 0, knobs
            got_acc = accs.cpu().numpy()
            bad = (got_acc.view(np.uint32) != want_acc.view(np.uint32)).any(-1)
            assert not bad.any(), (knobs, f"{int(bad.sum())} of {bad.size} accumulators differ", np.argwhere(bad)[:4])
            assert np.array_equal(imgs.cpu().numpy(), want_rgba), knobs
    finally:
        t.free_device()
