"""vr_accumulate_weights on the GPU: per leaf slot, max_weight is bit-equal to and hits equals the
restatement of trace_ray's loop with the per-leaf rule (tests/cpp/weights_restatement.c, tied to the oracle
by tests/test_weights_restatement.py) over EVERY slot of the tree.  The buffers start from a sentinel count
and a known non-negative float, so a slot no ray reached must still hold what the caller put there, and the
counts wrap modulo 2^32."""
import numpy as np
import pytest

from tests import aov_util as au
from tests import common
from tests import weights_util as wu
from tests.weights_util import accumulate, buffers, expected, host

pytestmark = pytest.mark.gpu

FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def check_reference(torch, ref, fp_mode, ndc=None, tuning=None, **opt_kw):
    """Upload, one call with all poses, compare every slot."""
    from volrend_amd import api
    tree, trs, w, h, f, want_mw, want_hits, _ = ref
    t = api.N3Tree.from_synth(tree, ndc=ndc)
    try:
        if tuning:
            t.set_tuning(**tuning)
        mw, hc = accumulate(torch, t, w, h, f, trs, fp_mode, tree=tree, **opt_kw)
        torch.cuda.synchronize()
        assert t.status() == 0
        exp_mw, exp_hits = expected(want_mw, want_hits)
        wu.assert_same_slots(host(mw), host(hc), exp_mw, exp_hits)
    finally:
        t.free_device()
    assert (want_hits == 0).any() and (want_mw > 0).any(), "the case shows nothing"


CASES = wu.TIE_CASES + [("value_edge", "negative")]


@FP
@pytest.mark.parametrize("scene,optset", CASES, ids=[f"{s}-{o}" for s, o in CASES])
def test_every_slot_equals_the_restatement(torch_cuda, scene, optset, fp_mode):
    """Three poses per call at 96 x 96."""
    ref = wu.reference(scene, optset, fp_mode, 3, 96)
    kw = wu.NEGATIVE if optset == "negative" else wu.OPTION_SETS[optset]
    check_reference(torch_cuda, ref, fp_mode, **kw)
    if optset == "negative":
        assert ref[7] > 0, "no hit sample with a weight <= 0 or NaN"


@FP
def test_split_invariance(torch_cuda, fp_mode):
    """One call of 6 poses == 3 calls of 2 on two streams into the same buffers == 6 calls into separate
    buffers merged on the host."""
    torch = torch_cuda
    from volrend_amd import api
    tree, trs, w, h, f, want_mw, want_hits, _ = wu.reference("sh16", "default", fp_mode, 6, 96)
    exp_mw, exp_hits = expected(want_mw, want_hits)
    t = api.N3Tree.from_synth(tree)
    try:
        t.reserve(w, h, 6)
        one = accumulate(torch, t, w, h, f, trs, fp_mode, tree=tree)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        mw, hc = buffers(torch, tree)
        torch.cuda.synchronize()
        for i, lo in enumerate((0, 2, 4)):
            s = streams[i % 2]
            with torch.cuda.stream(s):
                accumulate(torch, t, w, h, f, trs[lo:lo + 2], fp_mode, stream=s, mw=mw, hc=hc)
        parts = []
        for tr in trs:
            a = torch.zeros(wu.slots_shape(tree), dtype=torch.float32, device="cuda")
            b = torch.zeros(wu.slots_shape(tree), dtype=torch.int32, device="cuda")
            parts.append(accumulate(torch, t, w, h, f, [tr], fp_mode, mw=a, hc=b))
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    wu.assert_same_slots(host(one[0]), host(one[1]), exp_mw, exp_hits, "one call")
    wu.assert_same_slots(host(mw), host(hc), exp_mw, exp_hits, "three calls on two streams")
    merged_mw = np.maximum.reduce([host(p[0]) for p in parts])
    merged_hits = np.add.reduce([host(p[1]).view(np.uint32) for p in parts], dtype=np.uint32)   # modulo 2^32
    wu.assert_same_slots(merged_mw, merged_hits, want_mw, want_hits, "six calls merged on the host")
    assert (merged_mw > host(parts[0][0])).any(), "no leaf's maximum comes from a later pose"


@pytest.mark.parametrize("knobs", [dict(waves_per_cu=1, refill_min=1), dict(waves_per_cu=1, refill_min=64, march_max=1),
                                   dict(waves_per_cu=1, refill_min=20, chunk_max=64), dict(weights_check=0),
                                   dict(raygen_waves=4, frame_group=1, xcd_queues=0)],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_refill_chunks_and_knobs_change_nothing(torch_cuda, knobs):
    """8 poses of 96 x 96 on one wave per CU: every wave goes back to the queues several times.  Also the
    always-atomic form of the max (weights_check = 0) and the other ray-generation workgroup size."""
    check_reference(torch_cuda, wu.reference("sh16", "default", 0, 8, 96), 0, tuning=knobs)


@FP
@pytest.mark.parametrize("want", [("max_weight",), ("hits",), ("max_weight", "hits")], ids=["max", "hits", "both"])
def test_either_output_alone(torch_cuda, want, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    tree, trs, w, h, f, want_mw, want_hits, _ = wu.reference("sh9_near", "default", fp_mode, 3, 96)
    t = api.N3Tree.from_synth(tree)
    try:
        # through `want`: the tensors are allocated zeroed by the call
        res = t.accumulate_weights(api.Camera(w, h, f, f), trs, api.RenderOptions(), want=want, fp_mode=fp_mode)
        torch.cuda.synchronize()
        assert t.status() == 0
        assert sorted(res) == sorted(want)
        wu.assert_same_slots(host(res.get("max_weight")), host(res.get("hits")), want_mw, want_hits)
        assert all(tuple(v.shape) == wu.slots_shape(tree) for v in res.values())
    finally:
        t.free_device()


@FP
def test_blocked_brick_order(torch_cuda, fp_mode):
    """Bricks in 4 x 4 x 2 line blocks: depth 7 under a 2^2 top grid with 8^3 bricks, the geometry of
    tests/test_gpu_aov.py::test_blocked_brick_order."""
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=7, basis_dim=4, seed=1201)
    trs, w, h = wu.poses(2, size=72), 72, 72
    f = common.camera_for(size=72)[3]
    want_mw, want_hits, _ = wu.restate(tree, trs, w, h, f, fp_mode)
    api.set_tuning(top_levels=2, brick_levels=3, brick_blocked=1)
    try:
        t = api.N3Tree.from_synth(tree)
    finally:
        api.set_tuning(top_levels=0, brick_levels=3, brick_blocked=-1)
    try:
        assert t.info()["brick_blocked"] == 1
        mw, hc = accumulate(torch, t, w, h, f, trs, fp_mode, tree=tree)
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    wu.assert_same_slots(host(mw), host(hc), *expected(want_mw, want_hits))
    assert (want_mw > 0).sum() > 500


@FP
def test_ndc_tree(torch_cuda, fp_mode):
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=5, basis_dim=4, seed=51)
    w, h, f = 96, 72, 80.0
    tr2 = au.NDC_TRANSFORM.copy()
    tr2[9:12] += np.float32(0.05)
    trs = [au.NDC_TRANSFORM, tr2]
    want_mw, want_hits, _ = wu.restate(tree, trs, w, h, f, fp_mode, ndc=au.NDC)
    t = api.N3Tree.from_synth(tree, ndc=au.NDC)
    try:
        mw, hc = accumulate(torch, t, w, h, f, trs, fp_mode, tree=tree)
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    wu.assert_same_slots(host(mw), host(hc), *expected(want_mw, want_hits))
    assert (want_mw > 0).any()


@FP
def test_26_level_chain_takes_the_descent(torch_cuda, fp_mode):
    """N = 2 but deeper than the lookup reaches: the literal descent, with its own leaf-id arithmetic."""
    torch = torch_cuda
    from volrend_amd import api, _abi
    tree, T = common.deep_chain_tree_n2(depth=26, basis_dim=4, seed=26)
    tr, w, h, f = common.camera_at(T)
    want_mw, want_hits, _ = wu.restate(tree, [tr], w, h, f, fp_mode, step_size=1e-8)
    t = api.N3Tree.from_synth(tree)
    try:
        assert t.info()["query_mode"] == _abi.QUERY_DESCENT
        mw, hc = accumulate(torch, t, w, h, f, [tr], fp_mode, tree=tree, step_size=1e-8)
        torch.cuda.synchronize()
        assert t.status() == 0
    finally:
        t.free_device()
    wu.assert_same_slots(host(mw), host(hc), *expected(want_mw, want_hits))
    assert (want_mw > 0).any()


def test_clone_device_bytes_and_colour_before_and_after(torch_cuda):
    """The table is built by the first call (device_bytes grows by 4 x capacity, not before); a clone builds
    its own and gives the same bits; a colour launch of the tree is the same before and after."""
    torch = torch_cuda
    from volrend_amd import api
    tree, trs, w, h, f, want_mw, want_hits, _ = wu.reference("sh16", "default", 0, 3, 96)
    exp = expected(want_mw, want_hits)
    cam = api.Camera(w, h, f, f)

    def colour(t):
        img = torch.zeros((3, h, w, 4), dtype=torch.uint8, device="cuda")
        api.launch_renderer_batch(t, cam, trs, api.RenderOptions(), list(img), None, True)
        torch.cuda.synchronize()
        return img.cpu().numpy()

    t = api.N3Tree.from_synth(tree)
    c = c2 = None
    try:
        bytes0 = t.info()["device_bytes"]
        before = colour(t)
        assert t.info()["device_bytes"] == bytes0
        c = t.clone_to(0)                                   # cloned before the source has a table
        assert c.info()["device_bytes"] == bytes0
        t.accumulate_weights(cam, [], api.RenderOptions(), want=("hits",))     # the warm-up call: no launch
        assert t.info()["device_bytes"] == bytes0 + 4 * tree.capacity
        mw, hc = accumulate(torch, t, w, h, f, trs, tree=tree)
        torch.cuda.synchronize()
        assert t.info()["device_bytes"] == bytes0 + 4 * tree.capacity
        wu.assert_same_slots(host(mw), host(hc), *exp, "source")
        assert np.array_equal(colour(t), before)
        assert before.any()
        c2 = t.clone_to(0)                                  # cloned after: the clone does not inherit the table
        assert c2.info()["device_bytes"] == bytes0
        for name, cl in (("clone", c), ("late clone", c2)):
            mw, hc = accumulate(torch, cl, w, h, f, trs, tree=tree)
            torch.cuda.synchronize()
            assert cl.info()["device_bytes"] == bytes0 + 4 * tree.capacity
            wu.assert_same_slots(host(mw), host(hc), *exp, name)
            assert cl.status() == 0
        assert t.status() == 0
    finally:
        for x in (t, c, c2):
            if x is not None:
                x.free_device()


def test_sample_guard_sets_the_status_bit(torch_cuda):
    """The case of tests/test_gpu_grad.py::test_sample_guard_sets_the_status_bit (the weights march is the
    backward's first march over the same rays): max_iter = 2 cuts every wave whose rays outlive its first pass
    of march rounds.  The call returns and the bit is set; a cut ray contributes a prefix of its samples, so
    no slot counts more hits or holds a larger weight than after the full march."""
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=6, basis_dim=9, seed=941)
    tr, w, h, f = common.camera_for(pose_idx=3, size=96)
    cam = api.Camera(w, h, f, f)
    want = ("max_weight", "hits")
    t = api.N3Tree.from_synth(tree)
    try:
        full = t.accumulate_weights(cam, [tr], api.RenderOptions(), want=want)
        torch.cuda.synchronize()
        assert t.status() == 0 and bool((full["hits"] != 0).any())
        t.set_tuning(max_iter=2)
        try:
            cut = t.accumulate_weights(cam, [tr], api.RenderOptions(), want=want)
            torch.cuda.synchronize()
            assert t.status() & 1, "rays were cut by the guard but the status word says nothing"
            assert t.status(reset=True) & 1 and t.status() == 0
        finally:
            t.set_tuning(max_iter=1 << 22)
        hits_full, hits_cut = (host(r["hits"]).view(np.uint32) for r in (full, cut))
        mw_full, mw_cut = (host(r["max_weight"]) for r in (full, cut))
        assert (hits_cut <= hits_full).all()
        assert (mw_cut <= mw_full).all()
    finally:
        t.free_device()


def test_more_poses_than_one_launch_in_one_python_call(torch_cuda):
    """513 poses at 40 x 40 in one call are two launches: 512 decoys whose every ray misses the box, then the real
    pose.  The result must be that of the real pose alone, bit for bit: a chunk loop that reuses the first
    chunk's cameras gives zeros."""
    torch = torch_cuda
    from tests import grad_util as gu
    from volrend_amd import _abi, api
    ref = gu.reference("sh4", "default", 0, 1, 40)
    real, both = ref["trs"][0], ("max_weight", "hits")
    decoy = gu.decoy_pose(real)
    cam, opts = api.Camera(ref["w"], ref["h"], ref["f"], ref["f"]), api.RenderOptions(**ref["opt"])
    t = api.N3Tree.from_synth(ref["tree"])
    try:
        runs = [t.accumulate_weights(cam, trs, opts, want=both)
                for trs in ([decoy], [real], [decoy] * _abi.MAX_BATCH + [real])]
        torch.cuda.synchronize()
        assert t.status() == 0
        alone, one, many = ({k: host(v) for k, v in r.items()} for r in runs)
    finally:
        t.free_device()
    for k in both:
        assert not alone[k].any(), f"the decoy pose reaches the tree ({k})"
    assert (one["max_weight"] > 0).any() and one["hits"].any(), "the real pose shows nothing"
    for k in both:
        assert np.array_equal(many[k].view(np.uint32), one[k].view(np.uint32)), k
