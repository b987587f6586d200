"""vr_render_backward on the GPU against the float64 restatement of the formulas (tests/cpp/grad_restatement.c,
tied to the oracle and to central differences by tests/test_grad_restatement.py).

Per element of grad_data: |gpu - f64| <= K * unit, unit = 2^-24 M (+ 2^-126 U where binary32 underflows:
tests/grad_util.py unit()), K = 4 * K32 = 148 -- no element is left out.  The buffers start from a sentinel
pattern, so an element no hit sample touches must still hold the caller's bits.

The value domain (section 8): saturated colours, edge densities and non-finite records and gradients, judged
with the edge-aware unit (tests/grad_util.py unit_edge(), K_EDGE = 4 * K32_EDGE = 116) on the clean elements --
those of the slots that no ray outside the formulas hits."""
import numpy as np
import pytest

from tests import common
from tests import grad_util as gu
from tests.grad_util import assert_contained, assert_edge_parity, assert_parity, sentinel, upload, upload_edge

pytestmark = pytest.mark.gpu
FP = pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def backward(torch, t, ref, fp_mode, g=None, trs=None, grad_data=None, stream=None, opt=None):
    from volrend_amd import api
    g = ref["g"] if g is None else g
    g_dev = g if hasattr(g, "is_contiguous") else torch.from_numpy(np.array(g, np.float32)).cuda()
    return t.render_backward(api.Camera(ref["w"], ref["h"], ref["f"], ref["f"]), ref["trs"] if trs is None else trs,
                             api.RenderOptions(**(ref["opt"] if opt is None else opt)), g_dev, grad_data=grad_data,
                             fp_mode=fp_mode, stream=stream)


# ---- 5. parity ------------------------------------------------------------------------------------------
@FP
@pytest.mark.parametrize("name,size,n,optset,gkind", gu.PARITY_CASES,
                         ids=[f"{c[0]}-{c[3]}-{c[4]}" for c in gu.PARITY_CASES])
def test_parity_with_the_float64_formulas(torch_cuda, name, size, n, optset, gkind, fp_mode):
    torch = torch_cuda
    ref = gu.reference(name, optset, fp_mode, n, size, gkind)
    t = upload(ref, name)
    try:
        got = backward(torch, t, ref, fp_mode)
        torch.cuda.synchronize()
        assert t.status() == 0
        assert tuple(got.shape) == ref["grad"].shape and got.dtype == torch.float32
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert (ref["mag"] > 0).sum() > 200, "the case shows nothing"
    assert_parity(got, ref, what=f"{name} {optset} {gkind} fp{fp_mode}")


# ---- 6. edges of the launch -----------------------------------------------------------------------------
@FP
@pytest.mark.parametrize("w,h", [(8, 5), (67, 3)], ids=["8x5", "67x3"])
def test_frames_smaller_than_a_wave_and_ragged(torch_cuda, w, h, fp_mode):
    torch = torch_cuda
    tree = gu.tree_of("sh16")[0]
    tr = gu.poses(1, size=96)[0]
    f = 20.0   # (wide enough for these few pixels to look into the volume)
    trace = gu.Trace(tree, tr, w, h, f, fp_mode)
    g = gu.upstream("normal", 1, h, w, seed=3)
    grad, mag, under = trace.backward64(gu.data64_of(tree), g[0].astype(np.float64))
    ref = dict(tree=tree, ndc=None, trs=[tr], w=w, h=h, f=f, g=g, grad=grad, mag=mag, under=under, opt={})
    assert (mag > 0).sum() > 100
    t = upload(ref)
    try:
        got = backward(torch, t, ref, fp_mode)
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert_parity(got, ref, what=f"{w}x{h} fp{fp_mode}")


@FP
def test_one_call_three_calls_two_streams(torch_cuda, fp_mode):
    """3 poses at 24 x 24: one call == one call per pose == a split over two streams, within 2 K units (both
    sides carry the error); each of them within K of float64."""
    torch = torch_cuda
    ref = gu.reference("sh16", "default", fp_mode, 3, 24)
    t = upload(ref)
    try:
        t.reserve(ref["w"], ref["h"], 3)
        g = torch.from_numpy(np.array(ref["g"])).cuda()
        one = backward(torch, t, ref, fp_mode, g=g)
        three = None
        for i in range(3):
            three = backward(torch, t, ref, fp_mode, g=g[i:i + 1], trs=ref["trs"][i:i + 1], grad_data=three)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        split = torch.zeros_like(one)
        torch.cuda.synchronize()
        for s, (lo, hi) in zip(streams, ((0, 2), (2, 3))):
            with torch.cuda.stream(s):
                backward(torch, t, ref, fp_mode, g=g[lo:hi], trs=ref["trs"][lo:hi], grad_data=split, stream=s)
        torch.cuda.synchronize()
        assert t.status() == 0
        one, three, split = (x.cpu().numpy() for x in (one, three, split))
    finally:
        t.free_device()
    unit = gu.unit(ref)
    pos = ref["mag"] > 0
    for what, other in (("three calls", three), ("two streams", split)):
        assert_parity(other, ref, what=what)
        d = np.abs(one.astype(np.float64) - other.astype(np.float64))
        assert (d[pos] <= 2 * gu.K * unit[pos]).all() and (d[~pos] == 0).all(), what
    assert_parity(one, ref, what="one call")


def test_no_frames_launches_nothing(torch_cuda):
    torch = torch_cuda
    from volrend_amd import api
    ref = gu.reference("sh4", "default", 0, 1, 40)
    t = upload(ref)
    try:
        start = sentinel(ref["grad"].shape)
        buf = torch.from_numpy(start.copy()).cuda()
        bytes0 = t.info()["device_bytes"]
        g = torch.zeros((0, ref["h"], ref["w"], 4), dtype=torch.float32, device="cuda")
        out = t.render_backward(api.Camera(ref["w"], ref["h"], ref["f"], ref["f"]), [], api.RenderOptions(), g,
                                grad_data=buf)
        torch.cuda.synchronize()
        assert out is buf and t.status() == 0
        assert t.info()["device_bytes"] == bytes0 + 4 * ref["tree"].capacity     # the file-order table, nothing else
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), start.view(np.uint32))
    finally:
        t.free_device()


# ---- 7. what must not be written ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sh16", "basis1", "n4"])
def test_untouched_elements_keep_the_callers_bits(torch_cuda, name):
    torch = torch_cuda
    size, n = next((c[1], c[2]) for c in gu.PARITY_CASES if c[0] == name)
    ref = gu.reference(name, "default", 0, n, size)
    tree = ref["tree"]
    start = sentinel(ref["grad"].shape)
    t = upload(ref)
    try:
        got = backward(torch, t, ref, 0, grad_data=torch.from_numpy(start.copy()).cuda())
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert_parity(got, ref, start=start, what=f"{name} into a sentinel")
    same = got.view(np.uint32) == start.view(np.uint32)
    assert not same.all(), "nothing was written at all"
    interior = np.asarray(tree.child) != 0
    assert interior.any() and same[interior].all(), "a slot of an interior node was written"
    if name == "basis1":
        bd = tree.basis_dim
        unused = np.ones(tree.data_dim, bool)
        unused[[0, bd, 2 * bd, 3 * bd]] = False
        assert same[..., unused].all(), "a coefficient b > 0 of a basis-1 tree was written"
        assert not same[..., ~unused].all()


def test_fog_below_the_threshold_and_zero_gradient(torch_cuda):
    torch = torch_cuda
    # the fog scene with sigma_thresh = 0.5 has no hit sample: nothing is written
    ref = gu.reference("fog", (("sigma_thresh", 0.5),), 0, 1, 40)
    assert not (ref["mag"] > 0).any()
    start = sentinel(ref["grad"].shape)
    t = upload(ref)
    try:
        got = backward(torch, t, ref, 0, grad_data=torch.from_numpy(start.copy()).cuda())
        torch.cuda.synchronize()
        assert t.status() == 0
        assert np.array_equal(got.cpu().numpy().view(np.uint32), start.view(np.uint32))
    finally:
        t.free_device()
    # an all-zero grad_accum leaves every value equal
    ref = gu.reference("sh16", "default", 0, 2, 96, "zero")
    t = upload(ref)
    try:
        got = backward(torch, t, ref, 0, grad_data=torch.from_numpy(start_for(ref)).cuda())
        torch.cuda.synchronize()
        assert t.status() == 0
        assert np.array_equal(got.cpu().numpy(), start_for(ref))
    finally:
        t.free_device()


def start_for(ref):
    return sentinel(ref["grad"].shape).copy()


# ---- 8. the value domain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fp_mode", gu.EDGE_RUNS, ids=gu.EDGE_IDS)
def test_finite_edge_values_match_the_float64_formulas(torch_cuda, name, fp_mode):
    """Saturated colours and edge densities, all finite (the finite catalogue of tests/grad_util.py), into a
    zeroed buffer."""
    torch = torch_cuda
    ref = gu.edge_reference(name, "finite", fp_mode)
    t = upload_edge(ref)
    try:
        got = backward(torch, t, ref, fp_mode)
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert_edge_parity(got, ref, what=f"finite {name} fp{fp_mode}")


@pytest.mark.parametrize("name,fp_mode", gu.EDGE_RUNS, ids=gu.EDGE_IDS)
def test_non_finite_rays_are_contained(torch_cuda, name, fp_mode):
    """NaN and +-inf in records and in grad_accum (the full catalogue), into the sentinel: the call returns, a ray
    that meets none of them and whose binary32 forward is finite leaves what the formulas say, and what no ray
    hits keeps its bits."""
    torch = torch_cuda
    ref = gu.edge_reference(name, "full", fp_mode)
    start = sentinel(ref["grad"].shape)
    t = upload_edge(ref)
    try:
        got = backward(torch, t, ref, fp_mode, grad_data=torch.from_numpy(start.copy()).cuda())
        torch.cuda.synchronize()
        assert t.status() == 0
        got = got.cpu().numpy()
    finally:
        t.free_device()
    assert_contained(got, ref, start, what=f"full {name} fp{fp_mode}")


# ---- 9. the sample guard --------------------------------------------------------------------------------
def test_sample_guard_sets_the_status_bit(torch_cuda):
    """The case of tests/test_gpu_status.py::test_status_word_through_the_api: max_iter = 2 cuts every wave
    whose rays outlive its first pass of march rounds.  The call returns, the bit is set, nothing hangs."""
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=6, basis_dim=9, seed=941)
    tr, w, h, f = common.camera_for(pose_idx=3, size=96)
    t = api.N3Tree.from_synth(tree)
    try:
        g = torch.ones((1, h, w, 4), dtype=torch.float32, device="cuda")
        cam = api.Camera(w, h, f, f)
        full = t.render_backward(cam, [tr], api.RenderOptions(), g)
        torch.cuda.synchronize()
        assert t.status() == 0 and bool((full != 0).any())
        t.set_tuning(max_iter=2)
        cut = t.render_backward(cam, [tr], api.RenderOptions(), g)
        torch.cuda.synchronize()
        assert t.status() & 1, "rays were cut by the guard but the status word says nothing"
        assert t.status(reset=True) & 1 and t.status() == 0
        assert bool(torch.isfinite(cut).all())
    finally:
        t.free_device()


# ---- refusals that need the tree ------------------------------------------------------------------------
def test_tree_dependent_refusals_write_nothing(torch_cuda):
    """SG / ASG trees and a basis_minmax that leaves out a basis function of the tree: VR_ERR_UNSUPPORTED once
    the handle is followed, before any device work -- the buffer keeps its bits, no table is uploaded."""
    torch = torch_cuda
    from volrend_amd import _abi, api
    tr, w, h, f = common.camera_for(size=24)
    cam = api.Camera(w, h, f, f)
    g = torch.ones((1, h, w, 4), dtype=torch.float32, device="cuda")
    cases = [(common.small_scene(depth=4, basis_dim=9, fmt="SG", seed=2), api.RenderOptions(), "SG"),
             (common.small_scene(depth=4, basis_dim=4, fmt="ASG", seed=2), api.RenderOptions(), "SG"),
             (gu.tree_of("sh16")[0], api.RenderOptions(basis_minmax=(0, 8)), "basis_minmax"),
             (gu.tree_of("sh16")[0], api.RenderOptions(basis_minmax=(1, 24)), "basis_minmax")]
    for tree, opts, word in cases:
        t = api.N3Tree.from_synth(tree)
        try:
            start = sentinel(tuple(tree.data.shape))
            buf = torch.from_numpy(start.copy()).cuda()
            bytes0 = t.info()["device_bytes"]
            with pytest.raises(_abi.VolrendError) as e:
                t.render_backward(cam, [tr], opts, g, grad_data=buf)
            torch.cuda.synchronize()
            assert e.value.code == 5 and word in str(e.value) and "vr_render_backward" in str(e.value)
            assert t.info()["device_bytes"] == bytes0
            assert np.array_equal(buf.cpu().numpy().view(np.uint32), start.view(np.uint32))
        finally:
            t.free_device()
    # an RGBA tree has no basis: basis_minmax does not matter
    ref = gu.reference("rgba", "default", 0, 1, 40)
    t = upload(ref)
    try:
        got = backward(torch, t, ref, 0, opt=dict(basis_minmax=(3, 5)))
        torch.cuda.synchronize()
        assert t.status() == 0
        assert_parity(got.cpu().numpy(), ref, what="rgba with a narrowed basis_minmax")
    finally:
        t.free_device()


def test_more_poses_than_one_launch_in_one_python_call(torch_cuda):
    """513 poses at 40 x 40 in one call are two launches, the second reading grad_accum from frame 512 on: 512
    decoys whose every ray misses the box (their grad_accum is finite non-zero garbage), then the real pose with
    the reference's g.  A wrong byte offset reads the garbage, or zeros."""
    torch = torch_cuda
    from volrend_amd import _abi, api
    ref = gu.reference("sh4", "default", 0, 1, 40)
    n, real = _abi.MAX_BATCH, ref["trs"][0]
    decoy = gu.decoy_pose(real)
    g = torch.empty((n + 1, ref["h"], ref["w"], 4), dtype=torch.float32, device="cuda")
    g[:n] = torch.from_numpy(sentinel((ref["h"], ref["w"], 4)) * np.float32(2.0 ** 40)).cuda()   # 1 .. 251
    g[n] = torch.from_numpy(np.array(ref["g"][0])).cuda()
    t = upload(ref)
    try:
        alone = t.accumulate_weights(api.Camera(ref["w"], ref["h"], ref["f"], ref["f"]), [decoy],
                                     api.RenderOptions(**ref["opt"]), want=("max_weight", "hits"))
        one = backward(torch, t, ref, 0)
        many = backward(torch, t, ref, 0, g=g, trs=[decoy] * n + [real])
        torch.cuda.synchronize()
        assert t.status() == 0
        alone = {k: v.cpu().numpy() for k, v in alone.items()}
        one, many = one.cpu().numpy(), many.cpu().numpy()
    finally:
        t.free_device()
    assert not alone["max_weight"].any() and not alone["hits"].any(), "the decoy pose reaches the tree"
    assert_parity(many, ref, what="513 poses")
    worst = float((np.abs(many.astype(np.float64) - one.astype(np.float64)) - 2 * gu.K * gu.unit(ref)).max())
    assert worst <= 0, "513 poses and the real pose alone differ by more than two runs of the atomic sum may"
