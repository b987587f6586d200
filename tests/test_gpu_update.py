"""vr_tree_update_data / vr_tree_read_data on the GPU.  Everything is bit-exact: the expected side is the file's own
array or a FRESH upload of the new data (a path the other tests pin to the oracle); one case compares the updated
tree's frame with the oracle directly.

The scenes' own data has density only in the finest leaves, so the trees here carry one of two seeded data sets
(tests/update_util.py variant): between them sigma crosses sigma_thresh in both directions in leaves whose sigma
lives in top-grid entries, in brick entries and in node words only -- each test asserts that of its data."""
import functools

import numpy as np
import pytest

from tests import common
from tests import update_util as uu
from tests.update_util import dev, upload

pytestmark = pytest.mark.gpu
FP_MODES = (0, 1)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def bits16(x):
    return x.cpu().numpy().view(np.uint16)


def render(torch, t, name, pose=0, fp_mode=0, stream=None):
    from volrend_amd import api
    c = uu.case(name)
    cam = api.Camera(c["w"], c["h"], c["f"], c["f"])
    cam.transform = c["trs"][pose]
    img = torch.zeros((c["h"], c["w"], 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((c["h"], c["w"], 4), dtype=torch.float32, device="cuda")
    api.launch_renderer(t, cam, api.RenderOptions(), img, None, torch.cuda.current_stream() if stream is None else stream,
                        True, accum=acc, fp_mode=fp_mode)
    return img, acc


def observe(torch, t, name):
    """Every output an update has to carry, as numpy: frames and accumulators in both FP modes, a grid query, the leaf
    weights of two poses in both FP modes, the read-back."""
    from volrend_amd import api
    c = uu.case(name)
    out = {}
    for fp in FP_MODES:
        img, acc = render(torch, t, name, 0, fp)
        out[f"rgba{fp}"], out[f"accum{fp}"] = img, acc
        w = t.accumulate_weights(api.Camera(c["w"], c["h"], c["f"], c["f"]), c["trs"], api.RenderOptions(),
                                 want=("max_weight", "hits"), fp_mode=fp)
        out[f"max_weight{fp}"], out[f"hits{fp}"] = w["max_weight"], w["hits"]
    res = min(2 ** (t.info()["max_depth"] + 1), 64)
    q = t.query_grid((0, 0, 0), (1, 1, 1), (res, res, res), want=("sigma", "depth", "coeffs"), space="tree")
    out.update({f"grid_{k}": v for k, v in q.items()})
    out["read"] = t.read_data()
    torch.cuda.synchronize()
    assert t.status() == 0
    return {k: (v.view(torch.int16) if v.dtype == torch.float16 else v).cpu().numpy() for k, v in out.items()}


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        bad = g.view(np.uint8) != w.view(np.uint8)
        assert not bad.any(), f"{what}: {k} differs from the fresh upload in {int(bad.sum())} of {bad.size} bytes"


@functools.lru_cache(maxsize=None)
def fresh(name, which):
    """What a fresh upload of data set `which` gives: once per session, read-only."""
    import torch
    t = upload(name, uu.variant(name, which))
    try:
        return observe(torch, t, name)
    finally:
        t.free_device()


def assert_flips(t, name, d_from, d_to, all_kinds=False):
    info = t.info()
    f = uu.flips(uu.case(name)["tree"], info["top_levels"], info["brick_levels"], d_from, d_to)
    assert f and all(up > 0 and down > 0 for up, down in f.values()), (name, f)
    if all_kinds:
        assert sorted(f) == [uu.TOP, uu.BRICK, uu.WORD], (name, f)
    return f


# ---- 1. read-back -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", uu.CASES)
def test_read_back_is_the_file(torch_cuda, name):
    torch = torch_cuda
    tree = uu.case(name)["tree"]
    want = uu.stored(tree, tree.data)
    t = upload(name)
    try:
        h = t.read_data()
        f = t.read_data(dtype=torch.float32)
        torch.cuda.synchronize()
        assert h.dtype == torch.float16 and f.dtype == torch.float32 and tuple(h.shape) == tuple(f.shape) == tree.data.shape
        assert np.array_equal(bits16(h.view(torch.int16)), want.view(np.uint16))
        assert np.array_equal(f.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    finally:
        t.free_device()


# ---- 2. update = fresh upload -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("name", uu.CASES)
def test_update_equals_a_fresh_upload(torch_cuda, name, dtype):
    torch = torch_cuda
    v1, v2 = uu.variant(name, 1), uu.variant(name, 2)
    t = upload(name, v1)
    try:
        print(name, "flips (up, down) per kind:", assert_flips(t, name, v1, v2, all_kinds=name in ("mixed", "blocked")))
        t.update_data(dev(torch, v2, torch.float32 if dtype == "f32" else None))
        got = observe(torch, t, name)
    finally:
        t.free_device()
    assert_same(got, fresh(name, 2), f"{name} {dtype}")
    assert np.array_equal(got["read"].view(np.uint16), uu.stored(uu.case(name)["tree"], v2).view(np.uint16))
    assert not np.array_equal(got["rgba0"], fresh(name, 1)["rgba0"]), "the two data sets render the same frame"


def test_updated_frame_equals_the_oracle(torch_cuda):
    torch = torch_cuda
    name = "sh16"
    c = uu.case(name)
    v2 = uu.variant(name, 2)
    t = upload(name)
    try:
        t.update_data(dev(torch, v2))
        for fp in FP_MODES:
            img, acc = render(torch, t, name, 1, fp)
            torch.cuda.synchronize()
            rgba_o, acc_o, cnt = common.oracle_frame(uu.with_data(c["tree"], v2), c["trs"][1], c["w"], c["h"], c["f"], fp)
            assert cnt["hit_samples"] > 0
            assert np.array_equal(img.cpu().numpy(), rgba_o)
            assert np.array_equal(acc.cpu().numpy().view(np.uint32), acc_o.view(np.uint32))
        assert t.status() == 0
    finally:
        t.free_device()


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_an_array_off_the_16_byte_grid(torch_cuda, dtype):
    """An array that is not 16-byte aligned takes the element-wide kernels, in both directions."""
    torch = torch_cuda
    name = "sh16"
    tree = uu.case(name)["tree"]
    v2 = uu.variant(name, 2)
    td = torch.float32 if dtype == "f32" else torch.float16
    n = v2.size
    src = torch.zeros(n + 8, dtype=td, device="cuda")
    dst = torch.full((n + 8,), 3.0, dtype=td, device="cuda")
    src[1:n + 1] = dev(torch, v2.reshape(-1), td)
    assert src[1:n + 1].data_ptr() % 16 != 0
    t = upload(name)
    try:
        t.update_data(src[1:n + 1])
        t.read_data(out=dst[1:n + 1])
        img, acc = render(torch, t, name)
        torch.cuda.synchronize()
        want = uu.stored(tree, v2).reshape(-1)
        got = dst.cpu().numpy()
        assert got[0] == 3.0 and (got[n + 1:] == 3.0).all(), "written outside the array"
        assert np.array_equal(got[1:n + 1].astype(np.float16).view(np.uint16), want.view(np.uint16))
        assert np.array_equal(img.cpu().numpy(), fresh(name, 2)["rgba0"])
        assert np.array_equal(acc.cpu().numpy().view(np.uint32), fresh(name, 2)["accum0"].view(np.uint32))
    finally:
        t.free_device()


# ---- 3. rounding ------------------------------------------------------------------------------------------
def test_float32_rounds_like_numpy(torch_cuda):
    """update_data(float32) stores numpy.astype(float16): ties to even, subnormal halves, overflow to +-inf, the sign
    of zero; NaN stays NaN.  Renders nothing."""
    torch = torch_cuda
    name = "sh16"
    tree = uu.case(name)["tree"]
    rng = np.random.default_rng(5)
    a = np.array(uu.variant(name, 1), np.float32).reshape(-1)
    # random binary32 values across the binary16 range (and below it), all 23 fraction bits in use
    k = a.size // 2
    a[rng.choice(a.size, k, replace=False)] = (rng.standard_normal(k) * 2.0 ** rng.integers(-30, 17, k)).astype(np.float32)
    edges = uu.edge_values()
    at = rng.choice(a.size, 64 * edges.size, replace=False)
    a[at] = np.tile(edges, 64)
    a = a.reshape(tree.data.shape)
    sig = np.flatnonzero(np.asarray(tree.child).reshape(-1) == 0)[:edges.size]     # ... and in the sigma of leaves
    a.reshape(-1, tree.data_dim)[sig, -1] = edges
    with np.errstate(over="ignore"):
        want = uu.stored(tree, a.astype(np.float16))
    t = upload(name)
    try:
        t.update_data(dev(torch, a))
        got = t.read_data()
        wide = t.read_data(dtype=torch.float32)
        torch.cuda.synchronize()
        got, wide = got.cpu().numpy(), wide.cpu().numpy()
    finally:
        t.free_device()
    nan = np.isnan(want)
    # (64 copies of each edge value, less the few that fell on the sigma of an internal slot)
    assert nan.sum() >= 48 and np.isinf(want).sum() >= 48 * 12 and (want.view(np.uint16) == 0x8000).sum() >= 48 * 4
    assert np.isnan(got[nan]).all() and np.isnan(wide[nan]).all()
    bad = (got.view(np.uint16) != want.view(np.uint16)) & ~nan
    assert not bad.any(), (int(bad.sum()), a[bad][:8], got[bad][:8], want[bad][:8])
    assert np.array_equal(wide.view(np.uint32)[~nan], want.astype(np.float32).view(np.uint32)[~nan])


# ---- 4. no residue ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "blocked", "n4", "n4_sh9", "sg22"])
def test_there_and_back_leaves_no_residue(torch_cuda, name):
    torch = torch_cuda
    tree = uu.case(name)["tree"]
    t = upload(name)   # A: the scene's own data
    try:
        before = observe(torch, t, name)
        t.update_data(dev(torch, uu.variant(name, 2)))
        middle = render(torch, t, name)[0]
        t.update_data(dev(torch, tree.data, torch.float32))
        after = observe(torch, t, name)
        assert not np.array_equal(middle.cpu().numpy(), before["rgba0"])
        # update(read(tree)) changes nothing either
        t.update_data(t.read_data())
        again = observe(torch, t, name)
    finally:
        t.free_device()
    assert_same(after, before, f"{name} A -> B -> A")
    assert_same(again, before, f"{name} update(read)")
    assert np.array_equal(before["read"].view(np.uint16), uu.stored(tree, tree.data).view(np.uint16))


# ---- 5. ordering ------------------------------------------------------------------------------------------
def test_same_stream_and_one_event(torch_cuda):
    """A render enqueued on the update's stream right behind it shows the new values without any host
    synchronisation; so does a render on a second stream that waits for one event recorded behind the update."""
    torch = torch_cuda
    name = "mixed"
    v1, v2 = uu.variant(name, 1), uu.variant(name, 2)
    t = upload(name, v1)
    try:
        c = uu.case(name)
        t.reserve(c["w"], c["h"], 1)
        data = dev(torch, v2)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        t.read_data(stream=s1)          # (the tables: the one host-blocking step is behind us)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            t.update_data(data, stream=s1)
            img1, acc1 = render(torch, t, name, stream=s1)
            ev = torch.cuda.Event()
            ev.record(s1)
        with torch.cuda.stream(s2):
            s2.wait_event(ev)
            img2, acc2 = render(torch, t, name, stream=s2)
        torch.cuda.synchronize()
        assert t.status() == 0
        want = fresh(name, 2)
        for img, acc, what in ((img1, acc1, "same stream"), (img2, acc2, "second stream")):
            assert np.array_equal(img.cpu().numpy(), want["rgba0"]), what
            assert np.array_equal(acc.cpu().numpy().view(np.uint32), want["accum0"].view(np.uint32)), what
        assert not np.array_equal(want["rgba0"], fresh(name, 1)["rgba0"])
    finally:
        t.free_device()


# ---- 6. clones and quantised uploads ----------------------------------------------------------------------
def test_clone_after_an_update_and_update_of_a_clone(torch_cuda):
    torch = torch_cuda
    name = "mixed"
    v1, v2 = uu.variant(name, 1), uu.variant(name, 2)
    t = upload(name, v1)
    clone = None
    try:
        t.update_data(dev(torch, v2))
        clone = t.clone_to(torch.cuda.current_device())
        assert_same(observe(torch, clone, name), fresh(name, 2), "clone of an updated tree")
        clone.update_data(dev(torch, v1, torch.float32))     # the clone makes its own tables
        assert_same(observe(torch, clone, name), fresh(name, 1), "updated clone")
        assert_same(observe(torch, t, name), fresh(name, 2), "the source of the clone")
    finally:
        t.free_device()
        if clone is not None:
            clone.free_device()


def test_quantised_upload_accepts_an_update(torch_cuda, tmp_path):
    torch = torch_cuda
    from volrend_amd import api
    name = "basis1"     # depth 4, three basis functions: one retained, two with exact codebooks
    tree = uu.case(name)["tree"]
    path = str(tmp_path / "quantised.npz")
    common.write_quantised_npz(tree, path, n_retain=1, compressed=False)
    t = api.N3Tree(path)
    try:
        assert t.data_ is None and t.quant_ is not None      # decoded on the device: no host data array
        got = t.read_data()
        torch.cuda.synchronize()
        assert np.array_equal(bits16(got.view(torch.int16)), uu.stored(tree, tree.data).view(np.uint16))
        t.update_data(dev(torch, uu.variant(name, 2)))
        assert_same(observe(torch, t, name), fresh(name, 2), "quantised upload, updated")
    finally:
        t.free_device()


# ---- 7. bookkeeping ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "sh16", "n4"])
def test_the_first_call_keeps_two_tables(torch_cuda, name):
    torch = torch_cuda
    from volrend_amd import api
    tree = uu.case(name)["tree"]
    for first in ("read", "update"):
        t = upload(name)
        try:
            info = t.info()
            bricks = uu.n_bricks(tree, info["top_levels"], info["brick_levels"])
            if name == "mixed":
                assert bricks > 0
            if name == "n4":
                assert bricks == 0 and info["top_levels"] == 0
            # the file-order table, 4 bytes per node, and the brick-root table, 4 bytes per brick
            grown = 4 * tree.capacity + 4 * bricks
            data = dev(torch, uu.variant(name, 2))
            t.read_data() if first == "read" else t.update_data(data)
            assert t.info()["device_bytes"] == info["device_bytes"] + grown, (name, first)
            t.update_data(data)
            t.read_data(dtype=torch.float32)
            t.accumulate_weights(api.Camera(8, 8, 10.0, 10.0), [], api.RenderOptions())   # shares the file-order table
            torch.cuda.synchronize()
            assert t.info()["device_bytes"] == info["device_bytes"] + grown, (name, first)
            assert t.status() == 0
        finally:
            t.free_device()
