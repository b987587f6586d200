"""-m gpu: vr_quantize against the numpy restatement of tests/quantize_util.py, bit for bit: the raw C call over
data arrays of every shape the definition distinguishes (every output sized exactly, poisoned beforehand, with a guard
band behind it that must keep its bits; the workspace poisoned as well), the same bits from two streams, the decode of
the outputs, and through Python: N3Tree.quantize, N3Tree.save -> open, SparseTreeOptimizer.save."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import quantize_util as qz
from tests import update_util as uu
from volrend_amd import _abi, api

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512
OUTPUTS = ("quant_colors", "quant_map", "sigma", "data_retained")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


class Guarded:
    """A device buffer of exactly ``nbytes`` bytes, poisoned, with a poisoned guard band behind it."""

    def __init__(self, torch, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.raw.data_ptr()

    def bits(self):
        host = self.raw.cpu().numpy()
        assert (host[self.nbytes:] == POISON).all(), "a store went beyond the end of an output"
        return host[:self.nbytes].view(np.uint16)


def run_quantize(torch, data, retain, bits, thresh, stream=None, poison=POISON):
    """vr_quantize on ``stream`` (None: the null stream) -> dict name -> uint16 host array, shaped as the restatement's;
    the device buffers stay alive in "_dev" for the tests that hand them on."""
    n_slots, dim = data.shape
    n_quant = (dim - 1) // 3 - retain
    data_dev = torch.from_numpy(data.copy()).cuda()
    shapes = {"quant_colors": (n_quant, qz.ROWS, 3), "quant_map": (n_quant, n_slots), "sigma": (n_slots,),
              "data_retained": (retain, n_slots, 3)}
    bufs = {k: Guarded(torch, 2 * int(np.prod(s))) for k, s in shapes.items() if k != "data_retained" or retain}
    need = _abi.lib().vr_quantize_workspace(n_slots, dim)
    assert need > 0
    work = torch.full((need + 256 + GUARD,), poison, dtype=torch.uint8, device="cuda")
    base = (work.data_ptr() + 255) // 256 * 256
    q = _abi.VrQuantize()
    q.data = data_dev.data_ptr()
    for k, b in bufs.items():
        setattr(q, k, b.ptr)
    q.workspace, q.workspace_bytes = base, need
    q.n_slots, q.data_dim, q.n_retained, q.bits, q.sigma_thresh = n_slots, dim, retain, bits, thresh
    torch.cuda.synchronize()
    _abi.check(_abi.lib().vr_quantize(C.byref(q), None if stream is None else stream.cuda_stream))
    torch.cuda.synchronize()
    tail = work.cpu().numpy()[base - work.data_ptr() + need:]
    assert (tail == poison).all(), "a store went beyond the end of the workspace"
    assert np.array_equal(data_dev.cpu().numpy().view(np.uint16), data.view(np.uint16))       # the input stands
    got = {k: bufs[k].bits().reshape(shapes[k]) if k in bufs else None for k in OUTPUTS}
    got["_dev"] = (data_dev, bufs)
    return got


def assert_same(got, want):
    for k in OUTPUTS:
        if want[k] is None:
            assert got[k] is None
            continue
        w = want[k].view(np.uint16)
        bad = np.flatnonzero(got[k].reshape(-1) != w.reshape(-1))
        assert bad.size == 0, f"{k}: {bad.size} of {w.size} words differ, the first at {np.unravel_index(bad[0], w.shape)}"


# (kind, seed, n_slots, data_dim, kept, retained, bits, sigma_thresh): data_dim 4 / 13 / 28 / 49, bits 1 / 5 / 16,
# retained 0 / 1 / n_basis - 1, 8 / 8 * 37 / 8 * 1031 slots, kept counts 0, 1, 2, 2^bits, 2^bits + 1 and odd ones;
# "special": duplicates, equal ranges on two axes, +-0, subnormals, +-65504, a sigma at the threshold and a NaN one.
CASES = [
    ("special", 1, 8, 4, 0, 0, 1, 2.0),
    ("special", 2, 8, 4, 1, 0, 5, 2.0),
    ("special", 3, 8, 13, 2, 1, 1, 2.0),
    ("special", 4, 8, 13, 3, 3, 1, 2.0),
    ("special", 5, 8, 49, 8, 0, 16, 2.0),
    ("random", 6, 8 * 37, 28, 32, 0, 5, 2.0),
    ("special", 7, 8 * 37, 28, 33, 1, 5, 2.0),
    ("special", 8, 8 * 37, 49, 131, 15, 16, 2.0),
    ("special", 9, 8 * 37, 13, 8 * 37, 0, 5, 2.0),
    ("random", 10, 8 * 37, 4, 1, 0, 16, 2.0),
    ("random", 11, 8 * 1031, 49, 3001, 1, 5, 2.0),
    ("special", 12, 8 * 1031, 28, 3001, 8, 16, 2.0),
    ("special", 13, 8 * 1031, 13, 2001, 0, 16, 2.0),
    ("random", 14, 8 * 1031, 4, 4097, 0, 1, 2.0),
    ("special", 15, 8 * 1031, 13, 100, 1, 5, -5.0),
    ("random", 16, 8 * 1031, 13, 0, 3, 16, 2.0),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_quantize_matches_the_restatement(torch_cuda, case):
    data, want = qz.case(*case)
    got = run_quantize(torch_cuda, data, case[5], case[6], case[7])
    assert_same(got, want)
    assert got["quant_map"].max(initial=0) < 2 ** case[6]


def test_the_cases_are_what_they_were_chosen_for():
    kept = lambda c: int(qz.kept_slots(qz.case(*c)[0], c[7]).sum())
    assert [kept(c) for c in CASES[:5]] == [0, 1, 2, 3, 8] and kept(CASES[14]) == 8 * 1031 - 1   # all but the NaN sigma
    data = qz.case(*CASES[7])[0]
    assert np.isnan(data[:, -1].astype(np.float32)).sum() == 1 and (data[:, -1] == np.float16(2.0)).any()
    pts = qz.channels(data, 15)[qz.kept_slots(data, 2.0)]
    assert np.unique(pts.view(np.uint16), axis=0).shape[0] <= 3                      # ties go by slot index
    r = qz.channels(data, 0).astype(np.float64)
    assert np.ptp(r[:, 0]) == np.ptp(r[:, 1]) == 131008.0                            # equal ranges; +-65504
    bits = data.view(np.uint16)
    assert (bits == 0x8000).any() and (bits == 0).any() and ((bits & 0x7FFF) == 1).any()


def test_two_streams_and_two_workspaces_give_the_same_bits(torch_cuda):
    torch = torch_cuda
    case = CASES[11]
    data, want = qz.case(*case)
    a = run_quantize(torch, data, case[5], case[6], case[7], stream=torch.cuda.Stream(), poison=0x00)
    b = run_quantize(torch, data, case[5], case[6], case[7], stream=torch.cuda.Stream(), poison=0xFF)
    assert_same(a, want)
    assert_same(b, want)


def _device_decode(torch, got, n_slots, dim, retain):
    """vr_decode_quantized of the device outputs of a run_quantize -> uint16 [n_slots, dim]."""
    _, bufs = got["_dev"]
    d = _abi.VrTreeDesc()
    _abi.lib().vr_default_tree_desc(C.byref(d))
    d.N, d.capacity, d.data_dim, d.memory = 2, n_slots // 8, dim, 1
    qd = _abi.VrQuantDesc()
    qd.quant_colors, qd.quant_map, qd.sigma = bufs["quant_colors"].ptr, bufs["quant_map"].ptr, bufs["sigma"].ptr
    qd.n_quant, qd.n_retained = (dim - 1) // 3 - retain, retain
    if retain:
        qd.data_retained = bufs["data_retained"].ptr
    out = Guarded(torch, n_slots * dim * 2)
    _abi.check(_abi.lib().vr_decode_quantized(C.byref(d), C.byref(qd), out.ptr))
    torch.cuda.synchronize()
    return out.bits().reshape(n_slots, dim)


@pytest.mark.parametrize("case", [CASES[7], CASES[10], CASES[12]], ids=lambda c: "-".join(map(str, c)))
def test_the_outputs_decode(torch_cuda, case):
    data, want = qz.case(*case)
    n_slots, dim, retain = case[2], case[3], case[5]
    got = run_quantize(torch_cuda, data, retain, case[6], case[7])
    dec = _device_decode(torch_cuda, got, n_slots, dim, retain)
    host = api._decode_arrays(want["quant_colors"], want["quant_map"], want["sigma"], want["data_retained"], dim)
    assert np.array_equal(dec, host.view(np.uint16))
    if case is CASES[7]:                                             # 131 kept slots, 2^16 boxes: lossless
        kept = qz.kept_slots(data, case[7])
        assert np.array_equal(dec.view(np.float16)[kept].astype(np.float32), data[kept].astype(np.float32))


def _frame(torch, t):
    tr, w, h, f = common.camera_for(pose_idx=2, size=64)
    cam = api.Camera(w, h, f, f)
    cam.transform = np.asarray(tr, dtype=np.float32)
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    api.launch_renderer(t, cam, api.RenderOptions(), img, None, torch.cuda.current_stream(), True)
    torch.cuda.synchronize()
    assert t.status() == 0
    return img.cpu().numpy()


def test_a_quantised_upload_of_the_outputs_renders_the_decode(torch_cuda):
    torch = torch_cuda
    tree = common.small_scene(depth=4, basis_dim=4, seed=44)
    data = np.ascontiguousarray(tree.data.reshape(-1, tree.data_dim))
    got = run_quantize(torch, data, 1, 5, 2.0)
    assert_same(got, qz.restate(data, 1, 5, 2.0))
    arrays = {k: np.ascontiguousarray(got[k]) for k in OUTPUTS}
    a = api.N3Tree()
    a._set_arrays(tree.child, None, tree.offset, tree.invradius3, tree.data_format, None, data_dim=tree.data_dim)
    a.quant_ = {"quant_colors": arrays["quant_colors"].view(np.float16), "quant_map": arrays["quant_map"],
                "sigma": arrays["sigma"].view(np.float16), "data_retained": arrays["data_retained"].view(np.float16)}
    a.load_device()                                                  # vr_tree_upload_quantized
    decoded = api._decode_arrays(a.quant_["quant_colors"], a.quant_["quant_map"], a.quant_["sigma"],
                                 a.quant_["data_retained"], tree.data_dim).reshape(tree.data.shape)
    b = api.N3Tree.from_arrays(tree.child, decoded, tree.offset, tree.invradius3, tree.data_format)
    try:
        fa, fb = _frame(torch, a), _frame(torch, b)
        assert fa[..., :3].any() and np.array_equal(fa, fb)
    finally:
        a.free_device()
        b.free_device()


def test_through_python(torch_cuda, tmp_path):
    torch = torch_cuda
    tree = common.small_scene(depth=4, basis_dim=9, seed=45)
    t = api.N3Tree.from_synth(tree)
    back = None
    try:
        stored = t.read_data().cpu().numpy().reshape(-1, tree.data_dim)
        kw = dict(bits=6, retain=2, sigma_thresh=1.5)
        want = qz.restate(stored, 2, 6, 1.5)
        q = t.quantize(**kw)
        assert q["quant_map"].shape == (7, stored.shape[0]) and q["quant_colors"].shape == (7, 65536, 3)
        assert_same({k: q[k].cpu().numpy().view(np.uint16) for k in OUTPUTS}, want)
        q2 = api.quantize(torch.from_numpy(stored.copy()).cuda(), **kw)                    # a bare data tensor
        assert_same({k: q2[k].cpu().numpy().view(np.uint16) for k in OUTPUTS}, want)
        path = str(tmp_path / "quantised.npz")
        t.save(path, quantize=kw)
        z = np.load(path)
        cap = tree.capacity
        assert z["quant_colors"].shape == (7, 65536, 3) and z["quant_map"].shape == (7, cap, 2, 2, 2)
        assert z["sigma"].shape == (cap, 2, 2, 2) and z["data_retained"].shape == (2, cap, 2, 2, 2, 3)
        assert z["quant_map"].dtype == np.uint16 and "data" not in z.files
        assert np.array_equal(z["parent_depth"], t.parent_depth().cpu().numpy())
        back = api.N3Tree(path)
        dec = api._decode_arrays(want["quant_colors"], want["quant_map"], want["sigma"], want["data_retained"],
                                 tree.data_dim)
        assert np.array_equal(back.read_data().cpu().numpy().reshape(-1, tree.data_dim).view(np.uint16),
                              dec.view(np.uint16))
        plain = str(tmp_path / "plain.npz")
        t.clear_cpu_memory()
        t.save(plain)                                                # the device's values
        assert np.array_equal(np.load(plain)["data"].reshape(-1, tree.data_dim).view(np.uint16), stored.view(np.uint16))
    finally:
        t.free_device()
        if back is not None:
            back.free_device()


def test_optimizer_save(torch_cuda, tmp_path):
    torch = torch_cuda
    from tests import rays_util
    from volrend_amd import optim
    c = uu.case("sh9")
    o, d = (uu.dev(torch, x) for x in rays_util.rays_of_camera(c["trs"][0], c["w"], c["h"], c["f"])[:2])
    target = torch.full((o.shape[0], 3), 0.25, dtype=torch.float32, device="cuda")
    t = uu.upload("sh9")
    opened = []
    try:
        opt = optim.SparseTreeOptimizer(t, "sgd", lr=0.05, lr_sigma=0.3)
        before = t.read_data().cpu().numpy()
        opt.fit(o, d, target)
        opt.step()
        plain, quant = str(tmp_path / "plain.npz"), str(tmp_path / "quant.npz")
        opt.save(plain)
        opt.save(quant, quantize=dict(bits=8))
        now = t.read_data().cpu().numpy()
        assert not np.array_equal(now.view(np.uint16), before.view(np.uint16))             # the step moved values
        assert np.array_equal(np.load(plain)["data"].view(np.uint16), now.view(np.uint16))   # ... and the file has them
        for path in (plain, quant):
            opened.append(api.N3Tree(path))
            assert opened[-1].capacity == t.capacity and opened[-1].data_format == t.data_format
        want = qz.restate(now.reshape(-1, t.data_dim), 1, 8, 2.0)
        dec = api._decode_arrays(want["quant_colors"], want["quant_map"], want["sigma"], want["data_retained"], t.data_dim)
        assert np.array_equal(opened[1].read_data().cpu().numpy().reshape(-1, t.data_dim).view(np.uint16),
                              dec.view(np.uint16))
    finally:
        t.free_device()
        for x in opened:
            x.free_device()
