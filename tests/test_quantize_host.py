"""vr_quantize without a GPU: the symbols, prototypes and struct layout, every refusal of the header (with pointers
that are never followed) through C, C++ and Python, the workspace size, the properties of the restatement of
tests/quantize_util.py on random data (the loop over boxes agrees with the vectorised form; the lossless case,
containment, codes below 2^bits, the decode of _decode_arrays), and N3Tree.save -> open for both file kinds."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from tests import quantize_util as qz
from volrend_amd import _abi, api, optim

FUNCS = ("vr_quantize", "vr_quantize_workspace")
INVALID = 1


def test_symbols_are_exported_and_prototyped():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for f in FUNCS:
        assert f in exported and f in _abi.PROTOTYPES, f
    assert _abi.lib().vr_abi_version() == 3                       # additive: the version stands
    assert (_abi.QUANT_MAX_BITS, _abi.QUANT_ROWS) == (16, 65536)
    assert api.N3Tree.quantize is api.quantize
    assert callable(api.N3Tree.save) and callable(optim.SparseTreeOptimizer.save)


def test_struct_layout_matches_the_c_compiler():
    got = build_util.c_struct_layout("VrQuantize", _abi.VrQuantize, [("abi", "VR_ABI_VERSION")])
    assert got["size"] == C.sizeof(_abi.VrQuantize)
    for fname, _ in _abi.VrQuantize._fields_:
        assert got[fname] == getattr(_abi.VrQuantize, fname).offset, fname
    assert got["abi"] == 3


# ---- refusals through C: every pointer is junk and must never be followed ----
def _args(**kw):
    q = _abi.VrQuantize()
    q.data, q.quant_colors, q.quant_map, q.sigma, q.data_retained = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    q.workspace, q.n_slots, q.data_dim, q.n_retained, q.bits, q.sigma_thresh = 0x100000, 80, 13, 1, 5, 2.0
    q.workspace_bytes = _abi.lib().vr_quantize_workspace(80, 13)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _refused(arg, match):
    L = _abi.lib()
    rc = L.vr_quantize(None if arg is None else C.byref(arg), None)
    msg = L.vr_last_error().decode()
    assert rc == INVALID and "vr_quantize" in msg and match in msg, (rc, msg)


def test_c_refusals():
    _refused(None, "NULL")
    for field in ("data", "quant_colors", "quant_map", "sigma", "workspace"):
        _refused(_args(**{field: None}), "NULL")
    _refused(_args(data_retained=None), "data_retained")
    _refused(_args(n_retained=0), "data_retained")
    for n in (0, -1, 2 ** 31):
        _refused(_args(n_slots=n), "n_slots")
    for dim in (0, 1, 3, 12, 14, -2):
        _refused(_args(data_dim=dim), "data_dim")
    for r in (-1, 4, 5):
        _refused(_args(n_retained=r), "n_retained")
    _refused(_args(data_dim=4), "n_retained")                      # n_basis = 1: nothing can be retained
    for bits in (0, -1, 17):
        _refused(_args(bits=bits), "bits")
    _refused(_args(sigma_thresh=math.nan), "NaN")
    need = _abi.lib().vr_quantize_workspace(80, 13)
    for size in (need - 1, 0, -5):
        _refused(_args(workspace_bytes=size), "workspace")
    _refused(_args(workspace=0x100000 + 128), "workspace")
    for out in ("quant_colors", "quant_map", "sigma", "data_retained"):
        _refused(_args(**{out: 0x1000}), "input")


def test_workspace_size():
    size = _abi.lib().vr_quantize_workspace
    for n, dim in ((0, 13), (-1, 13), (2 ** 31, 13), (80, 0), (80, 1), (80, 12), (80, -4)):
        assert size(n, dim) == -1, (n, dim)
    ns = [1, 2, 63, 64, 65, 8 * 37, 8 * 1031, 10 ** 6, 10 ** 6 + 1, 2 ** 24, 2 ** 31 - 1]
    sizes = [size(n, 49) for n in ns]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] >= (2 ** 31 - 1) * 24                          # (int64: no wrap at the largest tree)
    assert size(1000, 4) == size(1000, 76)                          # the working set is per basis function


def test_refusals_through_cpp(tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("quantize_refusals", tmp_path), refusals=True)
    want = {"null_data": "NULL", "null_colors": "NULL", "null_map": "NULL", "null_sigma": "NULL",
            "null_workspace": "NULL", "retained_missing": "data_retained", "retained_unwanted": "data_retained",
            "slots_zero": "n_slots", "slots_large": "n_slots", "dim_small": "data_dim", "dim_odd": "data_dim",
            "retain_negative": "n_retained", "retain_all": "n_retained", "bits_zero": "bits", "bits_large": "bits",
            "thresh_nan": "NaN", "workspace_small": "workspace", "workspace_misaligned": "workspace",
            "output_is_input": "input", "size_slots": "refused", "size_dim": "refused"}
    assert sorted(got) == sorted(want)
    for case, text in got.items():
        assert text.startswith("runtime_error: vr_quantize") and want[case] in text, (case, text)


# ---- refusals through Python: before any C call ----
def test_python_refusals():
    data = common.FakeCudaTensor((10, 2, 2, 2, 13), "float16")

    def refused(match, x=data, calls=0, **kw):
        with pytest.raises(ValueError, match=match):
            api.quantize(x, **kw)
    refused("bits", bits=0)
    refused("bits", bits=17)
    refused("bits", bits=5.0)
    refused("bits", bits=True)
    refused("retain", retain=-1)
    refused("retain", retain=4)
    refused("retain", retain=1.0)
    refused("sigma_thresh", sigma_thresh=math.nan)
    refused("sigma_thresh", sigma_thresh="2")
    refused("data_dim", x=common.FakeCudaTensor((80, 12), "float16"))
    refused("data_dim", x=common.FakeCudaTensor((80, 1), "float16"))
    refused("retain", x=common.FakeCudaTensor((80, 4), "float16"))              # RGBA: retain defaults to 1
    refused("slots", x=common.FakeCudaTensor((0, 13), "float16"))
    refused("data must be float16", x=common.FakeCudaTensor((80, 13), "float32"))
    refused("contiguous", x=common.FakeCudaTensor((80, 13), "float16", contiguous=False))
    refused("device", x=common.FakeCudaTensor((80, 13), "float16", is_cuda=False))
    # a tree: its scalars are checked before it is asked anything
    for kw, match in ((dict(bits=0), "bits"), (dict(retain=16), "retain"), (dict(sigma_thresh=math.nan), "sigma_thresh")):
        t = common.FakeTree()
        with pytest.raises(ValueError, match=match):
            api.quantize(t, **kw)
        assert t.info_calls == 0

    class NoHandle:
        @property
        def handle(self):
            raise RuntimeError("tree is not on the device")
    with pytest.raises(RuntimeError, match="not on the device"):
        api.quantize(NoHandle())
    t = api.N3Tree()
    with pytest.raises(ValueError, match="npz"):
        t.save("tree.bin")
    with pytest.raises(ValueError, match="quantize"):
        t.save("tree.npz", quantize={"weighted": True})
    with pytest.raises(ValueError, match="quantize"):
        t.save("tree.npz", quantize=16)


# ---- the restatement's own properties ----
def _decode(want, data_dim):
    return api._decode_arrays(want["quant_colors"], want["quant_map"], want["sigma"], want["data_retained"], data_dim)


@pytest.mark.parametrize("kind,n_slots,dim,n_kept,retain,bits", [
    ("random", 8 * 37, 13, 200, 1, 5), ("special", 8 * 37, 28, 131, 0, 3), ("special", 8 * 37, 13, 296, 3, 16),
    ("random", 64, 4, 33, 0, 1), ("random", 8, 49, 0, 1, 5)])
def test_loop_over_boxes_agrees_with_the_vectorised_restatement(kind, n_slots, dim, n_kept, retain, bits):
    data, want = qz.case(kind, 5, n_slots, dim, n_kept, retain, bits)
    naive = qz.restate(data, retain, bits, 2.0, cut=qz.median_cut_naive)
    for k, v in want.items():
        assert (v is None and naive[k] is None) or np.array_equal(v.view(np.uint16), naive[k].view(np.uint16)), k
    assert int(qz.kept_slots(data, 2.0).sum()) == n_kept


@pytest.mark.parametrize("kind", ["random", "special"])
def test_containment_codes_and_decode(kind):
    n_slots, dim, retain, bits = 8 * 1031, 28, 1, 5
    data, want = qz.case(kind, 9, n_slots, dim, 3001, retain, bits)
    kept = qz.kept_slots(data, 2.0)
    assert want["quant_map"].max() < 2 ** bits and (want["quant_map"][:, ~kept] == 0).all()
    assert (want["sigma"].view(np.uint16)[~kept] == 0).all() and (want["data_retained"].view(np.uint16)[:, ~kept] == 0).all()
    assert (want["quant_colors"].view(np.uint16)[:, 2 ** bits:] == 0).all()
    for j in range(want["quant_map"].shape[0]):
        pts = qz.channels(data, retain + j)[kept].astype(np.float64)
        box = want["quant_map"][j][kept]
        sizes = np.bincount(box, minlength=2 ** bits)
        assert sizes.max() - sizes.min() <= 1                        # a median cut: the boxes are balanced
        for k in range(2 ** bits):
            entry = want["quant_colors"][j, k].astype(np.float64)
            assert (pts[box == k].min(axis=0) <= entry).all() and (entry <= pts[box == k].max(axis=0)).all(), (j, k)
    dec = _decode(want, dim).astype(np.float32)
    assert np.array_equal(dec[kept][:, :1], data[kept][:, :1].astype(np.float32))            # the retained function
    assert np.array_equal(dec[:, -1][kept], data[:, -1][kept].astype(np.float32)) and (dec[:, -1][~kept] == 0).all()


@pytest.mark.parametrize("bits,n_kept", [(5, 32), (5, 7), (16, 2000), (1, 2), (1, 1)])
def test_lossless_case(bits, n_kept):
    n_slots, dim = 8 * 1031, 13
    data, want = qz.case("special", 21, n_slots, dim, n_kept, 1, bits)
    kept = qz.kept_slots(data, 2.0)
    for j in range(want["quant_map"].shape[0]):
        assert np.unique(want["quant_map"][j][kept]).size == n_kept  # at most one point per box
    dec = _decode(want, dim)
    assert np.array_equal(dec[kept].astype(np.float32), data[kept].astype(np.float32))        # as values: -0 == +0
    quantised = [j + c * 4 for j in (1, 2, 3) for c in range(3)]
    assert n_kept < 32 or (data[kept][:, quantised].view(np.uint16) == 0x8000).any()           # -0 went in ...
    assert not (dec[kept][:, quantised].view(np.uint16) == 0x8000).any()                       # ... +0 comes back


def test_a_cut_small_enough_to_read():
    # one basis function, 5 kept slots; R has the largest range (ties would go to R as well)
    data = np.zeros((8, 4), np.float16)
    data[:, 3] = [3, 0, 3, 3, 2, 3, np.nan, 3]                       # slots 0, 2, 3, 5, 7 are kept (2.0 is not > 2.0)
    data[[0, 2, 3, 5, 7], 0] = [1.0, -0.0, 0.0, 1.0, -2.0]
    data[[0, 2, 3, 5, 7], 1] = [0.5, 0.5, 0.25, 0.5, 0.5]
    want = qz.restate(data, 0, 2, 2.0)
    # level 0 orders R: -2 (7), -0 (2), +0 (3), 1 (0), 1 (5): box 0 = {7, 2, 3}, box 1 = {0, 5}
    # level 1: box 0 cuts R again -> {7, 2} | {3}; box 1 has range 0 everywhere -> axis 0, by slot: {0} | {5}
    assert want["quant_map"][0].tolist() == [2, 0, 0, 1, 0, 3, 0, 0]
    assert want["quant_colors"][0, :4, 0].tolist() == [-1.0, 0.0, 1.0, 1.0]
    assert want["quant_colors"][0, :4, 1].tolist() == [0.5, 0.25, 0.5, 0.5]
    assert want["sigma"].tolist() == [3, 0, 3, 3, 0, 3, 0, 3]


# ---- files ----
def _host_tree(seed=3, basis_dim=4):
    return api.N3Tree.from_synth(common.small_scene(depth=3, basis_dim=basis_dim, seed=seed), upload=False)


def test_save_and_open_round_trip_on_the_host(tmp_path):
    t = _host_tree()
    path = str(tmp_path / "tree.npz")
    t.save(path)
    z = np.load(path)
    assert set(z.files) == {"data_dim", "data_format", "child", "invradius3", "offset", "data", "parent_depth"}
    assert str(z["data_format"]) == "SH4" and int(z["data_dim"]) == 13 and z["data"].dtype == np.float16
    back = api.N3Tree(path, upload=False)
    assert np.array_equal(back.child_, t.child_) and np.array_equal(back.data_.view(np.uint16), t.data_.view(np.uint16))
    assert np.array_equal(back.offset, t.offset) and np.array_equal(back.scale, t.scale)
    assert back.data_format == t.data_format and back.data_dim == t.data_dim
    # parent_depth: every node but the root is linked from the slot it names, one level below its parent
    pd, flat = z["parent_depth"], t.child_.reshape(t.capacity, -1)
    assert pd.shape == (t.capacity, 2) and pd[0].tolist() == [0, 0]
    m = np.arange(1, t.capacity)
    slot = pd[1:, 0]
    assert np.array_equal(slot // 8 + flat.reshape(-1)[slot], m) and np.array_equal(pd[1:, 1], pd[slot // 8, 1] + 1)


def test_a_quantised_file_opens_as_its_decode(tmp_path):
    """What save(quantize=...) writes, from the restatement's arrays in the shapes of the script: open() decodes it."""
    t = _host_tree()
    shape = (t.capacity, 2, 2, 2)
    flat = t.data_.reshape(-1, t.data_dim)
    want = qz.restate(flat, 1, 4, 2.0)
    path = str(tmp_path / "q.npz")
    np.savez_compressed(path, data_dim=np.int64(t.data_dim), data_format=np.array("SH4"), child=t.child_,
                        invradius3=t.scale, offset=t.offset, quant_colors=want["quant_colors"],
                        quant_map=want["quant_map"].reshape((3,) + shape), sigma=want["sigma"].reshape(shape),
                        data_retained=want["data_retained"].reshape((1,) + shape + (3,)))
    back = api.N3Tree(path, upload=False)
    assert np.array_equal(back.data_.reshape(-1, t.data_dim).view(np.uint16), _decode(want, t.data_dim).view(np.uint16))


def test_save_refuses_a_tree_without_values(tmp_path):
    t = _host_tree()
    t.clear_cpu_memory()
    with pytest.raises(RuntimeError, match="no data"):
        t.save(str(tmp_path / "t.npz"))
    with pytest.raises(RuntimeError, match="not on the device"):
        t.save(str(tmp_path / "t.npz"), quantize={})
