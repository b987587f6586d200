"""vr_tree_update_data / vr_tree_read_data, the part that needs no GPU: the C ABI (symbols, prototypes, header) and
every refusal that comes before the tree handle is followed -- through C, C++ and Python.  The calls below pass a
tree handle that is never followed and device pointers that are never read or written."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from volrend_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
TREE, D = 0x1000, 0x5000   # never dereferenced
CALLS = ("vr_tree_update_data", "vr_tree_read_data")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbols_prototypes_and_abi_version(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "volrend_hip.h")).read()
    for name in CALLS:
        assert name in exported
        res, args = _abi.PROTOTYPES[name]
        assert res is C.c_int and len(args) == 4
        assert getattr(L, name).argtypes == args
    assert L.vr_abi_version() == 3 and "#define VR_ABI_VERSION 3" in header   # additions only
    assert re.search(r"^int vr_tree_update_data\(vr_tree_t tree, const void\* data_dev, int dtype, void\* stream\);",
                     header, flags=re.M)
    assert re.search(r"^int vr_tree_read_data\(vr_tree_t tree, void\* data_dev, int dtype, void\* stream\);",
                     header, flags=re.M)
    assert "enum { VR_DATA_F16 = 0, VR_DATA_F32 = 1 };" in header
    assert (_abi.DATA_F16, _abi.DATA_F32) == (0, 1)


@pytest.mark.parametrize("name", CALLS)
def test_invalid_arguments_through_c(L, name):
    fn = getattr(L, name)

    def call(tree=TREE, data=D, dtype=0):
        return fn(tree, data, dtype, None), (L.vr_last_error() or b"").decode()

    for kw in (dict(tree=None), dict(data=None), dict(tree=None, data=None)):
        rc, msg = call(**kw)
        assert rc == INVALID and "NULL" in msg, kw
    for dtype in (2, -1, 16, 32):
        rc, msg = call(dtype=dtype)
        assert rc == INVALID and "dtype" in msg, dtype
    assert call(tree=None, dtype=1)[0] == INVALID and call(data=None, dtype=1)[0] == INVALID


def test_refusals_through_python(L):
    torch = pytest.importorskip("torch")
    from volrend_amd import api
    t = common.FakeTree(handle=TREE)
    shape = (10, 2, 2, 2, 49)

    def refused(x, match):
        with pytest.raises(ValueError, match=match):
            api.update_data(t, x)
        if x is not None:   # (read_data without `out` allocates its result)
            with pytest.raises(ValueError, match=match):
                api.read_data(t, out=x)

    refused(torch.zeros((10, 2, 2, 2, 48), dtype=torch.float16), "elements")          # wrong element count
    refused(torch.zeros((9,) + shape[1:], dtype=torch.float32), "elements")
    refused(torch.zeros(shape, dtype=torch.float64), "float16 or float32")           # wrong dtype
    refused(torch.zeros(shape, dtype=torch.bfloat16), "float16 or float32")
    refused(torch.zeros(shape, dtype=torch.int16), "float16 or float32")
    refused(torch.zeros((10, 2, 2, 49, 2), dtype=torch.float16).transpose(3, 4), "contiguous")
    refused(torch.zeros(shape, dtype=torch.float16), "device")                       # a host tensor
    refused(torch.zeros(shape, dtype=torch.float32), "device")
    refused(np.zeros(shape, np.float16), "torch CUDA tensor")
    refused(None, "torch CUDA tensor")
    with pytest.raises(ValueError, match="float16 or float32"):
        api.read_data(t, dtype=torch.float64)
    with pytest.raises(ValueError, match="float16 or float32"):
        api.read_data(t, dtype="int8")

    # anything with a device pointer: the interface is checked the same way, and what the C call refuses comes
    # back as VolrendError
    class Cai:
        def __init__(self, shape, typestr, ptr, strides=None):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), strides=strides,
                                                 version=3)

    refused(Cai((10, 8, 48), "<f2", D), "elements")
    refused(Cai((10, 8, 49), "<f8", D), "float16 or float32")
    refused(Cai((10, 8, 49), "<f4", D, strides=(8 * 49 * 8, 49 * 8, 8)), "contiguous")
    for fn in (api.update_data, lambda tree, x: api.read_data(tree, out=x)):
        with pytest.raises(_abi.VolrendError) as e:
            fn(t, Cai((10, 8, 49), "<f4", 0))          # a NULL device pointer: refused by the library, unfollowed
        assert e.value.code == INVALID and "NULL" in str(e.value)


def test_the_gpu_tests_data_sets_flip_sigma_in_every_kind_of_leaf():
    """What tests/test_gpu_update.py relies on, for every scene and whatever lookup structure an upload picks:
    between the two data sets sigma crosses sigma_thresh upwards and downwards in leaves whose sigma lives in
    top-grid entries, in brick entries and in node words only; and the oracle renders the two sets differently."""
    from tests import common
    from tests import update_util as uu
    for name in uu.CASES:
        tree = uu.case(name)["tree"]
        v1, v2 = uu.variant(name, 1), uu.variant(name, 2)
        assert not (v1.view(np.uint16) == v2.view(np.uint16)).all(-1).any(), "a record is the same in both sets"
        for top, brick in ((0, 0), (1, 1), (2, 1), (2, 3), (3, 3), (4, 3), (5, 3), (6, 3)):
            f = uu.flips(tree, top, brick, v1, v2)
            assert f and all(up > 0 and down > 0 for up, down in f.values()), (name, top, brick, f)
    c = uu.case("mixed")
    assert sorted(uu.flips(c["tree"], 2, 1, uu.variant("mixed", 1), uu.variant("mixed", 2))) == [uu.TOP, uu.BRICK, uu.WORD]
    assert sorted(uu.flips(uu.case("blocked")["tree"], 2, 3, uu.variant("blocked", 1), uu.variant("blocked", 2))) == \
        [uu.TOP, uu.BRICK, uu.WORD]
    kinds = uu.leaf_kinds(c["tree"], 2, 1)
    assert (kinds == uu.WORD).sum() > (kinds >= 0).sum() // 2, "most leaves lie below top grid and bricks"
    frames = [common.oracle_frame(uu.with_data(c["tree"], uu.variant("mixed", k)), c["trs"][0], c["w"], c["h"], c["f"])[0]
              for k in (1, 2)]
    assert not np.array_equal(*frames)
    # the scenes' own data cannot stand in for set 1: only their finest leaves carry density
    own = uu.flips(c["tree"], 2, 1, c["tree"].data, uu.variant("mixed", 2))
    assert own[uu.TOP][1] == 0 and own[uu.BRICK][1] == 0


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("update_refusals", tmp_path), refusals=True)
    for call in ("update", "read"):
        for case, word in (("null_tree", "NULL"), ("null_data", "NULL"), ("dtype", "dtype")):
            line = got[f"{call}_{case}"]
            assert line.startswith(f"runtime_error: vr_tree_{call}_data:") and word in line, (call, case, line)
