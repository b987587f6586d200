"""-m gpu: the C++ wrappers volrend::update_data / read_data (include/volrend/update.hpp) on one tree:
tests/cpp/update_check.cpp reads the uploaded tree back, writes a second data set into it as binary16 and as
binary32 and reads it back each time; every array it writes out is compared bit for bit with the file's."""
import numpy as np
import pytest

from tests import build_util
from tests import update_util as uu
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("update_check", tmp_path_factory.mktemp("bin"), gpu=True)


def test_cpp_update_and_read_back(exe, tmp_path):
    name = "sh16"
    tree = uu.case(name)["tree"]
    v2 = uu.variant(name, 2)
    npz, data, before, after32, after16 = (str(tmp_path / n) for n in ("t.npz", "data.raw", "b16.raw", "a32.raw", "a16.raw"))
    synth.save_npz(tree, npz, compressed=False)
    np.ascontiguousarray(v2).tofile(data)
    got = build_util.run_key_values(exe, npz, data, before, after32, after16)
    assert got["throws"] == "1" and int(got["elements"]) == v2.size
    want_a, want_b = uu.stored(tree, tree.data), uu.stored(tree, v2)
    assert np.array_equal(np.fromfile(before, np.uint16), want_a.view(np.uint16).reshape(-1))
    assert np.array_equal(np.fromfile(after32, np.uint32), want_b.astype(np.float32).view(np.uint32).reshape(-1))
    assert np.array_equal(np.fromfile(after16, np.uint16), want_b.view(np.uint16).reshape(-1))
    assert not np.array_equal(want_a, want_b)
