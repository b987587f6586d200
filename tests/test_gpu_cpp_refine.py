"""-m gpu: volrend::refine_plan / refine_apply and N3Tree's device-array constructor (include/volrend/refine.hpp,
n3tree.hpp): tests/cpp/refine_check.cpp refines one SH4 tree with a seeded selection and a float32 master and writes
the results out; the yardstick is the numpy restatement of tests/refine_util.py, bit for bit."""
import numpy as np
import pytest

from tests import build_util, common
from tests import refine_util as ru
from tests import update_util as uu
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("refine_check", tmp_path_factory.mktemp("bin"), gpu=True)


@pytest.mark.parametrize("sel_name", ["random30", "internal_only"])
def test_cpp_refine_matches_the_restatement(exe, tmp_path, sel_name):
    tree = common.small_scene(depth=4, basis_dim=4, seed=21)
    child, dd, N3, cap = common.rows_of(tree), tree.data_dim, 8, tree.capacity
    sel = ru.selections(child, seed=5)[sel_name]
    master = np.random.default_rng(7).standard_normal((cap * N3, dd)).astype(np.float32)
    held = uu.stored(tree, tree.data).reshape(-1, dd)          # what read_data gives: the sigma of internal slots +0
    want_child, want_slots, (w_data, w_master, w_moment) = ru.restate(
        child, sel, [(held, ru.COPY), (master, ru.COPY), (master, ru.ZERO)])
    n_new = want_slots.size
    assert (n_new == 0) == (sel_name == "internal_only")

    npz, sel_raw, master_raw, prefix = (str(tmp_path / x) for x in ("t.npz", "sel.raw", "master.raw", "out_"))
    synth.save_npz(tree, npz, compressed=False)
    ru.pack_bits(sel).tofile(sel_raw)
    master.tofile(master_raw)
    got = build_util.run_key_values(exe, npz, sel_raw, master_raw, prefix)
    assert got["throws"] == "4" and int(got["n_new"]) == n_new and int(got["capacity"]) == cap + n_new
    assert int(got["workspace"]) >= 20 * (cap * N3 // 32)

    assert np.array_equal(np.fromfile(prefix + "child.raw", np.int32).reshape(-1, N3), want_child)
    assert np.array_equal(np.fromfile(prefix + "src_slot.raw", np.int32), want_slots)
    assert np.array_equal(np.fromfile(prefix + "data.raw", np.uint16), w_data.view(np.uint16).reshape(-1))
    assert np.array_equal(np.fromfile(prefix + "master.raw", np.uint32), w_master.view(np.uint32).reshape(-1))
    assert np.array_equal(np.fromfile(prefix + "moment.raw", np.uint32), w_moment.view(np.uint32).reshape(-1))
    # the tree uploaded from the refined device arrays holds the refined values (refined slots are internal now)
    refined = w_data.copy()
    refined[want_child.reshape(-1) != 0, -1] = 0
    assert np.array_equal(np.fromfile(prefix + "reread.raw", np.uint16), refined.view(np.uint16).reshape(-1))
