"""-m gpu: volrend::collapse_plan / collapse_apply and N3Tree's device-array constructor
(include/volrend/collapse.hpp, n3tree.hpp): tests/cpp/collapse_check.cpp collapses one SH4 tree with a seeded selection
and a float32 master and writes the results out; the yardstick is the numpy restatement of tests/collapse_util.py, bit
for bit."""
import numpy as np
import pytest

from tests import build_util, common
from tests import collapse_util as cu
from tests import update_util as uu
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("collapse_check", tmp_path_factory.mktemp("bin"), gpu=True)


@pytest.mark.parametrize("sel_name", ["random50", "non_frontier_only"])
def test_cpp_collapse_matches_the_restatement(exe, tmp_path, sel_name):
    tree = common.small_scene(depth=4, basis_dim=4, seed=21)
    child, dd, N3, cap = common.rows_of(tree), tree.data_dim, 8, tree.capacity
    sel = cu.selections(child, seed=5)[sel_name]
    master = np.random.default_rng(7).standard_normal((cap * N3, dd)).astype(np.float32).view(np.uint32)
    held = uu.stored(tree, tree.data).reshape(-1, dd).view(np.uint16)   # read_data: the sigma of internal slots +0
    want = cu.restate(child, sel, [(held, cu.MEAN), (master, cu.MEAN), (master, cu.ZERO), (master, cu.KEEP)])
    n_keep = want["n_keep"]
    assert (n_keep == cap) == (sel_name == "non_frontier_only")

    npz, sel_raw, master_raw, prefix = (str(tmp_path / x) for x in ("t.npz", "sel.raw", "master.raw", "out_"))
    synth.save_npz(tree, npz, compressed=False)
    cu.pack_bits(sel).tofile(sel_raw)
    master.tofile(master_raw)
    got = build_util.run_key_values(exe, npz, sel_raw, master_raw, prefix)
    assert got["throws"] == "5" and int(got["n_keep"]) == n_keep and int(got["capacity"]) == n_keep
    assert int(got["workspace"]) >= 4 * cap

    assert np.array_equal(np.fromfile(prefix + "child.raw", np.int32).reshape(-1, N3), want["child_out"])
    for key in ("node_map", "src_node", "into_slot"):
        assert np.array_equal(np.fromfile(prefix + key + ".raw", np.int32), want[key]), key
    files = (("data", np.uint16, cu.MEAN), ("master", np.uint32, cu.MEAN), ("moment", np.uint32, cu.ZERO),
             ("kept", np.uint32, cu.KEEP))
    for (key, dtype, rule), w in zip(files, want["dsts"]):
        cu.assert_array(np.fromfile(prefix + key + ".raw", dtype).reshape(-1, dd), w, rule, want["into_slot"], key)
    # the tree uploaded from the collapsed device arrays holds the collapsed values (merged slots are leaves now)
    collapsed = want["dsts"][0].copy()
    collapsed[want["child_out"].reshape(-1) != 0, -1] = 0
    assert np.array_equal(np.fromfile(prefix + "reread.raw", np.uint16), collapsed.reshape(-1))
