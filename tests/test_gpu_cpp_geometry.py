"""-m gpu: volrend::tree_geometry / slot_points (include/volrend/geometry.hpp): tests/cpp/geometry_check.cpp runs a
tree and a slot list through both calls on one stream and prints a digest per output; the yardstick is the numpy
restatement of tests/geometry_util.py, bit for bit."""
import numpy as np
import pytest

from tests import build_util
from tests import geometry_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("geometry_check", tmp_path_factory.mktemp("bin"), gpu=True)


@pytest.mark.parametrize("name,k,mode,seed", [("full_n2_73", 1, gu.CENTER, 0), ("random_n3", 5, gu.JITTER, 4000000000)])
def test_cpp_geometry_matches_the_restatement(exe, tmp_path, name, k, mode, seed):
    child = np.ascontiguousarray(gu.TREES[name](), np.int32)
    N = gu.branching(child)
    parent, depth, origin = gu.restate(child)
    assert (depth >= 0).all()                                   # (the origin of every node is specified)
    leaves = gu.reachable_leaves(child, depth)
    slots = np.random.default_rng(3).permutation(leaves)[:max(65, leaves.size // 2)].astype(np.int32)
    pts, d, side = gu.points(depth, origin, N, slots, k, mode, seed)
    child_raw, slots_raw = str(tmp_path / "child.raw"), str(tmp_path / "slots.raw")
    child.tofile(child_raw)
    slots.tofile(slots_raw)
    got = build_util.run_key_values(exe, child_raw, N, child.shape[0], slots_raw, slots.size, k, mode, seed)
    assert got["throws"] == "2"
    for key, want in (("parent_slot", parent), ("node_depth", depth), ("node_origin", origin), ("points", pts),
                      ("depth", d), ("side", side)):
        assert got[key] == build_util.word_digest(want), key
