"""-m gpu: the C++ wrappers volrend::query_points / query_grid (include/volrend/query.hpp) on one
tree: tests/cpp/query_check.cpp prints a digest per output, and the same digests are computed here
from the CPU oracle's answers (or_query, the records, the colour recomposition of
tests/test_query_host.py)."""
import numpy as np
import pytest

from tests import build_util, common, query_util as qu
from tests.common import ob
from tests.query_util import direction_set, grid_coords
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("query_check", tmp_path_factory.mktemp("bin"), gpu=True)


def test_cpp_query_matches_oracle(exe, tmp_path):
    tree = common.small_scene(depth=5, basis_dim=9, seed=520)      # finite values: digests compare bits
    th = ob.TreeHandle(tree)
    n, res = 6001, (9, 4, 70)
    pts = qu.to_world(tree, qu.point_set(tree, n, 521))
    dirs = direction_set(n, 522)
    dirs[0] = (0.2, 0.3, -0.9)
    npz = str(tmp_path / "t.npz")
    synth.save_npz(tree, npz, compressed=False)
    pts.tofile(str(tmp_path / "p.raw"))
    dirs.tofile(str(tmp_path / "d.raw"))
    got = build_util.run_key_values(exe, npz, tmp_path / "p.raw", tmp_path / "d.raw", n, *res)
    assert got["throws"] == "1"
    g = grid_coords((-1.2,) * 3, (1.1,) * 3, res).reshape(-1, 3)
    for prefix, p, d in (("points", pts, dirs), ("grid", g, np.broadcast_to(dirs[0], g.shape))):
        ans = qu.oracle_answers(tree, th, p, "world")
        assert (ans["sigma"] > 0).any()
        ans["rgb"] = qu.recompose_rgb(tree, th, ans["coeffs"], d)
        assert not any(np.isnan(ans[k]).any() for k in ("sigma", "local", "coeffs", "rgb"))
        for k in ("sigma", "depth", "local", "coeffs", "rgb"):
            assert got[f"{prefix}.{k}"] == build_util.word_digest(ans[k]), f"{prefix}.{k}"
