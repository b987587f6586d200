"""-m gpu: the C++ wrappers volrend::query_points / query_grid (include/volrend/query.hpp) on one
tree: tests/cpp/query_check.cpp prints a digest per output, and the same digests are computed here
from the CPU oracle's answers (or_query, the records, the colour recomposition of
tests/test_query_host.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import common, query_util as qu
from tests.common import ob
from tests.test_gpu_query import direction_set, grid_coords
from volrend_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    subprocess.check_call(["make", "-C", ROOT, "host"], stdout=subprocess.DEVNULL)
    out = str(tmp_path_factory.mktemp("bin") / "query_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "query_check.cpp"),
                           os.path.join(ROOT, "volrend_amd", "libvolrend_host.a"),
                           "-L", os.path.join(ROOT, "volrend_amd"), "-lvolrend_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "volrend_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def digest(a) -> str:
    """sum_i (w_i + 1) * ((2 i + 1) * K) mod 2^64 over the 32-bit words (query_check.cpp)."""
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        d = ((w + np.uint64(1)) * ((np.uint64(2) * i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))).sum(dtype=np.uint64)
    return f"{int(d):016x}"


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
    r = subprocess.run([exe, npz, str(tmp_path / "p.raw"), str(tmp_path / "d.raw"), str(n), *map(str, res)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.splitlines() if len(line.split()) == 2)   # (the loader prints too)
    assert got["throws"] == "1"
    g = grid_coords((-1.2,) * 3, (1.1,) * 3, res).reshape(-1, 3)
    for prefix, p, d in (("points", pts, dirs), ("grid", g, np.broadcast_to(dirs[0], g.shape))):
        ans = qu.oracle_answers(tree, th, p, "world")
        assert (ans["sigma"] > 0).any()
        ans["rgb"] = qu.recompose_rgb(tree, th, ans["coeffs"], d)
        assert not any(np.isnan(ans[k]).any() for k in ("sigma", "local", "coeffs", "rgb"))
        for k in ("sigma", "depth", "local", "coeffs", "rgb"):
            assert got[f"{prefix}.{k}"] == digest(ans[k]), f"{prefix}.{k}"
