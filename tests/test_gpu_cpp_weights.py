"""-m gpu: the C++ wrapper volrend::accumulate_weights (include/volrend/weights.hpp) on one tree:
tests/cpp/weights_check.cpp accumulates six poses in two calls and prints a digest per output; the same
digests are computed here from the CPU restatement (tests/weights_util.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import weights_util as wu
from tests.test_gpu_cpp_query import digest
from volrend_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    subprocess.check_call(["make", "-C", ROOT, "host"], stdout=subprocess.DEVNULL)
    out = str(tmp_path_factory.mktemp("bin") / "weights_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "weights_check.cpp"),
                           os.path.join(ROOT, "volrend_amd", "libvolrend_host.a"),
                           "-L", os.path.join(ROOT, "volrend_amd"), "-lvolrend_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "volrend_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
def test_cpp_accumulate_weights_matches_the_restatement(exe, tmp_path, fp_mode):
    tree, trs, w, h, f, want_mw, want_hits, _ = wu.reference("sh16", "default", fp_mode, 6, 96)
    npz = str(tmp_path / "t.npz")
    synth.save_npz(tree, npz, compressed=False)
    np.stack(trs).astype(np.float32).tofile(str(tmp_path / "poses.raw"))
    r = subprocess.run([exe, npz, str(tmp_path / "poses.raw"), str(len(trs)), str(w), str(h), repr(float(f)),
                        str(fp_mode)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.splitlines() if len(line.split()) == 2)   # (the loader prints too)
    assert got["throws"] == "1"
    assert (want_mw > 0).any()
    assert got["max_weight"] == digest(want_mw)
    assert got["hits"] == digest(want_hits)
