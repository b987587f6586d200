"""-m gpu: the C++ wrappers of the sparse step -- the marked volrend::render_backward_rays (include/volrend/rays.hpp)
and volrend::tree_step (include/volrend/step.hpp) -- on one tree: tests/cpp/step_check.cpp runs a marked backward
and one SGD step and writes out what it got; the marks are those of the Python call over the same rays, and master,
gradient, bitmap and tree are compared bit for bit with the restatement (tests/step_util.py) of its own gradient."""
import os
import subprocess

import numpy as np
import pytest

from tests import step_util as su
from tests import update_util as uu
from volrend_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    subprocess.check_call(["make", "-C", ROOT, "host"], stdout=subprocess.DEVNULL)
    out = str(tmp_path_factory.mktemp("bin") / "step_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "step_check.cpp"),
                           os.path.join(ROOT, "volrend_amd", "libvolrend_host.a"),
                           "-L", os.path.join(ROOT, "volrend_amd"), "-lvolrend_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "volrend_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def test_cpp_marked_backward_and_step(exe, tmp_path):
    from tests import test_gpu_step as tgs
    name = "sh16"
    tree = uu.case(name)["tree"]
    o, d, g = tgs.rays_of(name)
    npz, prefix = str(tmp_path / "t.npz"), str(tmp_path / "out_")
    synth.save_npz(tree, npz, compressed=False)
    paths = []
    for what, a in (("o", o), ("d", d), ("g", g)):
        paths.append(str(tmp_path / f"{what}.raw"))
        np.ascontiguousarray(a, np.float32).tofile(paths[-1])
    r = subprocess.run([exe, npz, *paths, str(o.shape[0]), repr(float(tgs.LR)), repr(float(tgs.LR_SIGMA)), prefix],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.splitlines() if len(line.split()) == 2)   # (the loader prints too)
    slots = tree.capacity * tree.N ** 3
    assert got["throws"] == "2" and int(got["elements"]) == tree.data.size and int(got["words"]) == su.n_words(slots)

    def raw(what, dtype):
        return np.fromfile(prefix + what + ".raw", dtype)

    mask = su.unpack_bits(raw("touched", np.uint32), slots)
    assert np.array_equal(mask, tgs.sgd_run(name)["mask"]), "the C++ call marks other slots than the Python call"
    grad = raw("grad", np.float32).reshape(tree.data.shape)
    assert not (grad.reshape(slots, -1)[~mask] != 0).any() and (grad != 0).any()
    master0 = uu.stored(tree, tree.data).astype(np.float32)
    want = su.restate("sgd", master0, grad, mask, lr=tgs.LR, lr_sigma=tgs.LR_SIGMA)
    assert np.array_equal(raw("master", np.uint32), want["master"].view(np.uint32).reshape(-1))
    assert not raw("grad_after", np.uint32).any() and not raw("touched_after", np.uint32).any()
    expected = uu.stored(tree, su.mixture(uu.stored(tree, tree.data), want["master"], mask))
    assert np.array_equal(raw("tree", np.uint16), expected.view(np.uint16).reshape(-1))
    assert not np.array_equal(want["master"], master0)
