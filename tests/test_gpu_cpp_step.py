"""-m gpu: the C++ wrappers of the sparse step -- the marked volrend::render_backward_rays (include/volrend/rays.hpp)
and volrend::tree_step (include/volrend/step.hpp) -- on one tree: tests/cpp/step_check.cpp runs a marked backward
and one SGD step and writes out what it got; the marks are those of the Python call over the same rays, and master,
gradient, bitmap and tree are compared bit for bit with the restatement (tests/step_util.py) of its own gradient."""
import numpy as np
import pytest

from tests import build_util
from tests import step_util as su
from tests import update_util as uu
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("step_check", tmp_path_factory.mktemp("bin"), gpu=True)


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
    got = build_util.run_key_values(exe, npz, *paths, o.shape[0], repr(float(tgs.LR)), repr(float(tgs.LR_SIGMA)), prefix)
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
