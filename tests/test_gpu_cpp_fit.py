"""-m gpu: volrend::fit_rays (include/volrend/rays.hpp) on one SH9 tree: tests/cpp/fit_check.cpp fits a shuffled
camera-derived list and writes the results out; every yardstick is the CPU's -- accum: the oracle's frame bit for bit;
sq_err: the numpy head over it bit for bit; touched: the hit set of the march restatement; grad_data: the float64
gradient for the head's g within the K of tests/test_gpu_grad.py."""
import numpy as np
import pytest

from tests import build_util, common
from tests import fit_util as fu
from tests import grad_util as gu
from tests import step_util as su
from volrend_amd import synth

pytestmark = pytest.mark.gpu
BG, GRAD_SCALE = 0.625, 0.0078125     # (both exact in binary32 and in the decimal the program parses)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("fit_check", tmp_path_factory.mktemp("bin"), gpu=True)


def test_cpp_fit_rays_matches_its_yardsticks(exe, tmp_path):
    """Strict model, one orbit pose of the near SH9 scene at 96 x 96, shuffled."""
    base = gu.reference("sh9_near", "default", 0, 1, 96)
    tree, trs, w, h, f = base["tree"], base["trs"], base["w"], base["h"], base["f"]
    o, d = fu.camera_rays(trs, w, h, f)
    n = len(o)
    idx = np.random.default_rng(3).permutation(n)
    target = fu.targets(n, 4)
    accum = common.oracle_frame(tree, trs[0], w, h, f, 0)[1].reshape(-1, 4)
    want = fu.head(accum, target, BG, GRAD_SCALE)
    ref = fu.reference_for(base, want["g"])
    hit = np.zeros(tree.capacity * tree.N ** 3, bool)
    hit[base["traces"][0].all_slots()[0]] = True

    npz, o_raw, d_raw, t_raw = (str(tmp_path / x) for x in ("t.npz", "o.raw", "d.raw", "target.raw"))
    prefix = str(tmp_path / "out_")
    synth.save_npz(tree, npz, compressed=False)
    o[idx].tofile(o_raw)
    d[idx].tofile(d_raw)
    target[idx].tofile(t_raw)
    got = build_util.run_key_values(exe, npz, o_raw, d_raw, n, 0, t_raw, BG, GRAD_SCALE, prefix)
    assert got["throws"] == "2" and int(got["rays"]) == n

    got_accum = np.fromfile(prefix + "accum.raw", np.float32).reshape(-1, 4)
    got_sq = np.fromfile(prefix + "sq_err.raw", np.float32)
    assert np.array_equal(got_accum.view(np.uint32), accum[idx].view(np.uint32))
    assert np.array_equal(got_sq.view(np.uint32), want["sq_err"][idx].view(np.uint32))
    words = np.fromfile(prefix + "touched.raw", np.uint32)
    assert np.array_equal(su.unpack_bits(words, hit.size), hit) and hit.sum() > 50
    grad = np.fromfile(prefix + "grad.raw", np.float32).reshape(ref["grad"].shape)
    assert (ref["mag"] > 0).sum() > 1000 and (accum[:, 3] > 0).any()
    gu.assert_parity(grad, ref, what="C++ fit_rays sh9_near")
