"""-m gpu: the C++ wrapper volrend::render_backward (include/volrend/grad.hpp) on one tree: tests/cpp/grad_check.cpp
adds four poses in two calls into one buffer and writes it out; it is compared element by element with the
float64 restatement (tests/grad_util.py), within the K of tests/test_gpu_grad.py."""
import numpy as np
import pytest

from tests import build_util
from tests import grad_util as gu
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("grad_check", tmp_path_factory.mktemp("bin"), gpu=True)


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
def test_cpp_render_backward_matches_the_restatement(exe, tmp_path, fp_mode):
    ref = gu.reference("sh16", "default", fp_mode, 4, 48)
    tree, trs, w, h, f = ref["tree"], ref["trs"], ref["w"], ref["h"], ref["f"]
    npz, poses, g_raw, out_raw = (str(tmp_path / n) for n in ("t.npz", "poses.raw", "g.raw", "grad.raw"))
    synth.save_npz(tree, npz, compressed=False)
    np.stack(trs).astype(np.float32).tofile(poses)
    np.ascontiguousarray(ref["g"], np.float32).tofile(g_raw)
    got = build_util.run_key_values(exe, npz, poses, len(trs), w, h, repr(float(f)), fp_mode, g_raw, out_raw)
    assert got["throws"] == "1" and int(got["elements"]) == ref["grad"].size
    grad = np.fromfile(out_raw, np.float32).reshape(ref["grad"].shape)
    ratio, zeros_same = gu.worst_ratio(grad, ref)
    print(f"C++ wrapper fp{fp_mode}: worst |gpu - f64| / unit = {ratio:.3f} of {gu.K}")
    assert (ref["mag"] > 0).sum() > 1000
    assert ratio <= gu.K and zeros_same
