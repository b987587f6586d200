"""-m gpu: the C++ wrappers of include/volrend/rays.hpp on one tree: tests/cpp/rays_check.cpp renders, weighs and
differentiates a shuffled camera-derived list and writes the results out; each is compared with the yardstick of
its entry point -- the oracle's frames bit for bit, the leaf-weight restatement bit for bit, the float64 gradient
within the K of tests/test_gpu_grad.py."""
import numpy as np
import pytest

from tests import build_util, common
from tests import grad_util as gu
from tests import rays_util as ru
from tests import weights_util as wu
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("rays_check", tmp_path_factory.mktemp("bin"), gpu=True)


def test_cpp_ray_calls_match_their_yardsticks(exe, tmp_path):
    """Strict model, two orbit poses of the SH16 scene at 48 x 48, shuffled."""
    ref = gu.reference("sh16", "default", 0, 2, 48)
    tree, trs, w, h, f = ref["tree"], ref["trs"], ref["w"], ref["h"], ref["f"]
    parts = [ru.rays_of_camera(tr, w, h, f) for tr in trs]
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    idx = np.random.default_rng(3).permutation(len(o))
    frames = [common.oracle_frame(tree, tr, w, h, f, 0) for tr in trs]
    want_rgba = np.concatenate([fr[0].reshape(-1, 4) for fr in frames])[idx]
    want_accum = np.concatenate([fr[1].reshape(-1, 4) for fr in frames])[idx]
    want_mw, want_hits, _ = wu.restate(tree, trs, w, h, f, 0)

    npz, o_raw, d_raw, g_raw = (str(tmp_path / n) for n in ("t.npz", "o.raw", "d.raw", "g.raw"))
    prefix = str(tmp_path / "out_")
    synth.save_npz(tree, npz, compressed=False)
    o[idx].tofile(o_raw)
    d[idx].tofile(d_raw)
    np.ascontiguousarray(np.asarray(ref["g"]).reshape(-1, 4)[idx], np.float32).tofile(g_raw)
    got = build_util.run_key_values(exe, npz, o_raw, d_raw, len(idx), 0, g_raw, prefix)
    assert got["throws"] == "2" and int(got["rays"]) == len(idx)

    rgba = np.fromfile(prefix + "rgba.raw", np.uint8).reshape(-1, 4)
    accum = np.fromfile(prefix + "accum.raw", np.float32).reshape(-1, 4)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(accum.view(np.uint32), want_accum.view(np.uint32))
    mw = np.fromfile(prefix + "max_weight.raw", np.float32).reshape(want_mw.shape)
    hits = np.fromfile(prefix + "hits.raw", np.uint32).reshape(want_hits.shape)
    wu.assert_same_slots(mw, hits, want_mw, want_hits, "C++ accumulate_weights_rays")
    grad = np.fromfile(prefix + "grad.raw", np.float32).reshape(ref["grad"].shape)
    ratio, zeros_same = gu.worst_ratio(grad, ref)
    print(f"C++ render_backward_rays: worst |gpu - f64| / unit = {ratio:.3f} of {gu.K}")
    assert (ref["mag"] > 0).sum() > 1000 and (want_mw > 0).any() and (want_accum[:, 3] > 0).any()
    assert ratio <= gu.K and zeros_same
