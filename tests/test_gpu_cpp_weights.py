"""-m gpu: the C++ wrapper volrend::accumulate_weights (include/volrend/weights.hpp) on one tree:
tests/cpp/weights_check.cpp accumulates six poses in two calls and prints a digest per output; the same
digests are computed here from the CPU restatement (tests/weights_util.py)."""
import numpy as np
import pytest

from tests import build_util
from tests import weights_util as wu
from volrend_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("weights_check", tmp_path_factory.mktemp("bin"), gpu=True)


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
def test_cpp_accumulate_weights_matches_the_restatement(exe, tmp_path, fp_mode):
    tree, trs, w, h, f, want_mw, want_hits, _ = wu.reference("sh16", "default", fp_mode, 6, 96)
    npz = str(tmp_path / "t.npz")
    synth.save_npz(tree, npz, compressed=False)
    np.stack(trs).astype(np.float32).tofile(str(tmp_path / "poses.raw"))
    got = build_util.run_key_values(exe, npz, tmp_path / "poses.raw", len(trs), w, h, repr(float(f)), fp_mode)
    assert got["throws"] == "1"
    assert (want_mw > 0).any()
    assert got["max_weight"] == build_util.word_digest(want_mw)
    assert got["hits"] == build_util.word_digest(want_hits)
