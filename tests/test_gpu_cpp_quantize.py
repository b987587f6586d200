"""-m gpu: volrend::quantize (include/volrend/quantize.hpp): tests/cpp/quantize_check.cpp runs one data array
through the call on a stream of its own and prints a digest per output; the yardstick is the numpy restatement of
tests/quantize_util.py, bit for bit."""
import numpy as np
import pytest

from tests import build_util
from tests import quantize_util as qz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.cpp_program("quantize_check", tmp_path_factory.mktemp("bin"), gpu=True)


@pytest.mark.parametrize("case", [("special", 31, 8 * 1031, 28, 3001, 1, 7, 2.0), ("random", 32, 8 * 37, 13, 131, 0, 16, 2.0)],
                         ids=lambda c: "-".join(map(str, c)))
def test_cpp_quantize_matches_the_restatement(exe, tmp_path, case):
    data, want = qz.case(*case)
    raw = str(tmp_path / "data.raw")
    data.tofile(raw)
    got = build_util.run_key_values(exe, raw, *case[2:4], *case[5:8])
    assert got["throws"] == "2"
    for key, w in want.items():
        if w is None:
            assert key not in got
        else:
            assert got[key] == build_util.word_digest(w.view(np.uint16)), key
