"""-m gpu: the kernels' device math (volrend_amd/csrc/vr_device_math.h) over whole input domains
against the CPU oracle's C functions (oracle/vr_detmath.h through liboracle.so), bit for bit
(any NaN matches any NaN).

tests/cpp/device_math_check.hip includes the header unchanged and is compiled with the product's
own flags (build_util.hip_program: volrend_amd/build.py FLAGS without -shared / -fPIC), so -ffp-contract=off and
-fno-gpu-flush-denormals-to-zero are the contract under test:
  vr_expf / vr_expf2   all 2^32 float bit patterns (vr_expf2: a different pattern in the other lane)
  h2f                  all 65536 half patterns
  mul_half, fma_half,  all 65536 half patterns in either half of the word, times a table of
  mul_add_half         (b, c) operands: +-0, +-inf, NaN, subnormals, overflowing / underflowing
                       products and a few hundred random values
"""
import re
import subprocess

import pytest

from tests import build_util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.hip_program("device_math_check", tmp_path_factory.mktemp("bin"))


def run_checks(exe, what):
    p = subprocess.run([exe, what], capture_output=True, text=True, timeout=600)
    assert p.returncode in (0, 1), f"device_math_check {what} exited {p.returncode}\n{p.stdout}\n{p.stderr}"
    checks = {m.group(1): (int(m.group(2)), int(m.group(3)))
              for m in re.finditer(r"^check (\S+) total=(\d+) mismatches=(\d+)$", p.stdout, re.M)}
    return checks, p.stdout


@pytest.fixture(scope="module")
def expf_checks(exe):
    return run_checks(exe, "expf")


@pytest.mark.parametrize("name,total", [("vr_expf", 1 << 32), ("vr_expf2", 2 << 32)])
def test_expf_every_float(expf_checks, name, total):
    checks, out = expf_checks
    assert checks[name][0] == total, out
    assert checks[name][1] == 0, out


def test_half_operand_forms_every_half(exe):
    checks, out = run_checks(exe, "half")
    assert checks["h2f"] == (65536, 0), out
    for name in ("mul_half", "fma_half", "mul_add_half"):
        n, bad = checks[name]
        assert n >= 2 * 65536 * 700, out   # both halves x every (b, c) pair
        assert bad == 0, out
