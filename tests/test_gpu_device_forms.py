"""-m gpu: the arithmetic forms the kernels rest on, over whole operand domains, against the CPU oracle's C
(liboracle.so) and the same C expression under the oracle's flags (tests/cpp/forms_reference.c), bit for bit
(any NaN matches any NaN).

tests/cpp/device_forms_check.hip includes vr_internal.h, vr_device_math.h, vr_dev_shade.h and vr_dev_query.h
unchanged and is compiled with the product's own flags (build_util.hip_program), so the compiler's expansion of a
division, a square root, a float -> int conversion or an FP64 product under -ffp-contract=off and
-fno-gpu-flush-denormals-to-zero is what runs.  It refuses to run where host or device flushes subnormals.

One pass over every float bit pattern x ("sweep"; NaN patterns stay out only where a row says so; sigmoid, sigmoid2,
floor, invdir, div and the drawn-k part of ldexp_div take every OTHERS_EVERY-th pattern, see below):
  expf_nonan      vr_expf_nonan against or_expf; NaN is outside its contract: 2^32 - 2 (2^23 - 1) patterns
  sigmoid         sigmoid(x) of vr_dev_shade.h, the spelling of vr_render.hip, vr_query.hip and vr_dev_backward.h
  sigmoid2        weighted_sigmoid2(1, x, partner(x)): one count per pair, both components compared
  quant8          quant8(x) against the oracle's
  recip, sqrt, floor, invdir
                  1.f / x, sqrtf, floorf, (float)(1.0 / ((double)x + 1e-9))
  n2_axis         query_n2 on one coordinate -- median clamp, digits of (uint32_t)(c * 2^24), local coordinate
                  fract(c * 2^d) for d = 1..24 -- against max(min(x, hi), 0) and 24 rounds of
                  {c *= 2; k = floorf(c); c -= k}; every non-NaN pattern (NaN: the deviation that
                  vr_dev_query.h documents at the clamp)
  ldexp_div       ldexp(x, -k) against x / 2^k: every pattern with k = (bits * 0x9E3779B1) >> 27, plus every
                  k = 0..31 for each of the 2 * 33 * 2^23 patterns with a biased exponent <= 32 (every quotient
                  that can be subnormal)
  div             a / x for a = -2, 1e9, 1 - 2^-24 and a subnormal, plus a / b over all pairs of the 1568 values
                  of the operand table
Tables ("table"):
  byte_over_255   (float)b / 255.f for the 256 bytes
  box_t           (float)((((double)b +- 1e-6) - (double)c) * (double)inv), both signs, over the cube of 128 values
                  (the 22 special values, 53 moderate, 53 any-bits)
  dda_unit, norm3, normalize3, mv3, dot3, cross3
                  Policy<0> against the oracle's _strict, Policy<1> against its _fma: 2^22 seeded operand sets per
                  model, a quarter of them any bit pattern
  basis           precalc_basis against or_basis in 24 forms (SH 1 / 4 / 9 / 16 / 25 with a runtime and with a
                  compile-time size, SG 7, ASG 4; both FP models) over 2^20 lattice directions, the 26 axis and
                  diagonal directions, those with a component replaced by +-0 or a +-subnormal (26 * 12), and 2^12
                  non-unit or non-finite vectors
"""
import re
import subprocess

import pytest

from tests import build_util

pytestmark = pytest.mark.gpu

NON_NAN = (1 << 32) - 2 * ((1 << 23) - 1)
assert NON_NAN == 4_278_190_082
SMALL_EXPONENT = 2 * 33 * (1 << 23)
TABLE_VALUES = 2 * (22 * 22 + 300)
BASIS_DIRECTIONS = (1 << 20) + 26 + 26 * 12 + (1 << 12)

# expf_nonan, quant8, recip, sqrt and n2_axis take every pattern.  The other forms of the sweep take the patterns
# that are multiples of OTHERS_EVERY (odd; 1 = every pattern): the host reference is what the sweep costs, and with
# every pattern in every form the module takes 3.6 times as long as device_math_check's expf run, with 5 it takes 2.5
# times as long.  `device_forms_check sweep 1` runs the rest.
OTHERS_EVERY = 5
OTHERS = ((1 << 32) - 1) // OTHERS_EVERY + 1

SWEEP = {"expf_nonan": NON_NAN, "sigmoid": OTHERS, "sigmoid2": OTHERS, "quant8": 1 << 32, "recip": 1 << 32,
         "sqrt": 1 << 32, "floor": OTHERS, "invdir": OTHERS, "n2_axis": NON_NAN,
         "ldexp_div": OTHERS + 32 * SMALL_EXPONENT, "div": 4 * OTHERS + TABLE_VALUES ** 2}
TABLE = {"byte_over_255": 256, "box_t": 2 * 128 ** 3, "dda_unit": 2 << 22, "norm3": 2 << 22, "normalize3": 2 << 22,
         "mv3": 2 << 22, "dot3": 2 << 22, "cross3": 2 << 22, "basis": 24 * BASIS_DIRECTIONS}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.hip_program("device_forms_check", tmp_path_factory.mktemp("bin"), ("forms_reference.c",))


def run_checks(exe, *what):
    p = subprocess.run([exe, *map(str, what)], capture_output=True, text=True, timeout=900)
    assert p.returncode in (0, 1), f"device_forms_check {what} exited {p.returncode}\n{p.stdout}\n{p.stderr}"
    print(p.stdout)
    checks = {m.group(1): (int(m.group(2)), int(m.group(3)))
              for m in re.finditer(r"^check (\S+) total=(\d+) mismatches=(\d+)$", p.stdout, re.M)}
    return checks, p.stdout


@pytest.fixture(scope="module")
def sweep_checks(exe):
    return run_checks(exe, "sweep", OTHERS_EVERY)


@pytest.fixture(scope="module")
def table_checks(exe):
    return run_checks(exe, "table")


@pytest.mark.parametrize("name", SWEEP)
def test_form_over_every_float(sweep_checks, name):
    checks, out = sweep_checks
    assert checks[name][0] == SWEEP[name], out
    assert checks[name][1] == 0, out


@pytest.mark.parametrize("name", TABLE)
def test_form_over_operand_tables(table_checks, name):
    checks, out = table_checks
    assert checks[name][0] == TABLE[name], out
    assert checks[name][1] == 0, out
