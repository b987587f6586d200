"""The oracle's small helpers as exported for the device sweeps (or_quant8, or_dda_unit, or_norm3, or_normalize3,
or_mv3, or_dot3, or_cross3) against restatements in numpy binary32 (one rounding per operator: the strict model)
and in exact rational arithmetic (one rounding per fused multiply-add: the FMA model); and the host reference of
tests/cpp/device_forms_check.hip (tests/cpp/forms_reference.c) against numpy on sampled patterns."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import build_util
from tests.common import ob

F3 = C.c_float * 3
F9 = C.c_float * 9
f32 = np.float32

SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, 1.17549435e-38, 3e38, -3e38, 1.0, -1.0,
                    0.5, 65504.0], dtype=f32)


def operand_sets(n, width, seed, special=True):
    """n rows of `width` floats: moderate magnitudes, a third of the rows (special=True) with special values mixed
    in or of any bit pattern."""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(-2, 2, (n, width)) * 2.0 ** rng.integers(-20, 20, (n, width))).astype(f32)
    if special:
        pick = rng.random((n, width)) < 0.25
        pick[n // 3:] = False
        a[pick] = SPECIAL[rng.integers(0, SPECIAL.size, int(pick.sum()))]
        a[n // 3:n // 2] = rng.integers(0, 1 << 32, (n // 2 - n // 3, width), dtype=np.uint64).astype(np.uint32).view(f32)
    return a


def same(got, want):
    got, want = np.asarray(got, dtype=f32).ravel(), np.asarray(want, dtype=f32).ravel()
    return all((np.isnan(g) and np.isnan(w)) or g.view(np.uint32) == w.view(np.uint32) for g, w in zip(got, want))


def lib():
    L = ob.lib()
    L.or_quant8.restype = C.c_uint8
    L.or_quant8.argtypes = [C.c_float, C.c_int]
    for name in ("or_dda_unit", "or_dot3"):
        getattr(L, name).restype = C.c_float
        getattr(L, name).argtypes = [F3, F3, C.c_int]
    L.or_norm3.restype = C.c_float
    L.or_norm3.argtypes = [F3, C.c_int]
    L.or_normalize3.restype = None
    L.or_normalize3.argtypes = [F3, C.c_int]
    L.or_mv3.restype = None
    L.or_mv3.argtypes = [F9, F3, C.c_int, F3]
    L.or_cross3.restype = None
    L.or_cross3.argtypes = [F3, F3, C.c_int, F3]
    return L


def fminf(a, b):  # NaN loses, -0 < +0 (vr_detmath.h)
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    if a == b:
        return a if np.signbit(a) else b
    return a if a < b else b


def fmaxf(a, b):
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    if a == b:
        return b if np.signbit(a) else a
    return a if a > b else b


def round_f32(q):
    """The binary32 nearest to the rational q (ties to even); q in the normal range or 0."""
    if q == 0:
        return f32(0)
    s, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert -126 <= e <= 126
    ulp = Fraction(2) ** (e - 23)
    n = q / ulp
    k, rem = n.numerator // n.denominator, n - n.numerator // n.denominator
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
        k += 1
    return f32(s * float(k * ulp))


class Strict:
    mode = ob.FP_STRICT
    madd = staticmethod(lambda a, b, c: f32(f32(a * b) + c))
    msub = staticmethod(lambda a, b, c: f32(f32(a * b) - c))


class Fused:
    mode = ob.FP_FMA
    madd = staticmethod(lambda a, b, c: round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))
    msub = staticmethod(lambda a, b, c: round_f32(Fraction(float(a)) * Fraction(float(b)) - Fraction(float(c))))


def restated(P, m, v, w):
    """common.cuh:12-55 and rt_core.cuh:37-49 in the model P -> dda_unit, norm3, normalize3, mv3, dot3, cross3"""
    s = P.madd(v[2], v[2], P.madd(v[0], v[0], f32(v[1] * v[1])))
    norm = np.sqrt(s)
    inv = f32(1) / norm
    tmax = f32(1e4)
    for i in range(3):
        t1 = f32(-v[i] * w[i])
        t2 = P.madd(-v[i], w[i], w[i]) if P is Fused else f32(t1 + w[i])
        tmax = fminf(tmax, fmaxf(t1, t2))
    mv = [P.madd(m[6 + r], v[2], P.madd(m[r], v[0], f32(m[3 + r] * v[1]))) for r in range(3)]
    dot = P.madd(v[2], w[2], P.madd(v[0], w[0], f32(v[1] * w[1])))
    cross = [P.msub(v[1], w[2], f32(v[2] * w[1])), P.msub(v[2], w[0], f32(v[0] * w[2])),
             P.msub(v[0], w[1], f32(v[1] * w[0]))]
    return tmax, norm, [f32(x * inv) for x in v], mv, dot, cross


@pytest.mark.parametrize("P,n,special", [(Strict, 1500, True), (Fused, 300, False)], ids=["strict", "fma"])
def test_vector_helpers_match_their_restatement(P, n, special):
    L = lib()
    with np.errstate(all="ignore"):
        for row in operand_sets(n, 15, seed=5 + P.mode, special=special):
            m, v, w = row[:9], row[9:12], row[12:]
            tmax, norm, unit, mv, dot, cross = restated(P, m, v, w)
            assert same(L.or_dda_unit(F3(*v), F3(*w), P.mode), tmax), (v, w)
            assert same(L.or_norm3(F3(*v), P.mode), norm), v
            d = F3(*v)
            L.or_normalize3(d, P.mode)
            assert same(list(d), unit), v
            out = F3()
            L.or_mv3(F9(*m), F3(*v), P.mode, out)
            assert same(list(out), mv), (m, v)
            assert same(L.or_dot3(F3(*v), F3(*w), P.mode), dot), (v, w)
            L.or_cross3(F3(*v), F3(*w), P.mode, out)
            assert same(list(out), cross), (v, w)


def test_quant8_truncates_and_guards():
    L = lib()
    xs = np.concatenate([SPECIAL, operand_sets(400, 4, seed=9).ravel(), np.linspace(-2, 3, 2001, dtype=f32),
                         np.array([8421504.0, -8421504.5, 8421505.0, 2147483648.0 / 255, 1e30], dtype=f32)])
    for x in xs:
        with np.errstate(all="ignore"):
            s = f32(x * f32(255))
        want = 0 if np.isnan(s) or s >= 2147483648.0 or s < -2147483648.0 else int(np.trunc(s)) & 0xFF
        for mode in (ob.FP_STRICT, ob.FP_FMA):
            assert L.or_quant8(float(x), mode) == want, (x, mode)


def test_forms_reference_matches_numpy():
    """ref_sweep's plain-operator words, the recurrence of ref_n2_axis and the divisions by 2^k on sampled
    patterns: numpy binary32 rounds each operator once, np.ldexp rounds the scaled value once."""
    R = build_util.c_library("forms_reference.c", oracle=True)
    # (rows of device_forms.h)
    W = {"RECIP": 5, "SQRT": 6, "FLOOR": 7, "INVDIR": 8, "N2_U": 9, "N2_FOLD": 10, "LDEXP": 11, "DIV0": 12}
    words, n = 16, 1 << 12
    rng = np.random.default_rng(3)
    bases = [0, 0x00800000 - n, 0x3F7FFFF0 - n // 2, 0x7F800000 - n, 0x80000000, 0x807FFFFF - n // 2]
    bases += [int(b) for b in rng.integers(0, (1 << 32) - n, 40)]
    assert R.ref_keeps_subnormals() == 1
    for base in bases:
        out = np.zeros((words, n), dtype=np.uint32)
        R.ref_sweep(C.c_uint32(base), C.c_uint32(n), C.c_uint32(n), C.c_uint32(1), out.ctypes.data_as(C.c_void_p))
        u = np.arange(base, base + n, dtype=np.uint64).astype(np.uint32)
        x = u.view(f32)
        with np.errstate(all="ignore"):
            k = ((u * np.uint32(0x9E3779B1)) >> np.uint32(27)).astype(np.int32)
            want = {"RECIP": f32(1) / x, "SQRT": np.sqrt(x), "FLOOR": np.floor(x),
                    "INVDIR": (1.0 / (x.astype(np.float64) + 1e-9)).astype(f32), "LDEXP": np.ldexp(x, -k),
                    "DIV0": f32(-2) / x}
            for name, w in want.items():
                got = out[W[name]].view(f32)
                nan = np.isnan(w)
                assert np.array_equal(np.isnan(got), nan), (name, base)
                assert np.array_equal(got[~nan].view(np.uint32), w[~nan].view(np.uint32)), (name, base)
            # the claim of vr_dev_query.h on the reference alone: digits and local coordinates by the integer route
            ok = ~np.isnan(x)
            c = np.clip(x[ok], f32(0), f32(1) - f32(1e-6))
            digits = (c * f32(16777216)).astype(np.uint32)
            fold = np.zeros(c.size, dtype=np.uint32)
            for d in range(1, 25):
                t = c * f32(2.0 ** d)
                b = (t - np.floor(t)).view(np.uint32)
                fold += (b << np.uint32(d)) | (b >> np.uint32(32 - d))
            assert np.array_equal(out[W["N2_U"]][ok], digits), base
            assert np.array_equal(out[W["N2_FOLD"]][ok], fold), base
