"""Building blocks of the oracle: deterministic expf, fp16 conversion, counters."""
import numpy as np

from tests import common
from tests.common import ob


def test_half_conversion_exhaustive():
    L = ob.lib()
    bits = np.arange(65536, dtype=np.uint16)
    want = bits.view(np.float16).astype(np.float32)
    got = np.array([L.or_half2float(int(b)) for b in bits], dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_det_expf_accuracy_and_edges():
    L = ob.lib()
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-90, 88, 20000), rng.uniform(-1, 1, 20000),
                         np.array([0.0, -0.0, 1.0, -1.0, 88.7, -87.3, -100.0, -103.9])]).astype(
                             np.float32)
    got = np.array([L.or_expf(float(x)) for x in xs], dtype=np.float32)
    ref = np.exp(xs.astype(np.float64))
    ok = (ref > 1.2e-38) & (ref < 3.0e38)
    ulp = np.abs(got[ok].astype(np.float64) - ref[ok]) / np.spacing(ref[ok].astype(np.float32))
    assert ulp.max() < 1.0, ulp.max()
    assert L.or_expf(-200.0) == 0.0
    assert np.isinf(L.or_expf(100.0))
    assert np.isnan(L.or_expf(float("nan")))
    assert L.or_expf(0.0) == 1.0


def test_det_expf_within_one_ulp_dense_sweep():
    """vr_det_expf against double-precision exp on every 64th float of [-104, 89] (about 35 M
    inputs): normal, subnormal (x < -87.3) and overflowing (x > 88.72) results alike.  The error
    is measured in units of the binary32 grid below |exp(x)| (2^-149 in the subnormal band); a
    result that rounds beyond FLT_MAX must be +inf."""
    L = ob.lib()
    lo, hi = np.float32(-104.0).view(np.uint32), np.float32(89.0).view(np.uint32)
    sweeps = [np.arange(0, int(hi) + 1, 64, dtype=np.uint32),              # +0 .. 89
              np.arange(0x80000000, int(lo) + 1, 64, dtype=np.uint32)]     # -0 .. -104
    n, worst = 0, 0.0
    for bits in sweeps:
        for part in np.array_split(bits, max(1, bits.size // (1 << 22))):
            x = part.view(np.float32)
            got = np.empty_like(x)
            L.or_expf_n(x.ctypes.data, got.ctypes.data, x.size)
            ref = np.exp(x.astype(np.float64))
            with np.errstate(over="ignore"):
                ref32 = ref.astype(np.float32)
            inf = np.isinf(ref32)
            assert np.array_equal(np.isinf(got), inf), x[np.isinf(got) != inf][:8]
            r = ref32[~inf]
            below = np.where(r.astype(np.float64) > ref[~inf], np.nextafter(r, np.float32(0)), r)
            ulp = np.abs(got[~inf].astype(np.float64) - ref[~inf]) / np.spacing(below).astype(np.float64)
            assert ulp.max() < 1.0, (ulp.max(), x[~inf][np.argmax(ulp)])
            worst = max(worst, float(ulp.max()))
            n += x.size
    assert n > 30_000_000 and worst > 0.5


def test_counters_consistent():
    tree = common.small_scene(depth=6, basis_dim=16, seed=5)
    tr, w, h, f = common.camera_for(pose_idx=2, size=64)
    _, _, c = common.oracle_frame(tree, tr, w, h, f)
    dd = tree.data_dim
    assert c["rays"] == w * h
    assert c["child_reads"] >= c["samples"] >= c["hit_samples"] >= c["early_stops"]
    assert c["alg_bytes"] == 4 * c["child_reads"] + 2 * c["samples"] + \
        2 * (dd - 1) * c["hit_samples"] + 4 * w * h
    # single-threaded and multi-threaded runs agree
    th = ob.TreeHandle(tree)
    cam = ob.make_camera(tr, w, h, f)
    a, _, c1 = ob.render(th, cam, ob.default_options(), nthreads=1)
    b, _, c2 = ob.render(th, cam, ob.default_options(), nthreads=5)
    assert np.array_equal(a, b) and c1 == c2


def test_region_render_matches_full_frame():
    tree = common.small_scene(depth=5, basis_dim=4, seed=6)
    tr, w, h, f = common.camera_for(pose_idx=1, size=50)
    full, _, _ = common.oracle_frame(tree, tr, w, h, f)
    part, _, _ = common.oracle_frame(tree, tr, w, h, f, region=(10, 20, 30, 17))
    assert np.array_equal(part[20:37, 10:40], full[20:37, 10:40])
    assert (part[:20] == 0).all()
