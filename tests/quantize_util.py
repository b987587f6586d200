"""The numpy restatement of vr_quantize (include/volrend_hip.h): kept slots, the median cut level by level exactly as
the header words it (ranges in binary64, ties to the lowest axis, order of the bit patterns, ties by slot index,
ceil(n/2) to box 2k), and the codebook from exact int64 sums.  Vectorised over the boxes of a level; ``restate_naive``
is the same definition as a loop over boxes, for small inputs.  Also the data arrays the tests share."""
import functools

import numpy as np

ROWS = 65536


def ord16(bits):
    """binary16 bit patterns (uint16) -> the integers whose order is the sign-magnitude order (-0 before +0)."""
    b = bits.astype(np.int64)
    return np.where(b & 0x8000, 0xFFFF - b, b | 0x8000)


def kept_slots(data, sigma_thresh):
    with np.errstate(invalid="ignore"):
        return data[:, -1].astype(np.float32) > np.float32(sigma_thresh)    # (False for a NaN sigma)


def channels(data, b):
    """Basis function b of data [n_slots, data_dim] -> float16 [n_slots, 3]."""
    n_basis = (data.shape[1] - 1) // 3
    return data[:, [b, b + n_basis, b + 2 * n_basis]]


def median_cut(pts, slots, bits):
    """pts float16 [m, 3] of the kept slots ``slots`` (ascending) -> the box of each point after ``bits`` levels."""
    m = pts.shape[0]
    box = np.zeros(m, np.int64)
    if m == 0:
        return box
    val = pts.astype(np.float64)
    image = ord16(pts.view(np.uint16))
    for level in range(bits):
        nb = 1 << level
        lo, hi = np.full((nb, 3), np.inf), np.full((nb, 3), -np.inf)
        for c in range(3):
            np.minimum.at(lo[:, c], box, val[:, c])
            np.maximum.at(hi[:, c], box, val[:, c])
        count = np.bincount(box, minlength=nb)
        with np.errstate(invalid="ignore"):
            rng = np.where(count[:, None] > 0, hi - lo, 0.0)
        axis = np.argmax(rng, axis=1)                                       # (the first of equal ranges)
        on_axis = image[np.arange(m), axis[box]]
        order = np.lexsort((slots, on_axis, box))                           # box, then value, then slot index
        start = np.concatenate([[0], np.cumsum(count)[:-1]])
        sbox = box[order]
        rank = np.arange(m) - start[sbox]
        box[order] = 2 * sbox + (rank >= (count[sbox] + 1) // 2)
    return box


def codebook(pts, box, bits):
    """-> float16 [ROWS, 3]: per box the mean from the exact int64 sum of multiples of 2^-24, to float32, to float16."""
    out = np.zeros((ROWS, 3), np.float16)
    if pts.shape[0] == 0:
        return out
    fixed = (pts.astype(np.float64) * 2.0 ** 24).astype(np.int64)           # exact: every finite half is a multiple
    assert np.array_equal(fixed.astype(np.float64) * 2.0 ** -24, pts.astype(np.float64))
    cnt = np.bincount(box, minlength=1 << bits)
    S = np.zeros((1 << bits, 3), np.int64)
    for c in range(3):
        np.add.at(S[:, c], box, fixed[:, c])
    some = cnt > 0
    mean = (S[some].astype(np.float64) / cnt[some, None].astype(np.float64)) * 2.0 ** -24
    out[:1 << bits][some] = mean.astype(np.float32).astype(np.float16)
    return out


def restate(data, n_retained, bits, sigma_thresh, cut=median_cut):
    """data float16 [n_slots, data_dim] -> dict of the four outputs of vr_quantize (data_retained None without)."""
    data = np.ascontiguousarray(data, np.float16)
    n_slots, data_dim = data.shape
    n_basis = (data_dim - 1) // 3
    n_quant = n_basis - n_retained
    kept = kept_slots(data, sigma_thresh)
    slots = np.flatnonzero(kept)
    sigma = np.where(kept, data[:, -1].view(np.uint16), 0).astype(np.uint16).view(np.float16)
    retained = None
    if n_retained:
        retained = np.zeros((n_retained, n_slots, 3), np.uint16)
        for r in range(n_retained):
            retained[r][kept] = channels(data, r).view(np.uint16)[kept]
        retained = retained.view(np.float16)
    colors = np.zeros((n_quant, ROWS, 3), np.float16)
    qmap = np.zeros((n_quant, n_slots), np.uint16)
    for j in range(n_quant):
        pts = np.ascontiguousarray(channels(data, n_retained + j)[kept])
        box = cut(pts, slots, bits)
        qmap[j, slots] = box
        colors[j] = codebook(pts, box, bits)
    return {"quant_colors": colors, "quant_map": qmap, "sigma": sigma, "data_retained": retained}


def median_cut_naive(pts, slots, bits):
    """The same cut as a loop over the boxes: the header's sentences one by one."""
    boxes = {0: np.arange(pts.shape[0])}
    bitsu = pts.view(np.uint16)
    for level in range(bits):
        nxt = {}
        for k, members in boxes.items():
            if members.size == 0:
                continue
            v = pts[members].astype(np.float64)
            rng = v.max(axis=0) - v.min(axis=0)
            axis = 0
            for c in (1, 2):
                if rng[c] > rng[axis]:
                    axis = c
            keys = sorted(range(members.size),
                          key=lambda i: (int(ord16(bitsu[members[i], axis:axis + 1])[0]), int(slots[members[i]])))
            half = (members.size + 1) // 2
            nxt[2 * k] = members[keys[:half]]
            nxt[2 * k + 1] = members[keys[half:]]
        boxes = nxt
    box = np.zeros(pts.shape[0], np.int64)
    for k, members in boxes.items():
        box[members] = k
    return box


# ---- the arrays the tests share ----
def _sigma(rng, n_slots, n_kept, thresh=2.0):
    """Sigmas with exactly n_kept above the threshold, at random places; the others at or below it."""
    s = rng.uniform(-1.0, thresh, n_slots).astype(np.float16)
    s[s.astype(np.float32) > thresh] = np.float16(thresh)
    where = rng.permutation(n_slots)[:n_kept]
    s[where] = rng.uniform(thresh + 0.5, 60.0, n_kept).astype(np.float16)
    return s


def random_data(seed, n_slots, data_dim, n_kept, scale=1.0):
    rng = np.random.default_rng(seed)
    data = (rng.standard_normal((n_slots, data_dim)) * scale).astype(np.float16)
    data[:, -1] = _sigma(rng, n_slots, n_kept)
    return data


def special_data(seed, n_slots, data_dim, n_kept):
    """Many duplicate points, two axes of equal range, +-0, subnormals, +-65504, a sigma equal to the threshold (2.0)
    and a NaN sigma."""
    rng = np.random.default_rng(seed)
    n_basis = (data_dim - 1) // 3
    palette = np.array([0.0, -0.0, 6e-8, -6e-8, 5.96e-8, 1e-5, -1e-5, 65504.0, -65504.0, 1.0, -1.0, 0.5, 0.25, 3.0],
                       np.float16)
    data = palette[rng.integers(0, palette.size, (n_slots, data_dim))]
    for b in range(n_basis):                       # G repeats R permuted: equal ranges on axes 0 and 1
        data[:, b + n_basis] = data[rng.permutation(n_slots), b]
    if n_basis > 1:                                # the last basis function: few distinct points, many ties
        few = palette[rng.integers(9, palette.size, (3, 3))]
        pick = rng.integers(0, 3, n_slots)
        for c in range(3):
            data[:, n_basis - 1 + c * n_basis] = few[pick, c]
    data[:, -1] = _sigma(rng, n_slots, n_kept)
    not_kept = np.flatnonzero(~kept_slots(data, 2.0))
    if not_kept.size >= 2:
        data[not_kept[0], -1] = np.float16(2.0)
        data[not_kept[1], -1] = np.float16(np.nan)
    return data


@functools.lru_cache(maxsize=None)
def case(kind, seed, n_slots, data_dim, n_kept, n_retained, bits, sigma_thresh=2.0):
    """-> (data, the restated outputs): computed once per argument list, never written."""
    data = (special_data if kind == "special" else random_data)(seed, n_slots, data_dim, n_kept)
    want = restate(data, n_retained, bits, sigma_thresh)
    for a in (data, *want.values()):
        if a is not None:
            a.setflags(write=False)
    return data, want
