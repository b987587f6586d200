"""Helpers of the vr_tree_step tests: the numpy binary32 restatement of the step's arithmetic (include/volrend_hip.h),
the bitmap of touched slots, what the tree holds afterwards, the comparison of one call with the restatement, the
bitmap patterns and the value-domain catalogue the GPU tests run (needs no GPU: torch is handed in)."""
from __future__ import annotations

import functools

import numpy as np

from tests import update_util as uu

f32 = np.float32


def n_words(n_slots):
    return (n_slots + 31) // 32


def pack_bits(mask):
    """bool [n_slots] (any shape, flattened) -> uint32 [ceil(n_slots / 32)]: bit s & 31 of word s >> 5 is slot s."""
    mask = np.asarray(mask, bool).reshape(-1)
    padded = np.zeros(n_words(mask.size) * 32, bool)
    padded[:mask.size] = mask
    return np.packbits(padded, bitorder="little").view("<u4").copy()


def unpack_bits(words, n_slots):
    """uint32 / int32 words -> bool [n_slots]."""
    b = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(b, bitorder="little")[:n_slots].astype(bool)


def host_scalars(lr, lr_sigma, betas, step):
    """The four scalars the host forms in binary64 and rounds once to binary32 -> (omb1, omb2, sbc2, a, a_sigma),
    from the binary32 values of the betas and rates the C struct carries."""
    b1, b2 = float(f32(betas[0])), float(f32(betas[1]))
    bc1 = 1.0 - b1 ** step
    return (f32(1.0 - b1), f32(1.0 - b2), f32(np.sqrt(1.0 - b2 ** step)), f32(float(f32(lr)) / bc1),
            f32(float(f32(lr_sigma)) / bc1))


def restate(kind, master, grad, mask, *, lr, lr_sigma=None, m=None, v=None, betas=(0.9, 0.999), eps=1e-8, step=1):
    """vr_tree_step in numpy, binary32 with one rounding per operator.  master / grad / m / v: float32
    [..., data_dim] in the file's indexing; mask: bool, one per slot.  -> dict(master, grad, m, v) of new arrays
    (m, v None for SGD); slots whose mask is clear keep every bit in all of them."""
    shape = master.shape
    dd = shape[-1]
    mask = np.asarray(mask, bool).reshape(-1)
    lr_sigma = lr if lr_sigma is None else lr_sigma
    out = {k: (None if a is None else np.array(a, f32).reshape(-1, dd)) for k, a in
           (("master", master), ("grad", grad), ("m", m), ("v", v))}
    w0, g = out["master"][mask], out["grad"][mask]
    assert w0.dtype == f32 and g.dtype == f32
    with np.errstate(all="ignore"):
        if kind == "sgd":
            rate = np.full(dd, f32(lr), f32)
            rate[-1] = f32(lr_sigma)
            w = w0 - rate * g
        else:
            omb1, omb2, sbc2, a, a_sigma = host_scalars(lr, lr_sigma, betas, step)
            beta1, beta2, e = f32(betas[0]), f32(betas[1]), f32(eps)
            rate = np.full(dd, a, f32)
            rate[-1] = a_sigma
            m1 = beta1 * out["m"][mask] + omb1 * g
            v1 = beta2 * out["v"][mask] + (omb2 * g) * g
            w = w0 - rate * (m1 / (np.sqrt(v1) / sbc2 + e))
            assert m1.dtype == f32 and v1.dtype == f32
            out["m"][mask], out["v"][mask] = m1, v1
    assert w.dtype == f32
    out["master"][mask] = w
    out["grad"][mask] = f32(0.0)
    return {k: (None if a is None else a.reshape(shape)) for k, a in out.items()}


def mixture(old16, master, mask):
    """float16, the file's shape: binary16(master), rounded to nearest even, in the slots of `mask`, `old16`
    elsewhere -- the data array whose fresh upload the tree equals after a step."""
    dd = old16.shape[-1]
    out = np.array(old16, np.float16).reshape(-1, dd)
    mask = np.asarray(mask, bool).reshape(-1)
    with np.errstate(over="ignore"):
        out[mask] = np.asarray(master, f32).reshape(-1, dd)[mask].astype(np.float16)
    return out.reshape(old16.shape)


# ---- one call, compared (shared by tests/test_gpu_step.py and tests/test_gpu_step_shapes.py) ------------------------
SENTINEL = f32(-123.456)    # in grad / m / v of the slots a call must neither read nor write


def with_sentinel(a, mask):
    """A copy of float32 `a` [..., data_dim] with SENTINEL in every slot whose mask is clear."""
    out = np.array(a, f32, copy=True)
    out.reshape(-1, a.shape[-1])[~np.asarray(mask, bool).reshape(-1)] = SENTINEL
    return out


def device_call(torch, t, kind, host, mask, words, **kw):
    """One vr_tree_step from host arrays (grad, and for Adam m and v, with the sentinel in unmarked slots) -> what it
    left on the device, as numpy."""
    on_dev = {k: uu.dev(torch, host[k] if k == "master" else with_sentinel(host[k], mask))
              for k in (("master", "grad") + (("m", "v") if kind == "adam" else ()))}
    bits = uu.dev(torch, np.asarray(words, np.uint32).view(np.int32))
    t.step(on_dev["master"], on_dev["grad"], bits, kind=kind, m=on_dev.get("m"), v=on_dev.get("v"), **kw)
    read = t.read_data()
    torch.cuda.synchronize()
    got = {k: (on_dev[k].cpu().numpy() if k in on_dev else None) for k in ("master", "grad", "m", "v")}
    got.update(words=bits.cpu().numpy().view(np.uint32), read=read.cpu().numpy())
    return got


def same_or_nan(got, want):
    """Mask of the elements (binary32 or binary16) that are bit-equal, or NaN in both: tests/aov_util.same_bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    return (got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))


def element_mismatches(got, want):
    """int [data_dim]: per element index of a record, the number of slots in which `got` is not `want`."""
    return (~same_or_nan(got, want)).reshape(-1, got.shape[-1]).sum(0)


def assert_call(got, want, mask, expected16, what, nan_ok=False):
    """What one vr_tree_step call left behind.  got: dict(master, grad, m, v (None for SGD), words, read) as numpy,
    of a call whose grad / m / v carried SENTINEL in unmarked slots; want: restate()'s dict from the arrays WITHOUT
    the sentinel; expected16: update_util.stored(mixture(...)).  Everything is bit-exact; with nan_ok an element may
    instead be NaN on both sides (NaN in exactly the same elements)."""
    mask = np.asarray(mask, bool).reshape(-1)
    dd = want["master"].shape[-1]
    for key in ("master", "m", "v"):
        if want[key] is None:
            continue
        w = want[key] if key == "master" else with_sentinel(want[key], mask)
        ok = same_or_nan(got[key], w)
        if not nan_ok:
            assert not np.isnan(w).any(), f"{what}: the expected {key} holds a NaN"
        bad = element_mismatches(got[key], w)
        assert ok.all(), (f"{what}: {key} differs from the restatement in {int((~ok).sum())} elements; per element "
                          f"index, slots wrong: {dict((int(e), int(bad[e])) for e in np.flatnonzero(bad)[:12])}")
    g = got["grad"].reshape(-1, dd)
    assert (g[mask].view(np.uint32) == 0).all(), f"{what}: grad is not +0 in a marked slot"
    assert (g[~mask].view(np.uint32) == SENTINEL.view(np.uint32)).all(), f"{what}: grad of an unmarked slot was written"
    assert not got["words"].any(), f"{what}: the bitmap is not zero after the step"
    ok = same_or_nan(got["read"], expected16)
    if not nan_ok:
        assert not np.isnan(expected16).any()
    bad = element_mismatches(got["read"], expected16)
    assert ok.all(), (f"{what}: the tree differs from binary16(master) in {int((~ok).sum())} elements; per element "
                      f"index, slots wrong: {dict((int(e), int(bad[e])) for e in np.flatnonzero(bad)[:12])}")


def chunk_mismatches(got, want):
    """-> {range name: mismatching elements} over the element ranges a record longer than a wave is walked in: the
    first 64 elements, the rest but sigma, sigma."""
    bad = element_mismatches(got, want)
    dd = bad.size
    return {"e < 64": int(bad[:64].sum()), "64 <= e < data_dim - 1": int(bad[64:dd - 1].sum()),
            "e == data_dim - 1": int(bad[dd - 1])}


# ---- bitmaps (tests/test_gpu_step_shapes.py; the caps: tests/test_step_host.py) ------------------------------------
GROUP = 2048     # the slots of 64 consecutive bitmap words
COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129)   # the neighbours of 8 * {1, 2, 6, 8, 16}


def bitmap_patterns(n_slots, seed=31):
    """-> [(label, uint32 words, the groups the pattern names)] for a tree of n_slots >= GROUP + 4 slots: every word
    all ones (bits beyond the last slot included), one bit in the whole bitmap, runs of four across a word and a
    group boundary, exactly c bits inside group 0, words only at position 63 of a group, only the last group."""
    assert n_slots >= GROUP + 4
    rng = np.random.default_rng(seed)
    nw = n_words(n_slots)
    n_groups = (n_slots + GROUP - 1) // GROUP
    out = [("all ones", np.full(nw, 0xFFFFFFFF, np.uint32), list(range(n_groups)))]

    def of_slots(slots):
        m = np.zeros(n_slots, bool)
        m[np.asarray(slots)] = True
        return pack_bits(m)

    for s in (0, GROUP - 1, GROUP, n_slots - 1):
        out.append((f"one bit, slot {s}", of_slots([s]), [s // GROUP]))
    out.append(("slots 30..33", of_slots(np.arange(30, 34)), [0]))
    out.append((f"slots {GROUP - 2}..{GROUP + 1}", of_slots(np.arange(GROUP - 2, GROUP + 2)), [0, 1]))
    for c in COUNTS:
        out.append((f"{c} bits in group 0", of_slots(rng.choice(GROUP, c, replace=False)), [0]))
    words = np.zeros(nw, np.uint32)
    at = np.arange(63, nw, 64)
    words[at] = rng.integers(1, 2 ** 32, at.size, dtype=np.uint64).astype(np.uint32)
    out.append(("lane 63's words", words, [int(w) // 64 for w in at if int(w) * 32 < n_slots]))
    m = np.zeros(n_slots, bool)
    first = (n_groups - 1) * GROUP
    m[first:] = rng.random(n_slots - first) < 0.5
    out.append(("the last group", pack_bits(m), [n_groups - 1]))
    return out


# ---- the value domain of the step (GPU: tests/test_gpu_step.py; what it shows: tests/test_step_host.py) -------------
BELOW_ONE = float(np.nextafter(f32(1.0), f32(0.0)))     # the largest binary32 below 1
INF, NAN = float("inf"), float("nan")

# A handful of calls, not the product: every eps (0, 1e-8, 1), every pair of betas, every step count and every lr
# (with lr_sigma of the other sign) appears once; each call runs the whole catalogue of entries below.
# (adam_huge: beta1^step underflows, so a == lr stays finite.)
CALLS = {
    "sgd": dict(kind="sgd", lr=1e-3, lr_sigma=-0.5),
    "adam": dict(kind="adam", lr=1e-3, lr_sigma=-0.5, betas=(0.9, 0.999), eps=1e-8, step=1),
    "adam_eps0": dict(kind="adam", lr=-0.5, lr_sigma=1e-3, betas=(0.0, 0.0), eps=0.0, step=2),
    "adam_eps1": dict(kind="adam", lr=0.0, lr_sigma=-1e-3, betas=(0.5, BELOW_ONE), eps=1.0, step=1000),
    "adam_huge": dict(kind="adam", lr=3e38, lr_sigma=-3e38, betas=(BELOW_ONE, 0.0), eps=1e-8, step=2 ** 31 - 1),
}
# The step's summation constant (tests/test_step_host.py::test_restatement_against_float64 measures it): the largest
# |restate("adam") - the header's formulas in binary64| / (2^-24 (|w0| + |a_e| (|beta1 m| + |omb1 g|) / (sqrt(v') /
# sbc2 + eps))) over the elements of the catalogue below and of random draws under every pair of betas, eps and step
# count whose binary32 intermediates neither overflow nor underflow: 4.896 (random draws, betas (0.5, the largest
# binary32 below 1), eps 1e-8, step 2^31 - 1).  It ties the restatement to the formula; the GPU is compared with the
# restatement bit for bit, so no GPU tolerance comes from it.
K_STEP32 = 5.0
CATALOGUE_SCENES = ("sh16", "sh25")
COPIES, SIGMA_COPIES = 16, 6


def passes_through(call):
    """A zero gradient with zero moments leaves master as it is: SGD, and Adam with eps > 0 (0 / (0 + eps))."""
    return call["kind"] == "sgd" or call["eps"] > 0


@functools.lru_cache(maxsize=None)
def entries():
    """-> [(label, master, g, m, v)], one element each.  Pass-through rounding (g = m = v = 0 over
    update_util.edge_values()); every gradient with zero moments (1e-20: v' is a binary32 subnormal; 1e20: g * g
    overflows) and again beside ordinary moments; every pair of moments beside an ordinary gradient (v = -1 is a
    caller's mistake: sqrtf gives NaN, in that element alone)."""
    grads = [0.0, -0.0] + [s * x for x in (2.0 ** -149, 1e-20, 1e-10, 1.0, 1e19, 1e20, 3e38, INF) for s in (1, -1)] + [NAN]
    ms = [0.0, 1e-30, -1e-30, 1.0, -1.0, 3e38, -3e38]
    vs = [0.0, 2.0 ** -149, 1e-40, 1e-12, 1.0, 3e38, INF, -1.0]
    out = [(f"pass {float(x)!r}", float(x), 0.0, 0.0, 0.0) for x in uu.edge_values()]
    out += [(f"g {g!r}", 0.5, g, 0.0, 0.0) for g in grads]
    out += [(f"g {g!r} beside m 1, v 1e-12", 0.5, g, 1.0, 1e-12) for g in grads]
    out += [(f"m {m!r}, v {v!r}", 0.5, 1e-3, m, v) for m in ms for v in vs]
    assert len({e[0] for e in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """The arrays every call of CALLS starts from on scene `name`, read-only -> dict(old16: data set 1 of the scene,
    what the tree holds; master, grad, m, v: float32, the file's shape; mask: bool per slot -- half the leaves and a
    few internal slots; coeff: {label: flat element indices}, COPIES coefficient elements of marked leaves per entry;
    sigma: {label: slots}, SIGMA_COPIES marked leaves whose sigma element carries the entry).  Everything else in a
    marked slot is ordinary: master from data set 1, a random gradient, small moments with v >= 0."""
    tree = uu.case(name)["tree"]
    rng = np.random.default_rng(4100 + tree.data_dim)
    dd, shape = tree.data_dim, tree.data.shape
    slots = tree.capacity * tree.N ** 3
    internal = np.asarray(tree.child).reshape(-1) != 0
    mask = (rng.random(slots) < 0.5) & ~internal
    mask[np.flatnonzero(internal)[::29]] = True
    old16 = uu.variant(name, 1)
    arrays = dict(master=uu.stored(tree, old16).astype(f32),
                  grad=(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 0, shape)).astype(f32),
                  m=(rng.standard_normal(shape) * 0.1).astype(f32),
                  v=((rng.standard_normal(shape) * 0.1) ** 2).astype(f32))
    flat = {k: a.reshape(slots, dd) for k, a in arrays.items()}
    cat = entries()
    leaves = np.flatnonzero(mask & ~internal)
    # distinct coefficient elements, and distinct leaves for the sigma copies
    at = rng.choice(leaves.size * (dd - 1), len(cat) * COPIES, replace=False)
    c_slot, c_elem = leaves[at // (dd - 1)].reshape(len(cat), COPIES), (at % (dd - 1)).reshape(len(cat), COPIES)
    s_slot = rng.choice(leaves, len(cat) * SIGMA_COPIES, replace=False).reshape(len(cat), SIGMA_COPIES)
    coeff, sigma = {}, {}
    for n, (label, w0, g, m, v) in enumerate(cat):
        for key, x in (("master", w0), ("grad", g), ("m", m), ("v", v)):
            flat[key][c_slot[n], c_elem[n]] = f32(x)
            flat[key][s_slot[n], dd - 1] = f32(x)
        coeff[label], sigma[label] = c_slot[n] * dd + c_elem[n], s_slot[n]
    for a in arrays.values():
        a.setflags(write=False)
    mask.setflags(write=False)
    return dict(arrays, old16=old16, mask=mask, coeff=coeff, sigma=sigma)


def call_kw(call):
    return {k: v for k, v in call.items() if k != "kind"}


@functools.lru_cache(maxsize=None)
def catalogue_expected(name, call_name):
    """-> (restate()'s dict, the float16 data array a fresh upload of which the tree equals) of one call."""
    c, call = catalogue(name), CALLS[call_name]
    adam = call["kind"] == "adam"
    want = restate(call["kind"], c["master"], c["grad"], c["mask"], m=c["m"] if adam else None,
                   v=c["v"] if adam else None, **call_kw(call))
    return want, mixture(c["old16"], want["master"], c["mask"])


SIGMA_OUTCOMES = ("rises", "falls", "nan", "+inf", "-inf", "negative", "-0", "subnormal")


def sigma_outcomes(name, expected16):
    """-> {outcome: marked leaves}: what the step makes of sigma, against the threshold and as binary16."""
    c = catalogue(name)
    tree = uu.case(name)["tree"]
    leaf = c["mask"] & (np.asarray(tree.child).reshape(-1) == 0)
    dd = tree.data_dim
    old = c["old16"].reshape(-1, dd)[leaf, -1]
    new = np.asarray(expected16).reshape(-1, dd)[leaf, -1]
    on0, on1 = old.astype(f32) > uu.SIGMA_THRESH, new.astype(f32) > uu.SIGMA_THRESH
    bits = new.view(np.uint16)
    found = {"rises": ~on0 & on1, "falls": on0 & ~on1, "nan": np.isnan(new), "+inf": bits == 0x7C00, "-inf": bits == 0xFC00,
             "negative": np.isfinite(new) & (new < 0), "-0": bits == 0x8000,
             "subnormal": ((bits & 0x7C00) == 0) & ((bits & 0x03FF) != 0)}
    return {k: int(v.sum()) for k, v in found.items()}
