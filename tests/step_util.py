"""Helpers of the vr_tree_step tests: the numpy binary32 restatement of the step's arithmetic (include/volrend_hip.h),
the bitmap of touched slots, and what the tree holds afterwards (needs no GPU)."""
from __future__ import annotations

import numpy as np

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
