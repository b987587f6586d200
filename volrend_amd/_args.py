"""The one place where a caller's argument becomes a device address: ``_ptr`` / ``_stream_ptr`` for the frame
path, and ``check`` -- which every buffer argument of every operation goes through.  Imports no torch."""
from __future__ import annotations

from collections import namedtuple
from math import prod

F16, F32, I32, U8 = "float16", "float32", "int32", "uint8"
_TYPESTR = {"<f2": F16, "<f4": F32, "<i4": I32, "|u1": U8}
_TENSOR = ("data_ptr", "is_contiguous", "dtype", "shape", "is_cuda", "device")

# One buffer argument.  ``dtypes``: the names allowed.  ``shape``: the exact shape ("n": the call's row count) or
# None; ``count``: (elements, how the message words it) for buffers of any shape, or None.  ``rows``: the call's row
# count is this argument's -- a raw pointer here needs the caller's ``n``; the others are held to it.
Buf = namedtuple("Buf", "name x dtypes shape count rows", defaults=(None, None, False))


def _ptr(x) -> int | None:
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    raise TypeError(f"expected a device tensor or raw pointer, got {type(x)}")


def _stream_ptr(stream) -> int | None:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)  # torch.cuda.Stream


def placeholder(*ptrs):
    """The address passed where an empty tensor has none and nothing is read (n == 0, no poses): any non-NULL
    pointer of the call stands for it."""
    return next((p for p in ptrs if p), None)


def parse_want(want, known, empty_ok: bool = True) -> tuple:
    """``want``: a str or an iterable of names out of ``known``, each at most once."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in known for w in want) or len(set(want)) != len(want) or not (want or empty_ok):
        raise ValueError(f"want must name {'' if empty_ok else 'at least one of '}{sorted(known)}, each once: {want!r}")
    return want


class Checked:
    """What ``check`` found: ``ptr`` / ``dtype`` by argument name, the row count ``n``, and the tree's device,
    asked of the tree at most once."""

    def __init__(self, tree, n):
        self._tree, self._dev, self.ptr, self.dtype, self.n = tree, None, {}, {}, n

    def device_index(self) -> int:
        if self._dev is None:
            self._dev = int(self._tree.info()["device"])
        return self._dev


def check(tree, bufs, n=None) -> Checked:
    """Checks the buffer arguments ``bufs`` of one call.  Each is a tensor-like object (duck-typed), an object with
    ``__cuda_array_interface__`` or a raw device pointer (an int; nothing else can be checked of it, and a ray
    list of them needs ``n``).  In this order, each step over all arguments before the next: kind, dtype, shape or
    element count, contiguity, is_cuda -- none of which asks the tree anything -- then the device index against
    ``tree.info()``.  Every refusal is a ValueError naming the argument, raised before any C call."""
    c, seen, tensors = Checked(tree, n), [], []
    for b in bufs:
        x = b.x
        if isinstance(x, int) and not isinstance(x, bool):
            if n is None and b.rows:
                raise ValueError(f"{b.name} is a raw pointer: pass n")
            c.ptr[b.name], c.dtype[b.name] = x, None
        elif all(hasattr(x, a) for a in _TENSOR):
            c.ptr[b.name], c.dtype[b.name] = int(x.data_ptr()), str(x.dtype).replace("torch.", "")
            seen.append((b, tuple(x.shape), x.is_contiguous()))
            tensors.append((b.name, x))
        elif hasattr(x, "__cuda_array_interface__"):
            cai = x.__cuda_array_interface__
            c.ptr[b.name], c.dtype[b.name] = int(cai["data"][0]), _TYPESTR.get(cai["typestr"], cai["typestr"])
            seen.append((b, tuple(cai["shape"]), cai.get("strides") is None))
        else:
            raise ValueError(f"{b.name} must be a torch tensor on the device (a torch CUDA tensor or its like), expose "
                             f"__cuda_array_interface__ or be a raw device pointer, got {type(x)}")
    for b, _, _ in seen:
        if c.dtype[b.name] not in b.dtypes:
            raise ValueError(f"{b.name} must be {' or '.join(b.dtypes)}, not {c.dtype[b.name]}")
    for b, shape, _ in seen:
        if b.count is not None and prod(shape) != b.count[0]:
            raise ValueError(f"{b.name} must have {b.count[1]}, not {prod(shape)} of shape {shape}")
        if b.shape is not None:
            if c.n is None and b.rows and len(shape) == len(b.shape):
                c.n = int(shape[b.shape.index("n")])
            if shape != tuple(c.n if d == "n" else d for d in b.shape):
                raise ValueError(f"{b.name} must have shape [{', '.join(map(str, b.shape))}]"
                                 f"{'' if c.n is None else f' with n = {c.n}'}, not {shape}")
    for b, _, contiguous in seen:
        if not contiguous:
            raise ValueError(f"{b.name} must be contiguous")
    for name, x in tensors:
        if not x.is_cuda:
            raise ValueError(f"{name} must be on the tree's device, not {x.device}")
    for name, x in tensors:
        if x.device.index != c.device_index():
            raise ValueError(f"{name} must be on the tree's device cuda:{c.device_index()}, not {x.device}")
    if c.n is not None and c.n < 0:
        raise ValueError("n is negative")
    return c


def outputs(tree, inputs, specs, given, want, zeros: bool, n=None):
    """Checks ``inputs`` together with whichever outputs the caller passed (``given``: name -> buffer or None), then
    allocates those named in ``want`` and not passed.  ``specs``: name -> (dtype, shape) -> (Checked, dict name ->
    output)."""
    passed = {k: v for k, v in given.items() if v is not None}
    c = check(tree, list(inputs) + [Buf(k, v, (specs[k][0],), specs[k][1]) for k, v in passed.items()], n)
    return c, allocate(c, specs, passed, want, zeros)


def allocate(c: Checked, specs, passed, want, zeros: bool) -> dict:
    """The outputs of a checked call: what the caller ``passed``, and those named in ``want`` allocated on the tree's
    device (which a tensor input was just checked to be on)."""
    res = {}
    for name, (dt, shape) in specs.items():
        if name in passed:
            res[name] = passed[name]
        elif name in want:
            import torch
            res[name] = (torch.zeros if zeros else torch.empty)(
                tuple(c.n if d == "n" else d for d in shape), dtype=getattr(torch, dt),
                device=torch.device("cuda", c.device_index()))
            c.ptr[name] = int(res[name].data_ptr())
    return res
