"""The operations on an uploaded tree other than rendering frames: point queries, leaf weights, gradients, ray
lists, the values in place, the sparse step.  One function each: ``tree`` comes first and is duck-typed (``handle``,
``capacity``, ``N``, ``data_dim``, ``data_format``, ``info()``), and ``N3Tree`` binds the same function as a method,
so ``tree.render_rays(o, d, opts)`` is ``render_rays(tree, o, d, opts)``.

Every operation reads ``tree.handle`` first (a tree that is not on the device is refused before any argument is looked
at) and passes every buffer argument through ``_args.check``: a tensor-like object, an object with
``__cuda_array_interface__`` or a raw device pointer; what a caller passes as an output is returned as passed."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._args import F16, F32, I32, U8, _TYPESTR, Buf, _stream_ptr, allocate, check, outputs, parse_want, placeholder
from ._frame import Camera, RenderOptions, _cameras_c

_DATA_DTYPES = {F16: _abi.DATA_F16, F32: _abi.DATA_F32}


def _pose_chunks(cam: Camera, transforms):
    """``transforms`` in launches of at most ``_abi.MAX_BATCH`` poses -> (first, m, cams); no pose: one (0, 0, None)."""
    n = len(transforms)
    for first in range(0, max(n, 1), _abi.MAX_BATCH):
        m = min(_abi.MAX_BATCH, n - first)
        yield first, m, (_cameras_c(cam, [transforms[first + i] for i in range(m)]) if m else None)


def _marked_call(plain, marked, touched, *args, stream) -> None:
    """``plain``, or its ``_touched`` form ``marked`` with the bitmap's address when the caller wants the marks."""
    if touched is None:
        _abi.check(plain(*args, _stream_ptr(stream)))
    else:
        _abi.check(marked(*args, touched, _stream_ptr(stream)))


def _leaf_specs(tree) -> dict:
    shape = (tree.capacity, tree.N, tree.N, tree.N)
    return {"max_weight": (F32, shape), "hits": (I32, shape)}


def _leaf_weights_c(c) -> "_abi.VrLeafWeights":
    out = _abi.VrLeafWeights()
    out.max_weight, out.hits = c.ptr.get("max_weight"), c.ptr.get("hits")
    return out


def _data_buf(tree, name: str, x, dtypes=(F16, F32)) -> Buf:
    n = tree.capacity * tree.N ** 3 * tree.data_dim
    return Buf(name, x, dtypes, None, (n, f"capacity * N^3 * data_dim = {n} elements"))


def _touched_buf(tree, touched) -> Buf:
    n = touched_words(tree)
    return Buf("touched", touched, (I32,), None, (n, f"ceil(capacity * N^3 / 32) = {n} words"))


def _marks(tree, touched) -> list:
    """The optional ``touched=`` of the backward calls."""
    return [] if touched is None else [_touched_buf(tree, touched)]


def _touched_ptr(tree, touched) -> int:
    """Checks a ``touched`` bitmap -> its address."""
    return check(tree, [_touched_buf(tree, touched)]).ptr["touched"]


def _ray_bufs(origins, dirs) -> list:
    return [Buf("origins", origins, (F32,), ("n", 3), rows=True), Buf("dirs", dirs, (F32,), ("n", 3), rows=True)]


def _rays_c(c) -> "_abi.VrRays":
    rays = _abi.VrRays()
    rays.origins, rays.dirs = c.ptr["origins"], c.ptr["dirs"]
    return rays


# ---- bulk point queries (vr_query_points / vr_query_grid) --------------
def _query_outputs(tree, c, want, shape, have_dirs: bool, space: str):
    """Checks ``want`` / ``space`` and allocates the outputs [*shape(, k)] of the checked call ``c`` on the tree's
    device -> (dict of tensors, VrQueryOut, space code).  Raises ValueError before any C call."""
    widths = {"sigma": 0, "depth": 0, "local": 3, "coeffs": tree.data_dim - 1, "rgb": 3}
    want = parse_want(want, widths, empty_ok=False)
    if space not in _abi.SPACES:
        raise ValueError(f"space must be 'world' or 'tree', not {space!r}")
    if "rgb" in want and not have_dirs:
        raise ValueError("rgb needs directions")
    if "rgb" in want and tree.data_format[0] in ("SG", "ASG"):
        raise ValueError("rgb of SG / ASG trees is not supported by the point queries")
    specs = {w: (I32 if w == "depth" else F32, tuple(shape) + ((k,) if k else ())) for w, k in widths.items()}
    res = allocate(c, specs, {}, want, zeros=False)
    out = _abi.VrQueryOut()
    for w in want:
        setattr(out, w, c.ptr[w])
    return {w: res[w] for w in want}, out, _abi.SPACES[space]


def query_points(tree, points, dirs=None, *, want=("sigma",), space: str = "world", stream=None, n=None) -> dict:
    """What the tree holds at ``points`` [n, 3] (float32, contiguous, on the tree's device; or a
    raw device pointer with ``n``) -- vr_query_points, one launch, enqueued on ``stream``.

    ``want``: any of "sigma" [n], "depth" [n] int32, "local" [n, 3], "coeffs" [n, data_dim - 1],
    "rgb" [n, 3] (needs ``dirs`` [n, 3]; evaluated at the direction AS GIVEN, not normalised;
    strict model).  ``space``: "world" (offset + scale * x is applied) or "tree".  Returns a dict
    of torch tensors on the tree's device."""
    handle = tree.handle
    c = check(tree, [Buf(name, x, (F32,), ("n", 3), rows=True) for name, x in (("points", points), ("dirs", dirs))
                     if x is not None or name == "points"], n)
    res, out, sp = _query_outputs(tree, c, want, ("n",), dirs is not None, space)
    if c.n == 0:  # (empty tensors have no address to pass)
        return res
    _abi.check(_abi.lib().vr_query_points(handle, c.n, c.ptr["points"], c.ptr.get("dirs"), sp, C.byref(out),
                                          _stream_ptr(stream)))
    return res


def query_grid(tree, lo, hi, res, dir=None, *, want=("sigma",), space: str = "world", stream=None) -> dict:
    """The same at the res[0] x res[1] x res[2] cell centres of the box ``lo``..``hi``, generated
    on the device (vr_query_grid): cell (i, j, k) sits at lo + (i + 0.5) * ((hi - lo) / res) per
    axis, in float32.  ``dir``: one direction for all cells (needed for "rgb").  Returns tensors
    shaped [res0, res1, res2(, k)]."""
    handle = tree.handle
    vals = []
    for name, v, dt in (("lo", lo, np.float32), ("hi", hi, np.float32), ("res", res, np.int64),
                        ("dir", dir, np.float32)):
        if v is None and name == "dir":
            vals.append(None)
            continue
        a = np.asarray(v)
        if a.shape != (3,) or (name == "res" and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{name} must be 3 {'integers' if name == 'res' else 'numbers'}")
        vals.append(a.astype(dt))
    lo_a, hi_a, res_a, dir_a = vals
    if (res_a < 1).any() or (res_a > 2 ** 31 - 1).any() or int(res_a.prod(dtype=object)) > 2 ** 40:
        raise ValueError(f"res must be positive with at most 2^40 cells in all: {tuple(res_a)}")
    out_t, out, sp = _query_outputs(tree, check(tree, []), want, tuple(int(r) for r in res_a), dir_a is not None,
                                    space)
    c_lo, c_hi = (C.c_float * 3)(*map(float, lo_a)), (C.c_float * 3)(*map(float, hi_a))
    c_res = (C.c_int32 * 3)(*[int(r) for r in res_a])
    c_dir = None if dir_a is None else C.byref((C.c_float * 3)(*map(float, dir_a)))
    _abi.check(_abi.lib().vr_query_grid(handle, C.byref(c_lo), C.byref(c_hi), C.byref(c_res), c_dir,
                                        sp, C.byref(out), _stream_ptr(stream)))
    return out_t


# ---- per-leaf ray weights (vr_accumulate_weights) -----------------------
def accumulate_weights(tree, cam: Camera, transforms, options: RenderOptions, *, max_weight=None, hits=None,
                       want=("max_weight",), fp_mode: int = _abi.FP_STRICT, stream=None) -> dict:
    """Per leaf slot, over every pixel of every pose of ``transforms`` (12 floats each, as
    ``launch_renderer_batch`` takes them): the largest compositing weight a sample in the slot received
    ("max_weight", float32) and the number of hit samples in it ("hits", a uint32 count held in an int32
    tensor) -- vr_accumulate_weights, enqueued on ``stream``, one launch per 512 poses.

    Returns a dict of torch tensors shaped [capacity, N, N, N], indexed like the file's ``child`` /
    ``data`` arrays.  ``want`` names the outputs; a buffer passed as ``max_weight`` / ``hits`` is wanted
    too and is ACCUMULATED INTO (it must be contiguous, on the tree's device, and -- max_weight -- hold
    non-negative, non-NaN floats); the others are allocated zeroed.  Any split of a pose set into calls
    gives the same bits.  Of ``options`` only step_size, sigma_thresh, stop_thresh and render_bbox are
    read.  No poses: only the tree's file-order table is put on the device (the warm-up call)."""
    handle = tree.handle
    want = parse_want(want, ("max_weight", "hits"))
    c, res = outputs(tree, [], _leaf_specs(tree), {"max_weight": max_weight, "hits": hits}, want, zeros=True)
    L, o, out = _abi.lib(), options.to_c(), _leaf_weights_c(c)
    for _, m, cams in _pose_chunks(cam, transforms):
        _abi.check(L.vr_accumulate_weights(handle, m, cams, C.byref(o), int(fp_mode), C.byref(out),
                                           _stream_ptr(stream)))
    return res


# ---- gradients of a rendered batch (vr_render_backward) ----------------
def touched_words(tree) -> int:
    """Words of a ``touched`` bitmap of this tree: ceil(capacity * N^3 / 32)."""
    _ = tree.handle  # (a tree that is not on the device is refused, as by every operation)
    return (tree.capacity * tree.N ** 3 + 31) // 32


def render_backward(tree, cam: Camera, transforms, options: RenderOptions, grad_accum, *, grad_data=None,
                    fp_mode: int = _abi.FP_STRICT, stream=None, touched=None):
    """The derivative of a rendered batch with respect to the tree's values -- vr_render_backward,
    enqueued on ``stream``, one launch per 512 poses.

    ``grad_accum``: float32 [len(transforms), height, width, 4], contiguous, on the tree's device:
    dL/d of the four numbers ``accums`` of ``launch_renderer_batch`` receive per pixel.  Returns the
    float32 buffer [capacity, N, N, N, data_dim], indexed like the file's ``data`` array, that the
    contributions were ADDED into: ``grad_data`` when given (contiguous, float32), else one allocated
    zeroed.  The sum uses float atomics: two runs may differ in the last bits.  The march is that of
    ``accumulate_weights`` (offscreen, no mesh depth); render_depth, enable_probe, rot_dirs, a narrowed
    basis_minmax and SG / ASG trees are refused.

    ``touched``: an int32 buffer of ``touched_words()`` words selects the marked call
    (vr_render_backward_touched): the bit of every slot the call adds into is ORed into it -- bit s & 31 of
    word s >> 5, s = file node * N^3 + child slot; zero it once.  The marks are bit-reproducible; ``step``
    consumes them."""
    handle = tree.handle
    shape_d = (tree.capacity, tree.N, tree.N, tree.N, tree.data_dim)
    bufs = [Buf("grad_accum", grad_accum, (F32,), (len(transforms), cam.height, cam.width, 4))]
    c, res = outputs(tree, bufs + _marks(tree, touched), {"grad_data": (F32, shape_d)},
                     {"grad_data": grad_data}, ("grad_data",), zeros=True)
    L, o, g, d = _abi.lib(), options.to_c(), c.ptr["grad_accum"], c.ptr["grad_data"]
    frame_bytes = cam.height * cam.width * 16
    for first, m, cams in _pose_chunks(cam, transforms):
        _marked_call(L.vr_render_backward, L.vr_render_backward_touched, c.ptr.get("touched"), handle, m, cams,
                     C.byref(o), int(fp_mode), g + first * frame_bytes if m else placeholder(g, d), d, stream=stream)
    return res["grad_data"]


# ---- ray lists (vr_render_rays / vr_accumulate_weights_rays / vr_render_backward_rays / vr_fit_rays) ----
def render_rays(tree, origins, dirs, options: RenderOptions, *, want=("accum",), rgba=None, accum=None,
                fp_mode: int = _abi.FP_STRICT, stream=None, n=None) -> dict:
    """Colour along caller-supplied rays -- vr_render_rays, one launch, enqueued on ``stream``.

    ``origins`` / ``dirs``: float32 [n, 3], contiguous, on the tree's device, world space; a direction may have
    any finite non-zero length (or raw device pointers with ``n``).  Ray i is the ray of a pixel entered
    behind screen2worlddir's matrix product: the direction is normalised, then everything an offscreen frame
    does follows, so a list built from a camera gives that frame's bits.  ``want``: "accum" (float32 [n, 4]:
    trace_ray's output before the composite) and / or "rgba" (uint8 [n, 4]: composited over
    background_brightness); a buffer passed as ``rgba`` / ``accum`` is wanted too and is written.  Returns a
    dict of torch tensors.  64 consecutive rays share a wave; the library does not reorder them (``order_rays``
    computes an order to apply).
    render_depth and enable_probe are refused."""
    handle = tree.handle
    want = parse_want(want, ("rgba", "accum"))
    c, res = outputs(tree, _ray_bufs(origins, dirs), {"rgba": (U8, ("n", 4)), "accum": (F32, ("n", 4))},
                     {"rgba": rgba, "accum": accum}, want, zeros=False, n=n)
    if not res:
        raise ValueError("no output is wanted: name 'rgba' and / or 'accum'")
    if c.n == 0:  # (empty tensors have no address to pass, and nothing would be launched)
        return res
    out, rays, o = _abi.VrRayOut(), _rays_c(c), options.to_c()
    out.rgba, out.accum = c.ptr.get("rgba"), c.ptr.get("accum")
    _abi.check(_abi.lib().vr_render_rays(handle, c.n, C.byref(rays), C.byref(o), int(fp_mode), C.byref(out),
                                         _stream_ptr(stream)))
    return res


def accumulate_weights_rays(tree, origins, dirs, options: RenderOptions, *, max_weight=None, hits=None,
                            want=("max_weight",), fp_mode: int = _abi.FP_STRICT, stream=None, n=None) -> dict:
    """``accumulate_weights`` over the rays of a list (as ``render_rays`` takes them) --
    vr_accumulate_weights_rays, one launch.  No rays: only the file-order table is put on the device."""
    handle = tree.handle
    want = parse_want(want, ("max_weight", "hits"))
    c, res = outputs(tree, _ray_bufs(origins, dirs), _leaf_specs(tree), {"max_weight": max_weight, "hits": hits},
                     want, zeros=True, n=n)
    out, rays, o = _leaf_weights_c(c), _rays_c(c), options.to_c()
    if c.n == 0:
        rays.origins = rays.dirs = placeholder(out.max_weight, out.hits)
    _abi.check(_abi.lib().vr_accumulate_weights_rays(handle, c.n, C.byref(rays), C.byref(o), int(fp_mode),
                                                     C.byref(out), _stream_ptr(stream)))
    return res


def render_backward_rays(tree, origins, dirs, options: RenderOptions, grad_accum, *, grad_data=None,
                         fp_mode: int = _abi.FP_STRICT, stream=None, n=None, touched=None):
    """``render_backward`` over the rays of a list (as ``render_rays`` takes them) -- vr_render_backward_rays,
    one launch.  ``grad_accum``: float32 [n, 4], row i for ray i: dL/d of the four numbers ``render_rays``
    returns as "accum".  Returns the float32 buffer [capacity, N, N, N, data_dim] added into.  ``touched``: as
    ``render_backward`` takes it (vr_render_backward_rays_touched)."""
    handle = tree.handle
    bufs = _ray_bufs(origins, dirs) + [Buf("grad_accum", grad_accum, (F32,), ("n", 4))]
    c, res = outputs(tree, bufs + _marks(tree, touched),
                     {"grad_data": (F32, (tree.capacity, tree.N, tree.N, tree.N, tree.data_dim))},
                     {"grad_data": grad_data}, ("grad_data",), zeros=True, n=n)
    rays, o, g, d = _rays_c(c), options.to_c(), c.ptr["grad_accum"], c.ptr["grad_data"]
    if c.n == 0:
        rays.origins = rays.dirs = g = d
    L = _abi.lib()
    _marked_call(L.vr_render_backward_rays, L.vr_render_backward_rays_touched, c.ptr.get("touched"), handle, c.n,
                 C.byref(rays), C.byref(o), int(fp_mode), g, d, stream=stream)
    return res["grad_data"]


def fit_rays(tree, origins, dirs, options: RenderOptions, target, *, grad_scale, grad_data=None, touched=None,
             want=("sq_err",), fp_mode: int = _abi.FP_STRICT, n=None, stream=None) -> dict:
    """The L2 loss of the rays of a list against ``target`` and its gradient with respect to the tree's values --
    vr_fit_rays, one launch: what ``render_rays`` ("accum"), the composite over background_brightness, the
    residual and the marked ``render_backward_rays`` compute in sequence.

    ``origins`` / ``dirs``: as ``render_rays`` takes them.  ``target``: float32 [n, 3], the colour ray i should
    have.  ``grad_scale``: a finite number; the loss is grad_scale / 2 * sum r^2 over rays and channels, r the
    composite minus the target -- 2 / (3 n) for the mean.  ``grad_data`` / ``touched``: as ``render_backward_rays``
    takes them (added into / ORed into; ``grad_data`` is allocated zeroed when not given).  ``want``: "sq_err"
    (float32 [n]: r_0^2 + r_1^2 + r_2^2 per ray) and / or "accum" (float32 [n, 4]: the bits of ``render_rays``),
    or neither.  Returns a dict of torch tensors: "grad_data" and what ``want`` names.  include/volrend_hip.h has
    the operations of the loss head; "sq_err" and "accum" are bit-reproducible."""
    handle = tree.handle
    want = parse_want(want, ("sq_err", "accum"))
    scale = float(grad_scale)
    if not abs(scale) <= float(np.finfo(np.float32).max):   # (NaN fails the comparison too)
        raise ValueError(f"grad_scale must be a finite float32, not {grad_scale!r}")
    bufs = _ray_bufs(origins, dirs) + [Buf("target", target, (F32,), ("n", 3))]
    c, res = outputs(tree, bufs + _marks(tree, touched),
                     {"grad_data": (F32, (tree.capacity, tree.N, tree.N, tree.N, tree.data_dim))},
                     {"grad_data": grad_data}, ("grad_data",), zeros=True, n=n)
    res.update(allocate(c, {"sq_err": (F32, ("n",)), "accum": (F32, ("n", 4))}, {}, want, zeros=False))
    rays, o, fit = _rays_c(c), options.to_c(), _abi.VrFit()
    fit.target, fit.grad_scale, fit.grad_data = c.ptr["target"], scale, c.ptr["grad_data"]
    fit.touched = c.ptr.get("touched")
    if c.n == 0:  # (empty tensors have no address to pass; the call only uploads the file-order table)
        rays.origins = rays.dirs = fit.target = fit.grad_data
    else:
        fit.sq_err, fit.accum = c.ptr.get("sq_err"), c.ptr.get("accum")
    _abi.check(_abi.lib().vr_fit_rays(handle, c.n, C.byref(rays), C.byref(o), int(fp_mode), C.byref(fit),
                                      _stream_ptr(stream)))
    return res


# ---- the order that makes a ray list coherent (vr_order_rays) ----
_ORDER_OUT = {"order": "order", "keys": "keys", "origins": "origins_out", "dirs": "dirs_out", "payload": "payload_out"}


def order_rays(tree, origins, dirs, options: RenderOptions, *, bits: int = 0, payload=None,
               want=("order", "origins", "dirs"), out=None, workspace=None, fp_mode: int = _abi.FP_STRICT, stream=None,
               n=None, payload_dim=None) -> dict:
    """The order in which the rays of a list are coherent, and the list gathered into it -- vr_order_rays, enqueued
    on ``stream``; no launch slot, the tree is only read.

    ``origins`` / ``dirs``: as ``render_rays`` takes them.  Each ray gets a key from where it enters and leaves the
    volume in tree coordinates (set up as the ray-list launches set it up in ``fp_mode``; of ``options`` only
    render_bbox is read): a 6-D Morton code of ``bits`` bits per coordinate (1..5; 0 = the library's default), all
    ones for a ray that misses.  "order" (int32 [n]) is the stable sort of 0..n-1 by that key -- unique and
    bit-reproducible; ``order[j]`` is the index of the ray at sorted position j.  ``want``: any of "order" (always
    produced), "keys" (int32 [n]: the sorted keys' bits), "origins" / "dirs" (float32 [n, 3]: the rows in sorted
    order, bit copies) -- and "payload" (float32 [n, k]) is produced whenever ``payload`` (float32 [n, k], k in 1..8,
    e.g. the targets of ``fit_rays``; a raw pointer needs ``payload_dim``) is given.  ``out``: a dict of buffers to
    write instead of allocating, by the same names; none may be its own input.  ``workspace``: a uint8 buffer of at
    least vr_order_rays_workspace(n) bytes, 256-byte aligned; allocated when not given.

    Returns a dict of torch tensors by those names, plus "workspace" (keep the dict until the work on ``stream`` is
    done).  Feed "origins" / "dirs" / "payload" to any ray-list call; a per-ray output ``y`` of that call goes back
    to the caller's order as ``x = torch.empty_like(y); x[order.long()] = y``."""
    handle = tree.handle
    want = parse_want(want, tuple(_ORDER_OUT))
    out = dict(out or {})
    if any(k not in _ORDER_OUT for k in out):
        raise ValueError(f"out names {sorted(_ORDER_OUT)}, not {sorted(out)!r}")
    if not isinstance(bits, int) or isinstance(bits, bool) or not 0 <= bits <= _abi.ORDER_MAX_BITS:
        raise ValueError(f"bits must be an integer in 0..{_abi.ORDER_MAX_BITS}, not {bits!r}")
    k = payload_dim
    if payload is None:
        if "payload" in want or out.get("payload") is not None or payload_dim is not None:
            raise ValueError("a gathered payload needs payload")
    else:
        shape = getattr(payload, "shape", None) or getattr(payload, "__cuda_array_interface__", {}).get("shape")
        if k is None and shape is not None and len(shape) == 2:
            k = int(shape[1])
        if k is None:
            raise ValueError("payload must have shape [n, k]; a raw pointer needs payload_dim")
        if not isinstance(k, int) or not 1 <= k <= _abi.ORDER_MAX_PAYLOAD:
            raise ValueError(f"payload must have 1..{_abi.ORDER_MAX_PAYLOAD} columns, not {k!r}")
    bufs = _ray_bufs(origins, dirs)
    if payload is not None:
        bufs.append(Buf("payload", payload, (F32,), ("n", k)))
    if workspace is not None:
        bufs.append(Buf("workspace", workspace, (U8,)))
    specs = {"order": (I32, ("n",)), "keys": (I32, ("n",)), "origins_out": (F32, ("n", 3)),
             "dirs_out": (F32, ("n", 3)), "payload_out": (F32, ("n", k or 0))}
    names = [_ORDER_OUT[w] for w in want] + ["order"] + (["payload_out"] if payload is not None else [])
    c, res = outputs(tree, bufs, specs, {_ORDER_OUT[w]: v for w, v in out.items()}, names, zeros=False, n=n)
    for a, b in (("origins", "origins_out"), ("dirs", "dirs_out"), ("payload", "payload_out")):
        if c.n and c.ptr.get(b) is not None and c.ptr.get(b) == c.ptr.get(a):
            raise ValueError(f"out[{a!r}] is its own input: the gather is not in place")
    result = {w: res[name] for w, name in _ORDER_OUT.items() if name in res}
    if c.n == 0:  # (empty tensors have no address to pass, and nothing would be enqueued)
        return result
    L = _abi.lib()
    need = int(L.vr_order_rays_workspace(c.n))
    if workspace is None:
        import torch
        workspace = torch.empty(need, dtype=torch.uint8, device=torch.device("cuda", c.device_index()))
        c.ptr["workspace"], have = int(workspace.data_ptr()), need
    else:   # (a raw pointer is taken to be large enough; the library checks what it is told)
        have = need if isinstance(workspace, int) else int(np.prod(_shape_of(workspace), dtype=np.int64))
    ro, rays, o = _abi.VrRayOrder(), _rays_c(c), options.to_c()
    ro.bits, ro.payload, ro.payload_dim = bits, c.ptr.get("payload"), k or 0
    for name in ("order", "keys", "origins_out", "dirs_out", "payload_out"):
        setattr(ro, name, c.ptr.get(name))
    _abi.check(L.vr_order_rays(handle, c.n, C.byref(rays), C.byref(o), int(fp_mode), C.byref(ro), c.ptr["workspace"],
                               have, _stream_ptr(stream)))
    result["workspace"] = workspace
    return result


def _shape_of(x) -> tuple:
    return tuple(x.shape) if hasattr(x, "shape") else tuple(x.__cuda_array_interface__["shape"])


# ---- the values of the device copy, in place (vr_tree_update_data / vr_tree_read_data) ----
def _data_dtype(dtype) -> str:
    """torch.float16 / torch.float32 (or their names, or a __cuda_array_interface__ typestr) -> the name."""
    name = _TYPESTR.get(dtype) if isinstance(dtype, str) and dtype in _TYPESTR else str(dtype).replace("torch.", "")
    if name not in _DATA_DTYPES:
        raise ValueError(f"the tree's data must be float16 or float32, not {dtype}")
    return name


def update_data(tree, data, stream=None) -> None:
    """Overwrites the values of the DEVICE copy with ``data`` -- vr_tree_update_data, enqueued on ``stream``:
    the step after ``render_backward`` once the optimiser has moved its master parameters.

    ``data``: a torch CUDA tensor (or any object with ``__cuda_array_interface__``) of dtype float16 or
    float32 with capacity * N^3 * data_dim elements, contiguous, on the tree's device, indexed like the
    file's ``data`` array ([capacity, N, N, N, data_dim], record [R.., G.., B.., sigma]); a raw device pointer
    is taken to hold float16.  float32 is rounded to float16 to nearest even, as ``numpy.astype(float16)``
    rounds.  Afterwards the device copy is bit for bit what a fresh upload of this array would be; the sigma of
    internal slots is ignored.

    The update WRITES the tree: launches and queries enqueued later on the same stream see the new values,
    work on other streams has to be ordered with events, and nothing may read the tree while it runs.  The
    host arrays of the tree object are NOT touched: ``data_`` goes stale, and ``load_device()`` from it would
    undo the update (``read_data`` returns what the device holds)."""
    handle = tree.handle
    c = check(tree, [_data_buf(tree, "data", data)])
    _abi.check(_abi.lib().vr_tree_update_data(handle, c.ptr["data"], _DATA_DTYPES[c.dtype["data"] or F16],
                                              _stream_ptr(stream)))


def read_data(tree, dtype=None, out=None, stream=None):
    """The current values of the DEVICE copy in file order -- vr_tree_read_data, enqueued on ``stream``: a
    torch tensor [capacity, N, N, N, data_dim] of ``dtype`` (torch.float16, the default, or torch.float32:
    the exact widening) on the tree's device; ``out`` when given (contiguous, that many elements; its dtype
    decides, ``dtype`` for a raw pointer).  The bits are those uploaded or last written, the sigma of internal
    slots +0.  Works where the host arrays are gone (``clear_cpu_memory``, a quantised upload, a clone)."""
    handle = tree.handle
    name = None if dtype is None else _data_dtype(dtype)
    if out is None:
        shape = (tree.capacity, tree.N, tree.N, tree.N, tree.data_dim)
        c, res = outputs(tree, [], {"out": (name or F16, shape)}, {}, ("out",), zeros=False)
        out = res["out"]
    else:
        c = check(tree, [_data_buf(tree, "out", out)])
        if name not in (None, c.dtype["out"] or name):
            raise ValueError(f"out is not of dtype {dtype}")
    _abi.check(_abi.lib().vr_tree_read_data(handle, c.ptr["out"], _DATA_DTYPES[c.dtype.get("out") or name or F16],
                                            _stream_ptr(stream)))
    return out


# ---- a tree with selected leaves subdivided (vr_refine_plan / vr_refine_apply) ----
def _pack_bits(flags):
    """bool tensor [n] -> the int32 bitmap of the ``touched`` format: bit s & 31 of word s >> 5."""
    import torch
    n = flags.numel()
    words = (n + 31) // 32
    bits = torch.zeros(words * 32, dtype=torch.int64, device=flags.device)
    bits[:n] = flags.reshape(-1)
    w = (bits.reshape(words, 32) << torch.arange(32, dtype=torch.int64, device=flags.device)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def refine(tree, sel, companions=(), stream=None) -> dict:
    """A NEW tree in which the selected leaves of ``tree`` are subdivided into N^3 leaves that hold their parent's
    values -- vr_refine_plan / vr_refine_apply on the tree's binary16 values (``read_data``) and its child array,
    then an upload of the result from device memory (``N3Tree.from_device_arrays``).  No value crosses to the host.

    ``sel``: a bool tensor of capacity * N^3 elements (any shape), or the int32 bitmap of ``touched_words()`` words
    (bit s & 31 of word s >> 5, s = file node * N^3 + child slot).  A set bit refines its slot if the slot is a
    leaf; bits of internal slots are ignored.  The refinement is append-only in the file's numbering: old nodes and
    slots keep their indices, the r-th refined slot in ascending order becomes node capacity + r.
    ``companions``: up to 7 ``(tensor, fill)`` pairs, each tensor float16 / float32 / int32 with capacity * N^3 * k
    elements indexed like the file's ``data`` array (a float32 master, Adam moments, leaf weights ...); ``fill``
    says what the slots of new nodes get: "copy" (the refined slot's elements) or "zero".

    Returns {"tree": the new ``N3Tree`` (same geometry, format, ``extra`` and NDC), "companions": the restated
    tensors [capacity + n_new, ...] in order, "src_slot": int32 [n_new], the slot new node capacity + r came from,
    "n_new": int}.  Host-blocking (the plan's count and the upload).  The old tree stays valid; the caller frees it."""
    _ = tree.handle
    N3 = tree.N ** 3
    n_slots, words = tree.capacity * N3, touched_words(tree)
    companions = [tuple(p) if isinstance(p, (tuple, list)) else (p,) for p in companions]
    if len(companions) + 1 > _abi.REFINE_MAX_ARRAYS:
        raise ValueError(f"at most {_abi.REFINE_MAX_ARRAYS - 1} companions, not {len(companions)}")
    packed = str(getattr(sel, "dtype", "")).replace("torch.", "") == "bool"
    bufs = [Buf("sel", sel, ("bool",), None, (n_slots, f"capacity * N^3 = {n_slots} flags")) if packed else
            _touched_buf(tree, sel)._replace(name="sel")]
    dims = []
    for i, p in enumerate(companions):
        if len(p) != 2 or p[1] not in _abi.REFINE_FILLS:
            raise ValueError(f"companions[{i}] must be (tensor, 'copy' or 'zero')")
        count = int(np.prod(_shape_of(p[0]), dtype=np.int64)) if hasattr(p[0], "shape") or hasattr(
            p[0], "__cuda_array_interface__") else 0
        if count < n_slots or count % n_slots:
            raise ValueError(f"companions[{i}] must have capacity * N^3 * k = {n_slots} * k elements, not {count}")
        dims.append(count // n_slots)
        bufs.append(Buf(f"companions[{i}]", p[0], (F16, F32, I32)))
    c = check(tree, bufs)
    import torch
    from ._tree import N3Tree
    device = torch.device("cuda", c.device_index())
    L, sp = _abi.lib(), _stream_ptr(stream)
    with torch.cuda.device(device):
        if packed:
            sel = _pack_bits(sel)
            torch.cuda.current_stream(device).synchronize()   # (torch's stream need not be ``stream``)
        data = read_data(tree, stream=stream)
        child = torch.from_numpy(np.ascontiguousarray(tree.child_, dtype=np.int32)).to(device)
        ws = torch.empty(int(L.vr_refine_workspace(tree.N, tree.capacity)), dtype=torch.uint8, device=device)
        r = _abi.VrRefine()
        r.child, r.sel = child.data_ptr(), int(sel.data_ptr()) if packed else c.ptr["sel"]
        r.workspace, r.workspace_bytes = ws.data_ptr(), ws.numel()
        r.capacity, r.N = tree.capacity, tree.N
        n_new = C.c_int64(0)
        _abi.check(L.vr_refine_plan(C.byref(r), C.byref(n_new), sp))
        n_new = int(n_new.value)
        cap = tree.capacity + n_new
        child_out = torch.empty((cap, tree.N, tree.N, tree.N), dtype=torch.int32, device=device)
        src_slot = torch.empty(n_new, dtype=torch.int32, device=device)
        data_out = torch.empty((cap, tree.N, tree.N, tree.N, tree.data_dim), dtype=torch.float16, device=device)
        outs = [torch.empty((cap, tree.N, tree.N, tree.N, k) if k > 1 else (cap, tree.N, tree.N, tree.N),
                            dtype=getattr(torch, c.dtype[f"companions[{i}]"]), device=device)
                for i, k in enumerate(dims)]
        arrays = (_abi.VrRefineArray * (len(outs) + 1))()
        srcs = [data.data_ptr()] + [c.ptr[f"companions[{i}]"] for i in range(len(companions))]
        for a, src, dst, k, fill in zip(arrays, srcs, [data_out] + outs, [tree.data_dim] + dims,
                                        ["copy"] + [p[1] for p in companions]):
            a.src, a.dst, a.elem_bytes, a.dim, a.fill = src, dst.data_ptr(), dst.element_size(), k, \
                _abi.REFINE_FILLS[fill]
        r.child_out, r.src_slot, r.n_new = child_out.data_ptr(), src_slot.data_ptr() if n_new else None, n_new
        r.arrays, r.n_arrays = arrays, len(arrays)
        _abi.check(L.vr_refine_apply(C.byref(r), sp))
        _abi.check(L.vr_stream_sync(sp))   # (the upload reads the arrays on streams of its own)
        new = N3Tree.from_device_arrays(child_out, data_out, tree.offset, tree.scale, tree.data_format,
                                        extra=getattr(tree, "extra_", None),
                                        ndc=(tree.ndc_width, tree.ndc_height, tree.ndc_focal) if tree.use_ndc else None)
    return {"tree": new, "companions": outs, "src_slot": src_slot, "n_new": n_new}


# ---- a tree with selected frontier nodes collapsed and the node array compacted (vr_collapse_plan / _apply) ----
def collapse(tree, sel, companions=(), values="mean", stream=None) -> dict:
    """A NEW tree in which the selected frontier nodes of ``tree`` (nodes all of whose slots are leaves) are merged
    into the parent slot that links to them, and the node array is compacted -- vr_collapse_plan / vr_collapse_apply
    on the tree's binary16 values (``read_data``) and its child array, then an upload of the result from device memory
    (``N3Tree.from_device_arrays``).  No value crosses to the host.  One level per call: repeat it to collapse deeper.

    ``sel``: a bool tensor of ``capacity`` elements, one per NODE, or the int32 bitmap of ceil(capacity / 32) words
    (bit m & 31 of word m >> 5) -- e.g. ``max_weight.view(capacity, -1).amax(1) < t``.  A set bit collapses its node
    if the node is a frontier node; bit 0 (the root) and bits of other nodes are ignored.  The kept nodes keep their
    relative order: the p-th kept node in ascending old index is new node p.
    ``companions``: up to 7 ``(tensor, rule)`` pairs, each tensor float16 / float32 / int32 with capacity * N^3 * k
    elements indexed like the file's ``data`` array; the slots of kept nodes move with their node, and ``rule`` says
    what a merged slot (the parent slot of a collapsed node) gets: "keep" (what it held), "zero", or "mean" (float16 /
    float32 only: per element the mean over the collapsed node's N^3 slots, summed in float32 in ascending slot order).
    ``values``: the rule for the tree's own values.  ``read_data`` reports the sigma of internal slots as +0, so
    "keep" produces EMPTY leaves (their coefficients are what the file held); "mean", the default, is svox's merge.

    Returns {"tree": the new ``N3Tree`` (same geometry, format, ``extra`` and NDC), "companions": the restated
    tensors [n_keep, ...] in order, "node_map": int32 [capacity], the new index of an old node or -1, "src_node":
    int32 [n_keep], the old index of a new node, "into_slot": int32 [capacity], the new slot a collapsed node went
    into or -1, "n_keep": int}.  Host-blocking (the plan's count and the upload).  The old tree stays valid; the caller
    frees it."""
    _ = tree.handle
    N3, cap = tree.N ** 3, tree.capacity
    n_slots, words = cap * N3, (cap + 31) // 32
    companions = [tuple(p) if isinstance(p, (tuple, list)) else (p,) for p in companions]
    if len(companions) + 1 > _abi.COLLAPSE_MAX_ARRAYS:
        raise ValueError(f"at most {_abi.COLLAPSE_MAX_ARRAYS - 1} companions, not {len(companions)}")
    if values not in _abi.COLLAPSE_RULES:
        raise ValueError(f"values names 'keep', 'zero' or 'mean', not {values!r}")
    packed = str(getattr(sel, "dtype", "")).replace("torch.", "") == "bool"
    bufs = [Buf("sel", sel, ("bool",), None, (cap, f"capacity = {cap} flags")) if packed else
            Buf("sel", sel, (I32,), None, (words, f"ceil(capacity / 32) = {words} words"))]
    dims = []
    for i, p in enumerate(companions):
        if len(p) != 2 or p[1] not in _abi.COLLAPSE_RULES:
            raise ValueError(f"companions[{i}] must be (tensor, 'keep', 'zero' or 'mean')")
        count = int(np.prod(_shape_of(p[0]), dtype=np.int64)) if hasattr(p[0], "shape") or hasattr(
            p[0], "__cuda_array_interface__") else 0
        if count < n_slots or count % n_slots:
            raise ValueError(f"companions[{i}] must have capacity * N^3 * k = {n_slots} * k elements, not {count}")
        dims.append(count // n_slots)
        bufs.append(Buf(f"companions[{i}]", p[0], (F16, F32) if p[1] == "mean" else (F16, F32, I32)))
    c = check(tree, bufs)
    import torch
    from ._tree import N3Tree
    device = torch.device("cuda", c.device_index())
    L, sp = _abi.lib(), _stream_ptr(stream)
    with torch.cuda.device(device):
        if packed:
            sel = _pack_bits(sel)
            torch.cuda.current_stream(device).synchronize()   # (torch's stream need not be ``stream``)
        data = read_data(tree, stream=stream)
        child = torch.from_numpy(np.ascontiguousarray(tree.child_, dtype=np.int32)).to(device)
        ws = torch.empty(int(L.vr_collapse_workspace(tree.N, cap)), dtype=torch.uint8, device=device)
        r = _abi.VrCollapse()
        r.child, r.sel = child.data_ptr(), int(sel.data_ptr()) if packed else c.ptr["sel"]
        r.workspace, r.workspace_bytes = ws.data_ptr(), ws.numel()
        r.capacity, r.N = cap, tree.N
        n_keep = C.c_int64(0)
        _abi.check(L.vr_collapse_plan(C.byref(r), C.byref(n_keep), sp))
        n_keep = int(n_keep.value)
        node = (n_keep, tree.N, tree.N, tree.N)
        child_out = torch.empty(node, dtype=torch.int32, device=device)
        node_map, into_slot = (torch.empty(cap, dtype=torch.int32, device=device) for _ in range(2))
        src_node = torch.empty(n_keep, dtype=torch.int32, device=device)
        data_out = torch.empty(node + (tree.data_dim,), dtype=torch.float16, device=device)
        outs = [torch.empty(node + ((k,) if k > 1 else ()), dtype=getattr(torch, c.dtype[f"companions[{i}]"]),
                            device=device) for i, k in enumerate(dims)]
        arrays = (_abi.VrCollapseArray * (len(outs) + 1))()
        srcs = [data.data_ptr()] + [c.ptr[f"companions[{i}]"] for i in range(len(companions))]
        for a, src, dst, k, rule in zip(arrays, srcs, [data_out] + outs, [tree.data_dim] + dims,
                                        [values] + [p[1] for p in companions]):
            a.src, a.dst, a.elem_bytes, a.dim, a.rule = src, dst.data_ptr(), dst.element_size(), k, \
                _abi.COLLAPSE_RULES[rule]
        r.child_out, r.node_map, r.src_node, r.into_slot = (x.data_ptr() for x in (child_out, node_map, src_node,
                                                                                    into_slot))
        r.n_keep, r.arrays, r.n_arrays = n_keep, arrays, len(arrays)
        _abi.check(L.vr_collapse_apply(C.byref(r), sp))
        _abi.check(L.vr_stream_sync(sp))   # (the upload reads the arrays on streams of its own)
        new = N3Tree.from_device_arrays(child_out, data_out, tree.offset, tree.scale, tree.data_format,
                                        extra=getattr(tree, "extra_", None),
                                        ndc=(tree.ndc_width, tree.ndc_height, tree.ndc_focal) if tree.use_ndc else None)
    return {"tree": new, "companions": outs, "node_map": node_map, "src_node": src_node, "into_slot": into_slot,
            "n_keep": n_keep}


# ---- where a slot is (vr_tree_geometry / vr_slot_points) ----
_GEOMETRY_OUT = ("parent_slot", "node_depth", "node_origin")


def _child_on_device(tree, device):
    """The tree's child array as an int32 tensor on ``device`` (the host copy ``child_``, as ``refine`` puts it
    there), complete before the caller enqueues on a stream of its own."""
    import torch
    child = torch.from_numpy(np.ascontiguousarray(tree.child_, dtype=np.int32)).to(device)
    torch.cuda.current_stream(device).synchronize()   # (torch's stream need not be the caller's)
    return child


def geometry(tree, want=_GEOMETRY_OUT, stream=None) -> dict:
    """Where the nodes of ``tree`` are -- vr_tree_geometry on its child array, enqueued on ``stream``; in the file's
    numbering, as everything indexed by slot (s = node * N^3 + (ix * N + iy) * N + iz).

    ``want``: any of "parent_slot" int32 [capacity] (the slot that links to the node; -1 for the root and for a node
    nothing links to), "node_depth" int32 [capacity] (links from the root, the ``depth`` of ``query_points`` for the
    node's leaves; -1 where the chain does not reach the root within 64 links) and "node_origin" int32 [capacity, 3]:
    the node's lower corner in the N^depth grid of its level -- the library's uint32 words modulo 2^32, as the bits
    of an int32 tensor (torch computes with those; exact while N^depth <= 2^31, ``.view(torch.uint32)`` beyond).
    Returns a dict of torch tensors on the tree's device; host-blocking (the child array goes up from the host copy
    and the call waits for ``stream``; the C call only enqueues).  A slot's cell: depth ``node_depth[s // N^3]``,
    lower corner ``(node_origin[s // N^3] * N + (ix, iy, iz)) / N^(depth + 1)`` in tree coordinates."""
    _ = tree.handle
    want = parse_want(want, _GEOMETRY_OUT, empty_ok=False)
    c = check(tree, [])
    import torch
    device = torch.device("cuda", c.device_index())
    cap = tree.capacity
    with torch.cuda.device(device):
        child = _child_on_device(tree, device)
        res = allocate(c, {"parent_slot": (I32, (cap,)), "node_depth": (I32, (cap,)), "node_origin": (I32, (cap, 3))},
                       {}, want, zeros=False)
        g = _abi.VrGeometry()
        g.child, g.capacity, g.N = child.data_ptr(), cap, tree.N
        g.parent_slot, g.node_depth, g.node_origin = (c.ptr.get(w) for w in _GEOMETRY_OUT)
        if g.parent_slot is None:   # the walk's links: from torch's cache, not from the device pool the C call would use
            links = torch.empty(cap, dtype=torch.int32, device=device)
            g.parent_slot = links.data_ptr()
        _abi.check(_abi.lib().vr_tree_geometry(C.byref(g), _stream_ptr(stream)))
        _abi.check(_abi.lib().vr_stream_sync(_stream_ptr(stream)))   # (the child copy is torch's to free)
    return {w: res[w] for w in want}


_tree_geometry = geometry   # (slot_points has a parameter of that name)


def slot_points(tree, slots, k: int = 1, mode: str = "center", seed: int = 0, space: str = "tree", geometry=None,
                stream=None) -> dict:
    """``k`` points in the cell of each slot of ``slots`` [n] (int32, on the tree's device, any order, repeats
    allowed; e.g. ``torch.nonzero(leaf & mask)``) -- vr_slot_points, one launch, enqueued on ``stream``: what svox's
    ``tree.sample(k)`` draws, for any list of slots.

    ``mode``: "center" (every point the cell's centre) or "jitter" (a hash of (slot, point, axis, ``seed``): the same
    bits whatever the list, its order or its split into calls).  ``geometry``: the dict of ``geometry()`` with
    "node_depth" and "node_origin" -- computed here when None.  ``space``: "tree" -- the library's bits, which
    ``query_points(space="tree")`` takes as they are and, for N a power of two and cells of at least 2^-24, finds the
    slot with -- or "world": ``(p - offset) / scale`` in torch, the inverse of the tree's offset + scale * x; not
    bit-pinned, and it waits for ``stream``.
    Returns {"points": float32 [n, k, 3], "depth": int32 [n], "side": float32 [n], the edge of the slot's cell in
    tree coordinates}.  A slot index out of range or of a node without a depth gives NaN points, depth -1, side NaN."""
    _ = tree.handle
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= _abi.POINTS_MAX_K:
        raise ValueError(f"k must be an integer in 1..{_abi.POINTS_MAX_K}, not {k!r}")
    if mode not in _abi.POINTS_MODES:
        raise ValueError(f"mode must be 'center' or 'jitter', not {mode!r}")
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 2 ** 32:
        raise ValueError(f"seed must be an integer in 0..2^32 - 1, not {seed!r}")
    if space not in _abi.SPACES:
        raise ValueError(f"space must be 'world' or 'tree', not {space!r}")
    cap = tree.capacity
    bufs = [Buf("slots", slots, (I32,), ("n",), rows=True)]
    if geometry is not None:
        if not isinstance(geometry, dict) or any(w not in geometry for w in ("node_depth", "node_origin")):
            raise ValueError("geometry must be a dict with 'node_depth' and 'node_origin' (what geometry() returns)")
        bufs += [Buf("geometry['node_depth']", geometry["node_depth"], (I32,), (cap,)),
                 Buf("geometry['node_origin']", geometry["node_origin"], (I32,), (cap, 3))]
    c = check(tree, bufs)
    res = allocate(c, {"points": (F32, ("n", k, 3)), "depth": (I32, ("n",)), "side": (F32, ("n",))}, {},
                   ("points", "depth", "side"), zeros=False)
    if c.n == 0:  # (empty tensors have no address to pass, and nothing would be enqueued)
        return res
    if geometry is None:
        geo = _tree_geometry(tree, ("node_depth", "node_origin"), stream=stream)
        c.ptr["geometry['node_depth']"], c.ptr["geometry['node_origin']"] = (
            int(geo[w].data_ptr()) for w in ("node_depth", "node_origin"))
    p = _abi.VrSlotPoints()
    p.node_depth, p.node_origin = c.ptr["geometry['node_depth']"], c.ptr["geometry['node_origin']"]
    p.slots, p.points, p.depth, p.side = c.ptr["slots"], c.ptr["points"], c.ptr["depth"], c.ptr["side"]
    p.capacity, p.n, p.N, p.k, p.mode, p.seed = cap, c.n, tree.N, k, _abi.POINTS_MODES[mode], seed
    L, sp = _abi.lib(), _stream_ptr(stream)
    _abi.check(L.vr_slot_points(C.byref(p), sp))
    if geometry is None or space == "world":
        _abi.check(L.vr_stream_sync(sp))   # (the arrays made here are torch's to free; torch computes on its own stream)
    if space == "world":
        import torch
        off, scale = (torch.as_tensor(np.asarray(v, np.float32), device=res["points"].device)
                      for v in (tree.offset, tree.scale))
        res["points"] = (res["points"] - off) / scale
    return res


def parent_depth(tree, stream=None):
    """The ``parent_depth`` array svox keeps and its tree files carry: int32 [capacity, 2], row m = (the slot that
    links to node m, the depth of node m); the root's row is (0, 0), as svox stores it.  From ``geometry()``; a torch
    tensor on the tree's device (``synth.save_npz(..., parent_depth=...)`` writes it)."""
    import torch
    geo = geometry(tree, ("parent_slot", "node_depth"), stream=stream)
    out = torch.stack([geo["parent_slot"], geo["node_depth"]], dim=1)
    out[0, 0] = 0
    return out


# ---- the median-cut encoder of the compressed file format (vr_quantize) ----
class _DeviceOf:
    """Stands where ``_args.check`` asks a tree for its device, for a data array that is no tree's: the device the
    array is on."""

    def __init__(self, x):
        self._x = x

    def info(self) -> dict:
        index = getattr(getattr(self._x, "device", None), "index", None)
        return {"device": 0 if index is None else int(index)}


def _quantize_args(data_dim, bits, retain, sigma_thresh) -> None:
    """What vr_quantize refuses of its scalars, as ValueErrors before any C call."""
    if not isinstance(data_dim, int) or data_dim < 4 or (data_dim - 1) % 3:
        raise ValueError(f"data_dim must be 3 * n_basis + 1 with n_basis >= 1, not {data_dim!r}")
    if not isinstance(bits, int) or isinstance(bits, bool) or not 1 <= bits <= _abi.QUANT_MAX_BITS:
        raise ValueError(f"bits must be an integer in 1..{_abi.QUANT_MAX_BITS}, not {bits!r}")
    n_basis = (data_dim - 1) // 3
    if not isinstance(retain, int) or isinstance(retain, bool) or not 0 <= retain <= n_basis - 1:
        raise ValueError(f"retain must be an integer in 0..n_basis - 1 = {n_basis - 1}, not {retain!r}")
    if isinstance(sigma_thresh, bool) or not isinstance(sigma_thresh, (int, float)) or sigma_thresh != sigma_thresh:
        raise ValueError(f"sigma_thresh must be a number and not NaN, not {sigma_thresh!r}")


def quantize(tree_or_data, *, bits: int = 16, retain: int = 1, sigma_thresh: float = 2.0, stream=None) -> dict:
    """The median-cut compression of scripts/compress_octree.py (unweighted; its defaults), on the device --
    vr_quantize, enqueued on ``stream``.  ``tree_or_data``: an uploaded tree, whose current values are read with
    ``read_data``, or a float16 tensor [..., data_dim] in the file's layout on the device.

    Slots with ``sigma > sigma_thresh`` are kept; per basis function beyond the first ``retain`` the (R, G, B) of the
    kept slots are cut ``bits`` times at the median of their widest axis and every box is replaced by its mean (the
    definition, exact to the bit, is in include/volrend_hip.h).  Returns {"quant_colors": float16 [n_quant, 65536, 3],
    "quant_map": int16 [n_quant, n_slots] (the library's uint16 codes as the bits of an int16 tensor: ``.cpu().numpy()
    .view(numpy.uint16)``), "sigma": float16 [n_slots], "data_retained": float16 [retain, n_slots, 3] or None}: the
    arrays of a VrQuantDesc, which ``N3Tree.save(quantize=...)`` writes.  Host-blocking: waits for ``stream`` (the
    workspace is torch's to free; the C call only enqueues)."""
    if hasattr(tree_or_data, "handle") or not hasattr(tree_or_data, "shape"):
        tree = tree_or_data
        _ = tree.handle
        _quantize_args(tree.data_dim, bits, retain, sigma_thresh)
        data = read_data(tree, stream=stream)
        owner, data_dim = tree, tree.data_dim
    else:
        data = tree_or_data
        shape = tuple(data.shape)
        data_dim = int(shape[-1]) if shape else 0
        _quantize_args(data_dim, bits, retain, sigma_thresh)
        owner = _DeviceOf(data)
    n_slots = 1
    for d in tuple(data.shape)[:-1]:
        n_slots *= int(d)
    if n_slots < 1 or n_slots >= 2 ** 31:
        raise ValueError(f"data must have between 1 and 2^31 - 1 slots, not {n_slots}")
    c = check(owner, [Buf("data", data, (F16,), tuple(data.shape))])
    n_quant = (data_dim - 1) // 3 - retain
    import torch
    device = torch.device("cuda", c.device_index())
    L = _abi.lib()
    need = int(L.vr_quantize_workspace(n_slots, data_dim))
    res = {"quant_colors": torch.empty((n_quant, _abi.QUANT_ROWS, 3), dtype=torch.float16, device=device),
           "quant_map": torch.empty((n_quant, n_slots), dtype=torch.int16, device=device),
           "sigma": torch.empty((n_slots,), dtype=torch.float16, device=device),
           "data_retained": torch.empty((retain, n_slots, 3), dtype=torch.float16, device=device) if retain else None}
    work = torch.empty((need + 256,), dtype=torch.uint8, device=device)
    q = _abi.VrQuantize()
    q.data = c.ptr["data"]
    q.quant_colors, q.quant_map, q.sigma = (int(res[k].data_ptr()) for k in ("quant_colors", "quant_map", "sigma"))
    q.data_retained = int(res["data_retained"].data_ptr()) if retain else None
    q.workspace = (int(work.data_ptr()) + 255) // 256 * 256
    q.workspace_bytes = need
    q.n_slots, q.data_dim, q.n_retained, q.bits, q.sigma_thresh = n_slots, data_dim, retain, bits, float(sigma_thresh)
    sp = _stream_ptr(stream)
    with torch.cuda.device(device):
        torch.cuda.current_stream(device).synchronize()   # (torch's allocations are its stream's; ours may differ)
        _abi.check(L.vr_quantize(C.byref(q), sp))
        _abi.check(L.vr_stream_sync(sp))
    return res


# ---- a sparse optimiser step, in place (vr_tree_step) ----
def tree_step(tree, master, grad, touched, *, kind="sgd", lr, lr_sigma=None, m=None, v=None, betas=(0.9, 0.999),
              eps: float = 1e-8, step: int = 1, stream=None) -> None:
    """An optimiser step over ONLY the slots marked in ``touched``, written into the DEVICE copy in place --
    vr_tree_step, enqueued on ``stream``.

    ``master`` / ``grad`` (and ``m`` / ``v`` for kind="adam"): float32 buffers of capacity * N^3 * data_dim
    elements, contiguous, on the tree's device, indexed like the file's ``data`` array; ``touched``: the int32
    bitmap a marked ``render_backward`` / ``render_backward_rays`` filled.  In every marked slot ``master``
    moves by the rule of include/volrend_hip.h (``lr_sigma``: the rate of the sigma entry, default ``lr``;
    Adam's moments of unmarked slots stand still), the tree takes float16(master), ``grad`` becomes +0; then
    the bitmap is zero.  Unmarked slots are neither read nor written.  WRITES the tree, ordered as
    ``update_data`` is; the host arrays of the tree object go stale."""
    handle = tree.handle
    if kind not in _abi.STEP_KINDS:
        raise ValueError(f"kind names 'sgd' or 'adam', not {kind!r}")
    bufs = []
    for name, x in (("master", master), ("grad", grad), ("m", m), ("v", v)):
        if x is not None:
            bufs.append(_data_buf(tree, name, x, (F32,)))
        elif name in ("master", "grad") or kind != "sgd":
            raise ValueError(f"{name} is missing" + (" (kind='adam' needs both moments)" if name in ("m", "v") else ""))
    s = _abi.VrStep()
    for name, ptr in check(tree, bufs + [_touched_buf(tree, touched)]).ptr.items():
        setattr(s, name, ptr)
    s.kind = _abi.STEP_KINDS[kind]
    s.lr, s.lr_sigma = float(lr), float(lr if lr_sigma is None else lr_sigma)
    s.beta1, s.beta2, s.eps, s.step = float(betas[0]), float(betas[1]), float(eps), int(step)
    _abi.check(_abi.lib().vr_tree_step(handle, C.byref(s), _stream_ptr(stream)))
