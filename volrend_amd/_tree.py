"""``N3Tree``: the host arrays of a tree file (npz loading, the quantised decode) and the device copy behind an
opaque handle.  The operations on the device copy are the functions of ``_ops``, bound here as methods."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi, _ops
from ._args import F16, I32, Buf, _stream_ptr, check


class _CurrentDevice:
    """Stands where ``_args.check`` asks a tree for its device, for arrays that are about to become one on the
    calling thread's current device (asked of torch only then: the other checks come first and need no device)."""

    def info(self) -> dict:
        import torch
        return {"device": int(torch.cuda.current_device())}


def parse_data_format(s: str):
    """``DataFormat::parse`` (src/n3tree.cpp:55-78) -> (format name, basis_dim)."""
    idx = next((i for i, ch in enumerate(s) if not ch.isalpha()), -1)
    if idx < 0:
        return "RGBA", -1
    head = s[:idx]
    try:
        dim = int("".join(ch for ch in s[idx:] if ch.isdigit() or ch == "-") or "0")
    except ValueError:
        dim = 0
    return (head if head in ("ASG", "SG", "SH") else "RGBA"), dim


class N3Tree:
    """Read-only N^3 tree: host arrays + the device copy behind an opaque handle."""

    def __init__(self, path: str | None = None, upload: bool = True):
        self.N = 0
        self.data_dim = 0
        self.data_format = ("RGBA", -1)
        self.capacity = 0
        self.scale = np.zeros(3, np.float32)
        self.offset = np.zeros(3, np.float32)
        self.use_ndc = False
        self.ndc_width = self.ndc_height = self.ndc_focal = 0.0
        self.child_ = None
        self.data_ = None
        self.extra_ = None
        self.quant_ = None  # codebook arrays of a quantised file awaiting the device decode
        self._handle = C.c_void_p()
        self._loaded = False
        if path is not None:
            self.open(path, upload=upload)

    # ---- construction ----------------------------------------------------
    @classmethod
    def from_arrays(cls, child, data, offset, invradius3, data_format: str, extra=None,
                    ndc=None, upload: bool = True) -> "N3Tree":
        t = cls()
        t._set_arrays(child, data, offset, invradius3, data_format, extra)
        if ndc:
            t.use_ndc = True
            t.ndc_width, t.ndc_height, t.ndc_focal = map(float, ndc)
        if upload:
            t.load_device()
        return t

    @classmethod
    def from_synth(cls, tree, upload: bool = True, ndc=None) -> "N3Tree":
        return cls.from_arrays(tree.child, tree.data, tree.offset, tree.invradius3,
                               tree.data_format, tree.extra, ndc=ndc, upload=upload)

    def _set_arrays(self, child, data, offset, invradius3, data_format, extra, data_dim=None):
        child = np.ascontiguousarray(child, dtype=np.int32)
        if child.ndim != 4 or not (child.shape[1] == child.shape[2] == child.shape[3]):
            raise RuntimeError("child must be int32 [capacity, N, N, N]")
        self.N = int(child.shape[1])
        self.capacity = int(child.shape[0])
        self.child_ = child.reshape(self.capacity, self.N, self.N, self.N)
        self.quant_ = None
        if data is None:  # quantised file, decoded on the device at upload
            self.data_ = None
            self.data_dim = int(data_dim)
        else:
            data = np.asarray(data)
            if data.dtype != np.float16:
                raise RuntimeError("data must be stored in half precision")  # n3tree.cpp:344-346
            self.data_ = np.ascontiguousarray(data)
            self.data_dim = int(self.data_.shape[-1])
            if self.data_.size != self.capacity * self.N ** 3 * self.data_dim:
                raise RuntimeError("data does not have capacity * N^3 * data_dim values")
        self.data_format = parse_data_format(data_format)
        self.scale = np.asarray(invradius3, dtype=np.float32).reshape(3).copy()
        self.offset = np.asarray(offset, dtype=np.float32).reshape(3).copy()
        self.extra_ = None if extra is None else np.ascontiguousarray(extra, dtype=np.float32)

    def open(self, path: str, upload: bool = True, device_decode: bool = True) -> None:
        """``N3Tree::open`` + ``load_npz`` (src/n3tree.cpp:111-154, 228-362).
        ``upload=False`` stops before ``load_cuda`` (host-only use, e.g. format tests).
        A quantised file is decoded on the device during the upload (``data_`` stays None
        until ``decode_host()``) unless ``device_decode=False`` or ``upload=False``."""
        if not path.endswith(".npz"):
            raise ValueError("tree file must end in .npz")  # assert at n3tree.cpp:119
        if not os.path.exists(path):
            raise FileNotFoundError(f"Can't load because file does not exist: {path}")
        z = np.load(path)
        data_dim = int(z["data_dim"])
        if "data_format" in z.files:
            fmt = str(z["data_format"])
        else:  # legacy files, n3tree.cpp:240-254
            fmt = "RGBA" if data_dim == 4 else f"SH{(data_dim - 1) // 3}"
        if "invradius3" in z.files:
            scale = z["invradius3"].astype(np.float32)
        else:
            scale = np.full(3, float(z["invradius"]), dtype=np.float32)
        child = z["child"]
        extra = z["extra_data"] if "extra_data" in z.files else None
        if "quant_colors" in z.files and upload and device_decode:
            self._set_arrays(child, None, z["offset"], scale, fmt, extra, data_dim=data_dim)
            self.quant_ = _quant_arrays(z, child)
        else:
            if "quant_colors" in z.files:
                data = _decode_quantised(z, child, data_dim)
            else:
                data = z["data"]
            self._set_arrays(child, data, z["offset"], scale, fmt, extra)
            if self.data_dim != data_dim:
                raise RuntimeError("data_dim does not match the data array")
        # LLFF NDC sidecar, n3tree.cpp:121,131-148
        pb = path[:-4] + "_poses_bounds.npy"
        if os.path.exists(pb):
            arr = np.load(pb).reshape(-1)
            self.use_ndc = True
            self.ndc_height, self.ndc_width, self.ndc_focal = float(arr[4]), float(arr[9]), float(
                arr[14])
        if upload:
            self.load_device()

    # ---- device ----------------------------------------------------------
    @classmethod
    def from_device_arrays(cls, child_dev, data_dev, offset, invradius3, data_format: str, extra=None,
                           ndc=None) -> "N3Tree":
        """A tree uploaded from arrays that are ALREADY ON THE DEVICE (vr_tree_upload with memory = 1): what
        ``refine`` produces, or anything else that builds the file's layout there.  ``child_dev``: int32
        [capacity, N, N, N], ``data_dev``: float16 [capacity, N, N, N, data_dim], contiguous tensors on the calling
        thread's current device, which becomes the tree's; the work that produced them must be finished (the
        upload does not run on the caller's stream).  The library copies what it needs: both may be freed
        afterwards.  ``child_`` holds a host copy of the child array; ``data_`` stays None, the state
        ``clear_cpu_memory`` leaves (``read_data`` returns what the device holds)."""
        shape = tuple(getattr(child_dev, "shape", ()))
        if len(shape) != 4 or not (shape[1] == shape[2] == shape[3]):
            raise ValueError("child_dev must be an int32 tensor [capacity, N, N, N]")
        dshape = tuple(getattr(data_dev, "shape", ()))
        if len(dshape) != 5 or dshape[:4] != shape or dshape[4] < 1:
            raise ValueError(f"data_dev must be a float16 tensor [capacity, N, N, N, data_dim] over {shape}, not {dshape}")
        c = check(_CurrentDevice(), [Buf("child_dev", child_dev, (I32,), shape), Buf("data_dev", data_dev, (F16,), dshape)])
        t = cls()
        t.capacity, t.N, t.data_dim = int(shape[0]), int(shape[1]), int(dshape[4])
        t.child_ = child_dev.cpu().numpy().reshape(shape)
        # (a tree's own (format name, basis_dim) pair is taken as it is: refine hands the old tree's on)
        t.data_format = parse_data_format(data_format) if isinstance(data_format, str) else tuple(data_format)
        t.scale = np.asarray(invradius3, dtype=np.float32).reshape(3).copy()
        t.offset = np.asarray(offset, dtype=np.float32).reshape(3).copy()
        t.extra_ = None if extra is None else np.ascontiguousarray(extra, dtype=np.float32)
        if ndc:
            t.use_ndc = True
            t.ndc_width, t.ndc_height, t.ndc_focal = map(float, ndc)
        t._upload(c.ptr["child_dev"], c.ptr["data_dev"], memory=1)
        return t

    def load_device(self) -> None:
        """``N3Tree::load_cuda`` (src/cuda/n3tree.cu:9-41)."""
        self.free_device()
        if self.data_ is None and self.quant_ is None:
            raise RuntimeError("tree has no data (clear_cpu_memory was called)")
        self._upload(self.child_.ctypes.data, None if self.data_ is None else self.data_.ctypes.data, memory=0)

    def _upload(self, child_ptr, data_ptr, memory: int) -> None:
        """vr_tree_upload (or its quantised form when there is no data array) of arrays in host (``memory`` 0) or
        device (1) memory."""
        L = _abi.lib()
        self.free_device()
        d = _abi.VrTreeDesc()
        L.vr_default_tree_desc(C.byref(d))
        d.child = child_ptr
        if data_ptr is not None:
            d.data = data_ptr
        if self.extra_ is not None:
            d.extra = self.extra_.ctypes.data
            d.extra_count = self.extra_.size
        for i in range(3):
            d.offset[i] = float(self.offset[i])
            d.scale[i] = float(self.scale[i])
        d.N = self.N
        d.capacity = self.capacity
        d.data_dim = self.data_dim
        d.format = _abi.FORMATS[self.data_format[0]]
        d.basis_dim = self.data_format[1]
        d.ndc_width = self.ndc_width if self.use_ndc else -1.0
        d.ndc_height = self.ndc_height
        d.ndc_focal = self.ndc_focal
        d.memory = memory
        h = C.c_void_p()
        if data_ptr is None:
            _abi.check(L.vr_tree_upload_quantized(C.byref(d), C.byref(self._quant_desc()),
                                                  C.byref(h)))
        else:
            _abi.check(L.vr_tree_upload(C.byref(d), C.byref(h)))
        self._handle = h
        self._loaded = True

    def _quant_desc(self) -> "_abi.VrQuantDesc":
        q = _abi.VrQuantDesc()
        a = self.quant_
        q.n_quant = a["quant_map"].shape[0]
        q.quant_colors = a["quant_colors"].ctypes.data
        q.quant_map = a["quant_map"].ctypes.data
        q.sigma = a["sigma"].ctypes.data
        if a["data_retained"] is not None:
            q.n_retained = a["data_retained"].shape[0]
            q.data_retained = a["data_retained"].ctypes.data
        return q

    def decode_host(self, on_device: bool = False) -> np.ndarray:
        """Materialises ``data_`` of a quantised tree: numpy restatement of the reference loop
        (src/n3tree.cpp:310-339), or the library's device decode copied back."""
        if self.data_ is None and self.quant_ is not None:
            shape = (self.capacity, self.N, self.N, self.N, self.data_dim)
            if on_device:
                d = _abi.VrTreeDesc()
                _abi.lib().vr_default_tree_desc(C.byref(d))
                d.N, d.capacity, d.data_dim, d.memory = self.N, self.capacity, self.data_dim, 0
                out = np.empty(shape, np.float16)
                _abi.check(_abi.lib().vr_decode_quantized(C.byref(d), C.byref(self._quant_desc()),
                                                          out.ctypes.data))
                self.data_ = out
            else:
                a = self.quant_
                self.data_ = _decode_arrays(a["quant_colors"], a["quant_map"], a["sigma"],
                                            a["data_retained"], self.data_dim).reshape(shape)
        return self.data_

    def clone_to(self, device: int) -> "N3Tree":
        """A replica of the DEVICE copy on another (or the same) device of this process
        (vr_tree_clone: device-to-device, no second upload / re-layout).  The replica shares the
        host-side metadata and owns its device copy."""
        t = N3Tree()
        for k in ("N", "data_dim", "data_format", "capacity", "scale", "offset", "use_ndc",
                  "ndc_width", "ndc_height", "ndc_focal", "child_"):
            setattr(t, k, getattr(self, k))
        h = C.c_void_p()
        _abi.check(_abi.lib().vr_tree_clone(self.handle, int(device), C.byref(h)))
        t._handle = h
        t._loaded = True
        return t

    def free_device(self) -> None:
        if self._handle:
            _abi.lib().vr_tree_free(self._handle)
            self._handle = C.c_void_p()
        self._loaded = False

    def is_device_loaded(self) -> bool:  # is_cuda_loaded
        return self._loaded

    def clear_cpu_memory(self) -> None:
        """n3tree.cpp:441-447: keeps ``child_`` (wireframes), drops ``data_``."""
        self.data_ = None
        self.quant_ = None

    def sched_stats(self, reset: bool = True) -> dict:
        """Scheduling tallies of instrumented launches (see vr_sched_stats)."""
        out = (C.c_uint64 * 8)()
        _abi.check(_abi.lib().vr_sched_stats(self._handle, C.byref(out), 1 if reset else 0))
        names = ("march_rounds", "march_lanes", "shade_rounds", "shade_lanes", "distinct_leaves",
                 "retire_rounds", "retired", "iterations")
        return dict(zip(names, [int(v) for v in out]))

    def cull_stats(self, reset: bool = True) -> dict:
        """8x8 pixel blocks that launches with the block cull on have seen, and those among them that ray
        generation skipped (vr_tree_cull_stats)."""
        out = (C.c_uint64 * 2)()
        _abi.check(_abi.lib().vr_tree_cull_stats(self.handle, C.byref(out), 1 if reset else 0))
        return {"blocks": int(out[0]), "culled": int(out[1])}

    def head_stats(self, reset: bool = False) -> dict:
        """Rays that entered the lead-in march of ray generation, those that ended there without a hit sample, and
        the samples marched there (vr_tree_head_stats)."""
        out = (C.c_uint64 * 3)()
        _abi.check(_abi.lib().vr_tree_head_stats(self.handle, C.byref(out), 1 if reset else 0))
        return {"entered": int(out[0]), "retired": int(out[1]), "samples": int(out[2])}

    def touch_enable(self, enable: bool = True) -> None:
        """Distinct-line meter of instrumented launches on / off (vr_touch_enable)."""
        _abi.check(_abi.lib().vr_touch_enable(self.handle, 1 if enable else 0))

    def touch_count(self, reset: bool = True) -> dict:
        """Distinct 128-byte lines touched since the last reset (vr_touch_count), per array."""
        out = (C.c_uint64 * 4)()
        _abi.check(_abi.lib().vr_touch_count(self.handle, C.byref(out), 1 if reset else 0))
        return dict(zip(("leaves", "nodes", "top", "bricks"), [int(v) for v in out]))

    def touch_read(self, which: int):
        """The distinct-line bitmap of array ``which`` (0 records, 1 child words, 2 top grid,
        3 bricks) as (uint32 numpy array, bytes per bit) -- vr_touch_read."""
        words, gran = C.c_uint64(0), C.c_uint64(0)
        _abi.check(_abi.lib().vr_touch_read(self.handle, int(which), None, 0, C.byref(words), C.byref(gran)))
        out = np.zeros(int(words.value), dtype=np.uint32)
        if out.size:
            _abi.check(_abi.lib().vr_touch_read(self.handle, int(which), out.ctypes.data, out.size, None, None))
        return out, int(gran.value)

    def reserve(self, width: int, height: int, n_frames: int, shard: "TileShard | None" = None,
                n_slots: int = 2) -> None:
        """Pre-allocate the per-launch ray buffers (vr_reserve / vr_reserve_tiles): no later
        launch of that size blocks or allocates."""
        if shard is None and n_slots == 2:
            _abi.check(_abi.lib().vr_reserve(self.handle, int(width), int(height), int(n_frames)))
        else:
            tw, th, world = (shard.tile_w, shard.tile_h, shard.world) if shard else (0, 0, 1)
            _abi.check(_abi.lib().vr_reserve_tiles(self.handle, int(width), int(height),
                                                   int(n_frames), tw, th, world, int(n_slots)))

    def set_tuning(self, **kw) -> None:
        """Scheduling knobs of THIS tree (vr_tree_set_tuning): march_max, refill_min,
        waves_per_cu, records_nt, ...  Results never depend on them."""
        for k, v in kw.items():
            _abi.check(_abi.lib().vr_tree_set_tuning(self.handle, k.encode(), int(v)))

    def status(self, reset: bool = False, stream=None) -> int:
        """Sticky device status word (vr_tree_status): bit 0 = a ray hit the sample guard.
        With ``stream``: read ON that stream and wait for it alone (vr_tree_status_on) -- other
        streams that render this tree are not waited for."""
        out = C.c_uint32(0)
        if stream is not None:
            _abi.check(_abi.lib().vr_tree_status_on(self.handle, C.byref(out), 1 if reset else 0,
                                                    _stream_ptr(stream)))
        else:
            _abi.check(_abi.lib().vr_tree_status(self.handle, C.byref(out), 1 if reset else 0))
        return int(out.value)

    def reserve_rays(self, n: int, n_slots: int = 2) -> None:
        """Sizes ``n_slots`` launch slots so that no later ray call of up to ``n`` rays on them allocates
        (vr_reserve_rays)."""
        _abi.check(_abi.lib().vr_reserve_rays(self.handle, int(n), int(n_slots)))

    # ---- the operations on the device copy: one function each, in _ops, bound as methods ----
    query, query_grid = _ops.query_points, _ops.query_grid
    accumulate_weights, render_backward = _ops.accumulate_weights, _ops.render_backward
    render_rays, accumulate_weights_rays = _ops.render_rays, _ops.accumulate_weights_rays
    render_backward_rays, touched_words = _ops.render_backward_rays, _ops.touched_words
    fit_rays, order_rays = _ops.fit_rays, _ops.order_rays
    step, update_data, read_data = _ops.tree_step, _ops.update_data, _ops.read_data
    refine, collapse = _ops.refine, _ops.collapse
    geometry, slot_points, parent_depth = _ops.geometry, _ops.slot_points, _ops.parent_depth
    quantize = _ops.quantize

    def save(self, path: str, quantize=None, *, from_device: bool = False) -> None:
        """Writes the tree as a ``tree.npz`` that ``open`` and the reference's ``load_npz`` read: ``child``,
        ``offset``, ``invradius3``, ``data_dim``, ``data_format``, ``extra_data`` when the tree has one and svox's
        ``parent_depth``; deflated (``numpy.savez_compressed``).

        ``quantize=None`` writes ``data``: the host array, or -- where ``data_`` is None (a device-built tree,
        ``clear_cpu_memory``, a quantised upload) or ``from_device`` is set (the host array is stale after
        ``step`` / ``update_data``) -- the device's values through ``read_data``.
        ``quantize=dict(bits=, retain=, sigma_thresh=)`` (any subset; the defaults of ``quantize()``) writes the
        median-cut form of scripts/compress_octree.py instead, computed on the device from the uploaded tree:
        ``quant_colors`` [n_quant, 65536, 3], ``quant_map`` [n_quant, capacity, N, N, N], ``sigma`` [capacity, N, N, N]
        and, with ``retain`` > 0, ``data_retained`` [retain, capacity, N, N, N, 3].  Host-blocking.  The NDC sidecar
        (``*_poses_bounds.npy``) is not written."""
        if not path.endswith(".npz"):
            raise ValueError("tree file must end in .npz")
        if quantize is not None:
            if not isinstance(quantize, dict) or any(k not in ("bits", "retain", "sigma_thresh") for k in quantize):
                raise ValueError("quantize must be None or a dict with any of 'bits', 'retain', 'sigma_thresh'")
        if self.child_ is None:
            raise RuntimeError("tree has no child array")
        name, dim = self.data_format
        fmt = "RGBA" if name == "RGBA" else f"{name}{dim}"
        shape = (self.capacity, self.N, self.N, self.N)
        arrays = dict(data_dim=np.int64(self.data_dim), data_format=np.array(fmt),
                      child=np.ascontiguousarray(self.child_, dtype=np.int32),
                      invradius3=np.asarray(self.scale, np.float32), offset=np.asarray(self.offset, np.float32))
        if self.extra_ is not None:
            arrays["extra_data"] = np.asarray(self.extra_, np.float32)
        if quantize is not None:
            q = _ops.quantize(self, **quantize)
            n_quant = q["quant_map"].shape[0]
            arrays["quant_colors"] = q["quant_colors"].cpu().numpy()
            arrays["quant_map"] = q["quant_map"].cpu().numpy().view(np.uint16).reshape((n_quant,) + shape)
            arrays["sigma"] = q["sigma"].cpu().numpy().reshape(shape)
            if q["data_retained"] is not None:
                r = q["data_retained"].cpu().numpy()
                arrays["data_retained"] = r.reshape((r.shape[0],) + shape + (3,))
        elif self.data_ is not None and not from_device:
            arrays["data"] = np.ascontiguousarray(self.data_, np.float16).reshape(shape + (self.data_dim,))
        elif self._loaded:
            arrays["data"] = _ops.read_data(self).cpu().numpy()
        else:
            raise RuntimeError("tree has no data (clear_cpu_memory was called) and is not on the device")
        arrays["parent_depth"] = (self.parent_depth().cpu().numpy() if self._loaded else _parent_depth_host(self.child_))
        np.savez_compressed(path, **arrays)

    def info(self) -> dict:
        i = _abi.VrTreeInfo()
        _abi.check(_abi.lib().vr_tree_info(self._handle, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in i._fields_}

    @property
    def handle(self):
        if not self._loaded:
            raise RuntimeError("tree is not on the device (call load_device)")
        return self._handle

    def __del__(self):
        try:
            self.free_device()
        except Exception:
            pass


def _parent_depth_host(child) -> np.ndarray:
    """svox's ``parent_depth`` [capacity, 2] from a host child array, for a tree that is not on the device: row m =
    (the slot that links to node m, the depth of node m), the root's row (0, 0).  The rule of vr_tree_geometry
    (include/volrend_hip.h), so that ``save`` writes the same array for a tree on and off the device: the slot is
    the one whose link, inside [1, capacity), points at m, whether or not the root reaches that slot's node, and -1
    where there is none; the depth is the number of links up that chain to node 0, and -1 where the chain does not
    get there within 64 links."""
    cap = child.shape[0]
    flat = np.ascontiguousarray(child, np.int32).reshape(-1).astype(np.int64)
    N3 = flat.size // cap
    s = np.flatnonzero(flat)
    m = s // N3 + flat[s]
    ok = (m >= 1) & (m < cap)
    parent = np.full(cap, -1, np.int64)
    parent[m[ok]] = s[ok]
    cur = np.arange(cap)
    depth = np.zeros(cap, np.int64)
    for _ in range(64):
        step = (cur != 0) & (parent[cur] >= 0)
        if not step.any():
            break
        cur = np.where(step, parent[cur] // N3, cur)
        depth += step
    depth[cur != 0] = -1
    out = np.stack([parent, depth], axis=1).astype(np.int32)
    out[0] = 0
    return out


def _quant_arrays(z, child) -> dict:
    """The codebook members of a quantised tree.npz (scripts/compress_octree.py:106-119),
    checked as src/n3tree.cpp:279-293 does and flattened to [.., n_slots, ..]."""
    qc = z["quant_colors"]
    if qc.dtype != np.float16:
        raise RuntimeError("codebook must be stored in half precision")
    qm = z["quant_map"]
    n_q = qm.shape[0]
    if qc.shape[0] != n_q:
        raise RuntimeError("codebook and map basis numbers does not match")
    cap, N = qm.shape[1], child.shape[1]
    if cap != child.shape[0] or qc.shape[1:] != (65536, 3):
        raise RuntimeError("quantised arrays do not match the tree")
    n_slots = cap * N * N * N
    retained = z["data_retained"] if "data_retained" in z.files else None
    return dict(
        quant_colors=np.ascontiguousarray(qc),
        quant_map=np.ascontiguousarray(qm.reshape(n_q, n_slots), dtype=np.uint16),
        sigma=np.ascontiguousarray(z["sigma"].reshape(n_slots), dtype=np.float16),
        data_retained=None if retained is None else np.ascontiguousarray(
            retained.reshape(retained.shape[0], n_slots, 3), dtype=np.float16))


def _decode_arrays(qc, qm, sigma, retained, data_dim: int) -> np.ndarray:
    """Median-cut codebook decode, src/n3tree.cpp:279-340.

    data[slot, j + n_retain + c*n_basis] = quant_colors[j, quant_map[j, slot], c]
    data[slot, j + c*n_basis]            = data_retained[j, slot, c]
    data[slot, data_dim-1]               = sigma[slot]
    """
    n_q, n_slots = qm.shape
    n_ret = 0 if retained is None else retained.shape[0]
    n_basis = n_q + n_ret
    data = np.zeros((n_slots, data_dim), dtype=np.float16)
    for j in range(n_q):
        cols = qc[j][qm[j].astype(np.int64)]  # [n_slots, 3]
        for c in range(3):
            data[:, j + n_ret + c * n_basis] = cols[:, c]
    data[:, data_dim - 1] = sigma
    for j in range(n_ret):
        for c in range(3):
            data[:, j + c * n_basis] = retained[j, :, c]
    return data


def _decode_quantised(z, child, data_dim: int) -> np.ndarray:
    a = _quant_arrays(z, child)
    cap, N = child.shape[0], child.shape[1]
    return _decode_arrays(a["quant_colors"], a["quant_map"], a["sigma"], a["data_retained"],
                          data_dim).reshape(cap, N, N, N, data_dim)
