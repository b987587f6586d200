"""Host-side mirror of the reference's renderer interface, over the C ABI.

Same names, argument meaning and defaults as the reference for this path:

* ``RenderOptions``   -- ``volrend::RenderOptions`` (include/volrend/render_options.hpp:11-53)
* ``Camera``          -- ``volrend::Camera`` pose/intrinsics part (include/volrend/camera.hpp:14-70)
* ``N3Tree``          -- ``volrend::N3Tree`` (include/volrend/n3tree.hpp:24-105; loader
  semantics of src/n3tree.cpp:111-362 incl. the quantised variant)
* ``launch_renderer`` -- ``volrend::launch_renderer`` (include/volrend/cuda/renderer_kernel.hpp:9-12)

Device memory and streams are the caller's (torch tensors / ``torch.cuda`` streams
are fine: anything with ``data_ptr()`` / ``cuda_stream``); the rendering itself is
always the HIP library -- there is no eager / CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

from . import _abi

CAMERA_DEFAULT_FOCAL_LENGTH = 1111.11  # camera.hpp:12
VOLREND_GLOBAL_BASIS_MAX = 25  # render_options.hpp:6


@dataclass
class RenderOptions:
    step_size: float = 1e-4
    sigma_thresh: float = 1e-2
    stop_thresh: float = 1e-2
    background_brightness: float = 1.0
    render_bbox: tuple = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    basis_minmax: tuple = (0, VOLREND_GLOBAL_BASIS_MAX - 1)
    rot_dirs: tuple = (0.0, 0.0, 0.0)
    show_grid: bool = False
    grid_max_depth: int = 4
    render_depth: bool = False
    enable_probe: bool = False
    probe: tuple = (0.0, 0.0, 1.0)
    probe_disp_size: int = 100

    def to_c(self) -> _abi.VrRenderOptions:
        o = _abi.VrRenderOptions()
        o.step_size = self.step_size
        o.sigma_thresh = self.sigma_thresh
        o.stop_thresh = self.stop_thresh
        o.background_brightness = self.background_brightness
        for i in range(6):
            o.render_bbox[i] = self.render_bbox[i]
        o.basis_minmax[0], o.basis_minmax[1] = self.basis_minmax
        for i in range(3):
            o.rot_dirs[i] = self.rot_dirs[i]
            o.probe[i] = self.probe[i]
        o.show_grid = int(self.show_grid)
        o.grid_max_depth = self.grid_max_depth
        o.render_depth = int(self.render_depth)
        o.enable_probe = int(self.enable_probe)
        o.probe_disp_size = self.probe_disp_size
        return o


class Camera:
    """Pose + intrinsics.  ``transform`` is the 4x3 column-major camera-to-world
    (right, up, back, centre) exactly as ``CameraSpec::transform``."""

    def __init__(self, width: int = 256, height: int = 256,
                 fx: float = CAMERA_DEFAULT_FOCAL_LENGTH, fy: float = -1.0):
        self.width, self.height = int(width), int(height)
        self.fx = float(CAMERA_DEFAULT_FOCAL_LENGTH if fx < 0 else fx)
        self.fy = float(self.fx if fy < 0 else fy)
        self.transform = np.zeros(12, dtype=np.float32)
        # default pose of camera.cpp:32-36
        self.v_back = np.array([-0.7071068, 0.0, 0.7071068], dtype=np.float32)
        self.v_world_up = np.array([0.0, 0.0, 1.0], dtype=np.float32)
        self.center = np.array([-3.55, 0.0, 3.55], dtype=np.float32)
        self._update()

    def _update(self, transform_from_vecs: bool = True) -> None:
        """camera.cpp:47-58 (the K / w2c matrices serve the mesh rasteriser only)."""
        if transform_from_vecs:
            b = self.v_back / np.linalg.norm(self.v_back)
            r = np.cross(self.v_world_up, b)
            r = r / np.linalg.norm(r)
            u = np.cross(b, r)
            self.transform = np.concatenate([r, u, b, self.center]).astype(np.float32)

    def set_c2w(self, c2w) -> None:
        """4x4 / 3x4 row-major camera-to-world, as read from a pose .txt
        (main_headless.cpp:40-63)."""
        m = np.asarray(c2w, dtype=np.float32)[:3, :4]
        self.transform = np.ascontiguousarray(m.T).reshape(12)

    def to_c(self) -> _abi.VrCamera:
        c = _abi.VrCamera()
        for i in range(12):
            c.transform[i] = float(self.transform[i])
        c.width, c.height, c.fx, c.fy = self.width, self.height, self.fx, self.fy
        return c


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
    def load_device(self) -> None:
        """``N3Tree::load_cuda`` (src/cuda/n3tree.cu:9-41)."""
        L = _abi.lib()
        self.free_device()
        d = _abi.VrTreeDesc()
        L.vr_default_tree_desc(C.byref(d))
        d.child = self.child_.ctypes.data
        if self.data_ is not None:
            d.data = self.data_.ctypes.data
        elif self.quant_ is None:
            raise RuntimeError("tree has no data (clear_cpu_memory was called)")
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
        d.memory = 0
        h = C.c_void_p()
        if self.data_ is None:
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

    # ---- bulk point queries (vr_query_points / vr_query_grid) --------------
    def _query_outputs(self, want, shape, have_dirs: bool, space: str):
        """Checks ``want`` / ``space`` and allocates the outputs [*shape(, k)] on the tree's device
        -> (dict of tensors, VrQueryOut, space code).  Raises ValueError before any C call."""
        import torch
        want = (want,) if isinstance(want, str) else tuple(want)
        widths = {"sigma": 0, "depth": 0, "local": 3, "coeffs": self.data_dim - 1, "rgb": 3}
        if not want or any(w not in widths for w in want) or len(set(want)) != len(want):
            raise ValueError(f"want must name at least one of {sorted(widths)}, each once: {want!r}")
        if space not in _abi.SPACES:
            raise ValueError(f"space must be 'world' or 'tree', not {space!r}")
        if "rgb" in want and not have_dirs:
            raise ValueError("rgb needs directions")
        if "rgb" in want and self.data_format[0] in ("SG", "ASG"):
            raise ValueError("rgb of SG / ASG trees is not supported by the point queries")
        dev = torch.device("cuda", self.info()["device"])
        res, out = {}, _abi.VrQueryOut()
        for w in want:
            k = widths[w]
            res[w] = torch.empty(tuple(shape) + ((k,) if k else ()), device=dev,
                                 dtype=torch.int32 if w == "depth" else torch.float32)
            setattr(out, w, res[w].data_ptr())
        return res, out, _abi.SPACES[space]

    def _query_input(self, x, what: str, n=None):
        """A [n, 3] float32 contiguous tensor on the tree's device, or a raw pointer with ``n``
        given -> (pointer, n)."""
        if isinstance(x, int):
            if n is None:
                raise ValueError(f"{what} is a raw pointer: pass n")
            return x, int(n)
        import torch
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{what} must be a torch tensor or a raw pointer, got {type(x)}")
        if x.dtype != torch.float32:
            raise ValueError(f"{what} must be float32, not {x.dtype}")
        if x.dim() != 2 or x.shape[1] != 3 or (n is not None and x.shape[0] != n):
            raise ValueError(f"{what} must have shape [{'n' if n is None else n}, 3], not {tuple(x.shape)}")
        if not x.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        dev = self.info()["device"]
        if not x.is_cuda or x.device.index != dev:
            raise ValueError(f"{what} must be on the tree's device cuda:{dev}, not {x.device}")
        return int(x.data_ptr()), int(x.shape[0])

    def query(self, points, dirs=None, *, want=("sigma",), space: str = "world", stream=None, n=None) -> dict:
        """What the tree holds at ``points`` [n, 3] (float32, contiguous, on the tree's device; or a
        raw device pointer with ``n``) -- vr_query_points, one launch, enqueued on ``stream``.

        ``want``: any of "sigma" [n], "depth" [n] int32, "local" [n, 3], "coeffs" [n, data_dim - 1],
        "rgb" [n, 3] (needs ``dirs`` [n, 3]; evaluated at the direction AS GIVEN, not normalised;
        strict model).  ``space``: "world" (offset + scale * x is applied) or "tree".  Returns a dict
        of torch tensors on the tree's device."""
        handle = self.handle
        xyz, n = self._query_input(points, "points", n)
        if n < 0:
            raise ValueError("n is negative")
        d = None if dirs is None else self._query_input(dirs, "dirs", n)[0]
        res, out, sp = self._query_outputs(want, (n,), d is not None, space)
        if n == 0:  # (empty tensors have no address to pass)
            return res
        _abi.check(_abi.lib().vr_query_points(handle, n, xyz, d, sp, C.byref(out), _stream_ptr(stream)))
        return res

    def query_grid(self, lo, hi, res, dir=None, *, want=("sigma",), space: str = "world", stream=None) -> dict:
        """The same at the res[0] x res[1] x res[2] cell centres of the box ``lo``..``hi``, generated
        on the device (vr_query_grid): cell (i, j, k) sits at lo + (i + 0.5) * ((hi - lo) / res) per
        axis, in float32.  ``dir``: one direction for all cells (needed for "rgb").  Returns tensors
        shaped [res0, res1, res2(, k)]."""
        handle = self.handle
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
        out_t, out, sp = self._query_outputs(want, tuple(int(r) for r in res_a), dir_a is not None, space)
        c_lo, c_hi = (C.c_float * 3)(*map(float, lo_a)), (C.c_float * 3)(*map(float, hi_a))
        c_res = (C.c_int32 * 3)(*[int(r) for r in res_a])
        c_dir = None if dir_a is None else C.byref((C.c_float * 3)(*map(float, dir_a)))
        _abi.check(_abi.lib().vr_query_grid(handle, C.byref(c_lo), C.byref(c_hi), C.byref(c_res), c_dir,
                                            sp, C.byref(out), _stream_ptr(stream)))
        return out_t

    # ---- per-leaf ray weights (vr_accumulate_weights) -----------------------
    def accumulate_weights(self, cam: "Camera", transforms, options: "RenderOptions", *, max_weight=None,
                           hits=None, want=("max_weight",), fp_mode: int = _abi.FP_STRICT, stream=None) -> dict:
        """Per leaf slot, over every pixel of every pose of ``transforms`` (12 floats each, as
        ``launch_renderer_batch`` takes them): the largest compositing weight a sample in the slot received
        ("max_weight", float32) and the number of hit samples in it ("hits", a uint32 count held in an int32
        tensor) -- vr_accumulate_weights, enqueued on ``stream``, one launch per 512 poses.

        Returns a dict of torch tensors shaped [capacity, N, N, N], indexed like the file's ``child`` /
        ``data`` arrays.  ``want`` names the outputs; a tensor passed as ``max_weight`` / ``hits`` is wanted
        too and is ACCUMULATED INTO (it must be contiguous, on the tree's device, and -- max_weight -- hold
        non-negative, non-NaN floats); the others are allocated zeroed.  Any split of a pose set into calls
        gives the same bits.  Of ``options`` only step_size, sigma_thresh, stop_thresh and render_bbox are
        read.  No poses: only the tree's file-order table is put on the device (the warm-up call)."""
        return accumulate_weights(self, cam, transforms, options, max_weight=max_weight, hits=hits, want=want,
                                  fp_mode=fp_mode, stream=stream)

    # ---- gradients of a rendered batch (vr_render_backward) ----------------
    def render_backward(self, cam: "Camera", transforms, options: "RenderOptions", grad_accum, *, grad_data=None,
                        fp_mode: int = _abi.FP_STRICT, stream=None, touched=None):
        """The derivative of a rendered batch with respect to the tree's values -- vr_render_backward,
        enqueued on ``stream``, one launch per 512 poses.

        ``grad_accum``: float32 [len(transforms), height, width, 4], contiguous, on the tree's device:
        dL/d of the four numbers ``accums`` of ``launch_renderer_batch`` receive per pixel.  Returns the
        float32 tensor [capacity, N, N, N, data_dim], indexed like the file's ``data`` array, that the
        contributions were ADDED into: ``grad_data`` when given (contiguous, float32), else one allocated
        zeroed.  The sum uses float atomics: two runs may differ in the last bits.  The march is that of
        ``accumulate_weights`` (offscreen, no mesh depth); render_depth, enable_probe, rot_dirs, a narrowed
        basis_minmax and SG / ASG trees are refused.

        ``touched``: an int32 tensor of ``touched_words()`` words selects the marked call
        (vr_render_backward_touched): the bit of every slot the call adds into is ORed into it -- bit s & 31 of
        word s >> 5, s = file node * N^3 + child slot; zero it once.  The marks are bit-reproducible; ``step``
        consumes them."""
        return render_backward(self, cam, transforms, options, grad_accum, grad_data=grad_data, fp_mode=fp_mode,
                               stream=stream, touched=touched)

    # ---- ray lists (vr_render_rays / vr_accumulate_weights_rays / vr_render_backward_rays) ----
    def reserve_rays(self, n: int, n_slots: int = 2) -> None:
        """Sizes ``n_slots`` launch slots so that no later ray call of up to ``n`` rays on them allocates
        (vr_reserve_rays)."""
        _abi.check(_abi.lib().vr_reserve_rays(self.handle, int(n), int(n_slots)))

    def render_rays(self, origins, dirs, options: "RenderOptions", *, want=("accum",), rgba=None, accum=None,
                    fp_mode: int = _abi.FP_STRICT, stream=None, n=None) -> dict:
        """Colour along caller-supplied rays -- vr_render_rays, one launch, enqueued on ``stream``.

        ``origins`` / ``dirs``: float32 [n, 3], contiguous, on the tree's device, world space; a direction may have
        any finite non-zero length (or raw device pointers with ``n``).  Ray i is the ray of a pixel entered
        behind screen2worlddir's matrix product: the direction is normalised, then everything an offscreen frame
        does follows, so a list built from a camera gives that frame's bits.  ``want``: "accum" (float32 [n, 4]:
        trace_ray's output before the composite) and / or "rgba" (uint8 [n, 4]: composited over
        background_brightness); a tensor passed as ``rgba`` / ``accum`` is wanted too and is written.  Returns a
        dict of torch tensors.  64 consecutive rays share a wave; the library does not reorder them.
        render_depth and enable_probe are refused."""
        return render_rays(self, origins, dirs, options, want=want, rgba=rgba, accum=accum, fp_mode=fp_mode,
                           stream=stream, n=n)

    def accumulate_weights_rays(self, origins, dirs, options: "RenderOptions", *, max_weight=None, hits=None,
                                want=("max_weight",), fp_mode: int = _abi.FP_STRICT, stream=None, n=None) -> dict:
        """``accumulate_weights`` over the rays of a list (as ``render_rays`` takes them) --
        vr_accumulate_weights_rays, one launch.  No rays: only the file-order table is put on the device."""
        return accumulate_weights_rays(self, origins, dirs, options, max_weight=max_weight, hits=hits, want=want,
                                       fp_mode=fp_mode, stream=stream, n=n)

    def render_backward_rays(self, origins, dirs, options: "RenderOptions", grad_accum, *, grad_data=None,
                             fp_mode: int = _abi.FP_STRICT, stream=None, n=None, touched=None):
        """``render_backward`` over the rays of a list (as ``render_rays`` takes them) -- vr_render_backward_rays,
        one launch.  ``grad_accum``: float32 [n, 4], row i for ray i: dL/d of the four numbers ``render_rays``
        returns as "accum".  Returns the float32 tensor [capacity, N, N, N, data_dim] added into.  ``touched``: as
        ``render_backward`` takes it (vr_render_backward_rays_touched)."""
        return render_backward_rays(self, origins, dirs, options, grad_accum, grad_data=grad_data, fp_mode=fp_mode,
                                    stream=stream, n=n, touched=touched)

    # ---- a sparse optimiser step, in place (vr_tree_step) ----
    def touched_words(self) -> int:
        """Words of a ``touched`` bitmap of this tree: ceil(capacity * N^3 / 32)."""
        return touched_words(self)

    def step(self, master, grad, touched, *, kind="sgd", lr, lr_sigma=None, m=None, v=None, betas=(0.9, 0.999),
             eps: float = 1e-8, step: int = 1, stream=None) -> None:
        """An optimiser step over ONLY the slots marked in ``touched``, written into the DEVICE copy in place --
        vr_tree_step, enqueued on ``stream``.

        ``master`` / ``grad`` (and ``m`` / ``v`` for kind="adam"): float32 tensors of capacity * N^3 * data_dim
        elements, contiguous, on the tree's device, indexed like the file's ``data`` array; ``touched``: the int32
        bitmap a marked ``render_backward`` / ``render_backward_rays`` filled.  In every marked slot ``master``
        moves by the rule of include/volrend_hip.h (``lr_sigma``: the rate of the sigma entry, default ``lr``;
        Adam's moments of unmarked slots stand still), the tree takes float16(master), ``grad`` becomes +0; then
        the bitmap is zero.  Unmarked slots are neither read nor written.  WRITES the tree, ordered as
        ``update_data`` is; the host arrays of this object go stale."""
        tree_step(self, master, grad, touched, kind=kind, lr=lr, lr_sigma=lr_sigma, m=m, v=v, betas=betas, eps=eps,
                  step=step, stream=stream)

    # ---- the values of the device copy, in place (vr_tree_update_data / vr_tree_read_data) ----
    def update_data(self, data, stream=None) -> None:
        """Overwrites the values of the DEVICE copy with ``data`` -- vr_tree_update_data, enqueued on ``stream``:
        the step after ``render_backward`` once the optimiser has moved its master parameters.

        ``data``: a torch CUDA tensor (or any object with ``__cuda_array_interface__``) of dtype float16 or
        float32 with capacity * N^3 * data_dim elements, contiguous, on the tree's device, indexed like the
        file's ``data`` array ([capacity, N, N, N, data_dim], record [R.., G.., B.., sigma]).  float32 is rounded
        to float16 to nearest even, as ``numpy.astype(float16)`` rounds.  Afterwards the device copy is bit for
        bit what a fresh upload of this array would be; the sigma of internal slots is ignored.

        The update WRITES the tree: launches and queries enqueued later on the same stream see the new values,
        work on other streams has to be ordered with events, and nothing may read the tree while it runs.  The
        host arrays of this object are NOT touched: ``data_`` goes stale, and ``load_device()`` from it would
        undo the update (``read_data`` returns what the device holds)."""
        update_data(self, data, stream=stream)

    def read_data(self, dtype=None, out=None, stream=None):
        """The current values of the DEVICE copy in file order -- vr_tree_read_data, enqueued on ``stream``: a
        torch tensor [capacity, N, N, N, data_dim] of ``dtype`` (torch.float16, the default, or torch.float32:
        the exact widening) on the tree's device; ``out`` when given (contiguous, that many elements; its dtype
        decides).  The bits are those uploaded or last written, the sigma of internal slots +0.  Works where
        the host arrays are gone (``clear_cpu_memory``, a quantised upload, a clone)."""
        return read_data(self, dtype=dtype, out=out, stream=stream)

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


@dataclass
class TileShard:
    """Screen-tile shard of one rank (multi-GPU): tiles ``t % world == rank``."""
    tile_w: int = 0
    tile_h: int = 0
    rank: int = 0
    world: int = 1
    compact: bool = False


@dataclass
class AovPlanes:
    """The extra float planes of ONE frame of an AOV launch (``vr_render_aov``): device float32
    [H,W] tensors or raw pointers, ``None`` = not wanted (at least one of the two); ``pitch``: bytes
    per row of both, 0 = width * 4.  Always addressed in frame position, whatever the shard's layout.
    ``depth`` holds D = sum of weight * t (``depth_units="tree"``) or D * delta_scale (``"world"``),
    ``transmittance`` the light the ray left the loop with; the expected depth of what a ray hit is
    ``depth / (1 - transmittance)``."""
    depth: object = None
    transmittance: object = None
    pitch: int = 0

    def to_c(self) -> "_abi.VrAov":
        a = _abi.VrAov()
        a.depth, a.transmittance, a.pitch = _ptr(self.depth), _ptr(self.transmittance), int(self.pitch)
        return a


def _aov_c(aov) -> "_abi.VrAov":
    """AovPlanes, or a (depth, transmittance[, pitch]) tuple."""
    return (aov if isinstance(aov, AovPlanes) else AovPlanes(*aov)).to_c()


def _depth_units(depth_units) -> int:
    if isinstance(depth_units, str):
        if depth_units not in _abi.DEPTH_UNITS:
            raise ValueError(f"depth_units must be one of {sorted(_abi.DEPTH_UNITS)}, got {depth_units!r}")
        return _abi.DEPTH_UNITS[depth_units]
    return int(depth_units)


def _fill_frame(f: "_abi.VrFrame", image, depth, accum, counters, offscreen: bool, pitch: int,
                shard: TileShard | None, fp_mode: int) -> None:
    """The ``VrFrame`` of one pose, into ``f``."""
    _abi.lib().vr_default_frame(C.byref(f))
    f.rgba = _ptr(image)
    f.pitch = pitch
    f.depth = _ptr(depth)
    f.accum = _ptr(accum)
    f.offscreen = 1 if offscreen else 0
    f.fp_mode = fp_mode
    f.counters = _ptr(counters)  # device int64[7], zeroed by the caller (instrumentation)
    if shard is not None:
        f.tile_w, f.tile_h, f.rank, f.world = shard.tile_w, shard.tile_h, shard.rank, shard.world
        f.layout = _abi.LAYOUT_COMPACT if shard.compact else _abi.LAYOUT_FRAME


def _cameras_c(cam: Camera, transforms):
    """``cam`` at every pose of ``transforms`` (12 floats each) as a ``VrCamera`` array.  ``cam.transform``
    is left at the last pose."""
    cams = (_abi.VrCamera * len(transforms))()
    for i, tr in enumerate(transforms):
        cam.transform = np.asarray(tr, dtype=np.float32)
        cams[i] = cam.to_c()
    return cams


def launch_renderer(tree: N3Tree, cam: Camera, options: RenderOptions, image, depth=None,
                    stream=None, offscreen: bool = False, *, accum=None, pitch: int = 0,
                    shard: TileShard | None = None, fp_mode: int = _abi.FP_STRICT,
                    counters=None, aov=None, depth_units="tree") -> None:
    """Enqueue one frame on ``stream`` (asynchronous, like the reference).

    ``image``: device RGBA8 buffer (``torch.uint8`` [H,W,4] or a raw pointer);
    ``depth``: device R32F mesh depth or None; ``offscreen=True`` is the
    ``volrend_headless`` mode (background_brightness composite).
    ``aov``: ``AovPlanes`` (or a (depth, transmittance[, pitch]) tuple): the same launch also writes
    the depth / transmittance planes (``vr_render_aov``), ``depth_units`` "tree" or "world".
    """
    f = _abi.VrFrame()
    L = _abi.lib()
    _fill_frame(f, image, depth, accum, counters, offscreen, pitch, shard, fp_mode)
    c = cam.to_c()
    o = options.to_c()
    if aov is not None:
        a = _aov_c(aov)
        _abi.check(L.vr_render_aov(tree.handle, 1, C.byref(c), C.byref(o), C.byref(f), C.byref(a),
                                   _depth_units(depth_units), _stream_ptr(stream)))
        return
    _abi.check(L.vr_render(tree.handle, C.byref(c), C.byref(o), C.byref(f), _stream_ptr(stream)))


class PreparedBatch:
    """The marshalled arguments of one ``vr_render_batch`` call.  Building them costs ~20 us of
    Python per pose; a render loop that knows its poses up front (``volrend_headless``,
    main_headless.cpp:207-225) builds them once and each ``launch`` is a single C call, so the
    host never leaves the GPU idle between launches."""

    def __init__(self, tree: N3Tree, cam: Camera, transforms, options: RenderOptions, images,
                 offscreen: bool = True, *, accums=None, depths=None, pitch: int = 0,
                 shard: TileShard | None = None, fp_mode: int = _abi.FP_STRICT, counters=None,
                 aov=None, depth_units="tree"):
        n = len(transforms)
        if n != len(images):
            raise ValueError("one image per pose")
        if aov is not None and len(aov) != n:
            raise ValueError("one AovPlanes per pose")
        self.tree, self.n = tree, n
        self.cams = _cameras_c(cam, transforms)
        self.frames = (_abi.VrFrame * n)()
        self._keep = (images, accums, depths, counters, aov)  # the buffers must outlive the launch
        # aov: one AovPlanes per pose -> launch() is vr_render_aov instead of vr_render_batch
        self.aovs, self.depth_units = None, _depth_units(depth_units)
        if aov is not None:
            self.aovs = (_abi.VrAov * n)()
            for i in range(n):
                self.aovs[i] = _aov_c(aov[i])
        for i in range(n):
            _fill_frame(self.frames[i], images[i], depths[i] if depths else None, accums[i] if accums else None,
                        counters[i] if counters else None, offscreen, pitch, shard, fp_mode)
        self.opts = options.to_c()

    def launch(self, stream=None) -> None:
        if self.aovs is not None:
            _abi.check(_abi.lib().vr_render_aov(self.tree.handle, self.n, self.cams, C.byref(self.opts),
                                                self.frames, self.aovs, self.depth_units, _stream_ptr(stream)))
            return
        _abi.check(_abi.lib().vr_render_batch(self.tree.handle, self.n, self.cams,
                                              C.byref(self.opts), self.frames, _stream_ptr(stream)))


def launch_renderer_batch(tree: N3Tree, cam: Camera, transforms, options: RenderOptions, images,
                          stream=None, offscreen: bool = True, *, accums=None, depths=None,
                          pitch: int = 0, shard: TileShard | None = None,
                          fp_mode: int = _abi.FP_STRICT, counters=None, aov=None,
                          depth_units="tree") -> None:
    """Several poses in ONE launch: ``transforms[i]`` (12-float c2w) -> ``images[i]``.
    ``aov``: one ``AovPlanes`` per pose -- the launch also writes their planes (``vr_render_aov``).

    The pose loop of ``volrend_headless`` (main_headless.cpp:207-225) with the
    poses known up front; intrinsics / options / sharding are shared.  ``counters``:
    optional list of device int64[7] tensors (instrumented flavour)."""
    PreparedBatch(tree, cam, transforms, options, images, offscreen, accums=accums, depths=depths,
                  pitch=pitch, shard=shard, fp_mode=fp_mode, counters=counters, aov=aov,
                  depth_units=depth_units).launch(stream)


def accumulate_weights(tree, cam: Camera, transforms, options: RenderOptions, *, max_weight=None, hits=None,
                       want=("max_weight",), fp_mode: int = _abi.FP_STRICT, stream=None) -> dict:
    """``N3Tree.accumulate_weights`` (documented there).  Outputs the caller passes may also be raw device
    pointers; they are returned as passed."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in ("max_weight", "hits") for w in want) or len(set(want)) != len(want):
        raise ValueError(f"want names 'max_weight' and / or 'hits', each once: {want!r}")
    given = {"max_weight": max_weight, "hits": hits}
    res = {}
    for name in ("max_weight", "hits"):
        buf = given[name]
        if buf is None and name in want:
            import torch
            dev = torch.device("cuda", tree.info()["device"])
            buf = torch.zeros((tree.capacity, tree.N, tree.N, tree.N), device=dev,
                              dtype=torch.float32 if name == "max_weight" else torch.int32)
        elif buf is not None and not isinstance(buf, int):
            shape, dt = (tree.capacity, tree.N, tree.N, tree.N), str(buf.dtype)
            if tuple(buf.shape) != shape or not buf.is_contiguous():
                raise ValueError(f"{name} must be a contiguous tensor of shape {shape}, not {tuple(buf.shape)}")
            if dt != ("torch.float32" if name == "max_weight" else "torch.int32"):
                raise ValueError(f"{name} must be {'float32' if name == 'max_weight' else 'int32'}, not {dt}")
        if buf is not None:
            res[name] = buf
    out = _abi.VrLeafWeights()
    out.max_weight, out.hits = _ptr(res.get("max_weight")), _ptr(res.get("hits"))
    L, o = _abi.lib(), options.to_c()
    n = len(transforms)
    for first in range(0, max(n, 1), _abi.MAX_BATCH):
        m = min(_abi.MAX_BATCH, n - first)
        cams = _cameras_c(cam, [transforms[first + i] for i in range(m)]) if m else None
        _abi.check(L.vr_accumulate_weights(tree.handle, m, cams, C.byref(o), int(fp_mode), C.byref(out),
                                           _stream_ptr(stream)))
    return res


def touched_words(tree) -> int:
    """Words of a ``touched`` bitmap of this tree: ceil(capacity * N^3 / 32)."""
    return (tree.capacity * tree.N ** 3 + 31) // 32


def _touched_ptr(tree, touched) -> int:
    """Checks a ``touched`` bitmap -- an int32 tensor of ``touched_words(tree)`` elements, contiguous, CUDA (or a raw
    device pointer) -> its address.  Raises ValueError before any C call."""
    if isinstance(touched, int) and not isinstance(touched, bool):
        return touched
    if not (hasattr(touched, "is_contiguous") and hasattr(touched, "data_ptr")):
        raise ValueError(f"touched must be a torch tensor or a raw device pointer, got {type(touched)}")
    if str(touched.dtype) != "torch.int32":
        raise ValueError(f"touched must be int32 (32 slots a word), not {touched.dtype}")
    n = touched_words(tree)
    if touched.numel() != n or not touched.is_contiguous():
        raise ValueError(f"touched must be a contiguous tensor of ceil(capacity * N^3 / 32) = {n} words, "
                         f"not {tuple(touched.shape)}")
    if not touched.is_cuda:
        raise ValueError(f"touched must be on the tree's device, not {touched.device}")
    return int(touched.data_ptr())


def render_backward(tree, cam: Camera, transforms, options: RenderOptions, grad_accum, *, grad_data=None,
                    fp_mode: int = _abi.FP_STRICT, stream=None, touched=None):
    """``N3Tree.render_backward`` (documented there)."""
    n = len(transforms)
    t_ptr = None if touched is None else _touched_ptr(tree, touched)
    shape_g = (n, cam.height, cam.width, 4)
    shape_d = (tree.capacity, tree.N, tree.N, tree.N, tree.data_dim)
    for name, buf, shape in (("grad_accum", grad_accum, shape_g), ("grad_data", grad_data, shape_d)):
        if buf is None and name == "grad_data":
            continue
        if buf is None or not hasattr(buf, "is_contiguous"):
            raise ValueError(f"{name} must be a torch tensor")
        if tuple(buf.shape) != shape or not buf.is_contiguous():
            raise ValueError(f"{name} must be a contiguous tensor of shape {shape}, not {tuple(buf.shape)}")
        if str(buf.dtype) != "torch.float32":
            raise ValueError(f"{name} must be float32, not {buf.dtype}")
    if grad_data is None:
        import torch
        grad_data = torch.zeros(shape_d, dtype=torch.float32, device=torch.device("cuda", tree.info()["device"]))
    L, o = _abi.lib(), options.to_c()
    frame_bytes = cam.height * cam.width * 16
    for first in range(0, max(n, 1), _abi.MAX_BATCH):
        m = min(_abi.MAX_BATCH, n - first)
        cams = _cameras_c(cam, [transforms[first + i] for i in range(m)]) if m else None
        # (no pose: an empty tensor has no address, and nothing is read -- any non-NULL pointer stands for it)
        g_ptr = _ptr(grad_accum) + first * frame_bytes if m else (_ptr(grad_accum) or _ptr(grad_data))
        if t_ptr is None:
            _abi.check(L.vr_render_backward(tree.handle, m, cams, C.byref(o), int(fp_mode), g_ptr, _ptr(grad_data),
                                            _stream_ptr(stream)))
        else:
            _abi.check(L.vr_render_backward_touched(tree.handle, m, cams, C.byref(o), int(fp_mode), g_ptr,
                                                    _ptr(grad_data), t_ptr, _stream_ptr(stream)))
    return grad_data


def _ray_list(tree, origins, dirs, n=None):
    """Checks a ray list -> (VrRays, n, a device for outputs or None).  Tensors: float32, [n, 3], contiguous, CUDA;
    raw device pointers need ``n``.  Raises ValueError before any C call and before the tree is asked anything."""
    rays = _abi.VrRays()
    tensors = []
    for name, x in (("origins", origins), ("dirs", dirs)):
        if isinstance(x, int) and not isinstance(x, bool):
            if n is None:
                raise ValueError(f"{name} is a raw pointer: pass n")
            setattr(rays, name, x)
            continue
        if not (hasattr(x, "is_contiguous") and hasattr(x, "data_ptr")):
            raise ValueError(f"{name} must be a torch tensor or a raw device pointer, got {type(x)}")
        if str(x.dtype) != "torch.float32":
            raise ValueError(f"{name} must be float32, not {x.dtype}")
        if x.dim() != 2 or x.shape[1] != 3 or (n is not None and x.shape[0] != n):
            raise ValueError(f"{name} must have shape [{'n' if n is None else n}, 3], not {tuple(x.shape)}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        n = int(x.shape[0])
        tensors.append((name, x))
        setattr(rays, name, int(x.data_ptr()))
    dev = None
    for name, x in tensors:  # (a host tensor is refused before the tree is asked anything)
        if not x.is_cuda:
            raise ValueError(f"{name} must be on the tree's device, not {x.device}")
    for name, x in tensors:
        dev = tree.info()["device"] if dev is None else dev
        if x.device.index != dev:
            raise ValueError(f"{name} must be on the tree's device cuda:{dev}, not {x.device}")
    if tensors:
        dev = tensors[0][1].device
    if n < 0:
        raise ValueError("n is negative")
    return rays, int(n), dev


def _ray_buffer(buf, name: str, shape, dtype: str):
    """An output or gradient of a ray call: a raw pointer, or a contiguous tensor of ``shape`` and ``dtype``."""
    if isinstance(buf, int) and not isinstance(buf, bool):
        return buf
    if buf is None or not hasattr(buf, "is_contiguous"):
        raise ValueError(f"{name} must be a torch tensor")
    if tuple(buf.shape) != tuple(shape) or not buf.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor of shape {tuple(shape)}, not {tuple(buf.shape)}")
    if str(buf.dtype) != "torch." + dtype:
        raise ValueError(f"{name} must be {dtype}, not {buf.dtype}")
    return buf


def _tree_device(tree, dev):
    if dev is not None:
        return dev
    import torch
    return torch.device("cuda", tree.info()["device"])


def render_rays(tree, origins, dirs, options: RenderOptions, *, want=("accum",), rgba=None, accum=None,
                fp_mode: int = _abi.FP_STRICT, stream=None, n=None) -> dict:
    """``N3Tree.render_rays`` (documented there).  Outputs may also be raw device pointers, returned as passed."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in ("rgba", "accum") for w in want) or len(set(want)) != len(want):
        raise ValueError(f"want names 'rgba' and / or 'accum', each once: {want!r}")
    rays, n, dev = _ray_list(tree, origins, dirs, n)
    res = {}
    outs = (("rgba", rgba, "uint8"), ("accum", accum, "float32"))
    for name, buf, dt in outs:  # (what the caller passed is checked before anything is allocated)
        if buf is not None:
            res[name] = _ray_buffer(buf, name, (n, 4), dt)
    for name, buf, dt in outs:
        if buf is None and name in want:
            import torch
            res[name] = torch.empty((n, 4), dtype=getattr(torch, dt), device=_tree_device(tree, dev))
    if not res:
        raise ValueError("no output is wanted: name 'rgba' and / or 'accum'")
    if n == 0:  # (empty tensors have no address to pass, and nothing would be launched)
        return res
    out = _abi.VrRayOut()
    out.rgba, out.accum = _ptr(res.get("rgba")), _ptr(res.get("accum"))
    o = options.to_c()
    _abi.check(_abi.lib().vr_render_rays(tree.handle, n, C.byref(rays), C.byref(o), int(fp_mode), C.byref(out),
                                         _stream_ptr(stream)))
    return res


def accumulate_weights_rays(tree, origins, dirs, options: RenderOptions, *, max_weight=None, hits=None,
                            want=("max_weight",), fp_mode: int = _abi.FP_STRICT, stream=None, n=None) -> dict:
    """``N3Tree.accumulate_weights_rays`` (documented there)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in ("max_weight", "hits") for w in want) or len(set(want)) != len(want):
        raise ValueError(f"want names 'max_weight' and / or 'hits', each once: {want!r}")
    rays, n, dev = _ray_list(tree, origins, dirs, n)
    shape = (tree.capacity, tree.N, tree.N, tree.N)
    res = {}
    outs = (("max_weight", max_weight, "float32"), ("hits", hits, "int32"))
    for name, buf, dt in outs:  # (what the caller passed is checked before anything is allocated)
        if buf is not None:
            res[name] = _ray_buffer(buf, name, shape, dt)
    for name, buf, dt in outs:
        if buf is None and name in want:
            import torch
            res[name] = torch.zeros(shape, dtype=getattr(torch, dt), device=_tree_device(tree, dev))
    out = _abi.VrLeafWeights()
    out.max_weight, out.hits = _ptr(res.get("max_weight")), _ptr(res.get("hits"))
    if n == 0:  # (an empty tensor has no address, and nothing is read: any non-NULL pointer stands for it)
        rays.origins = rays.dirs = out.max_weight or out.hits
    o = options.to_c()
    _abi.check(_abi.lib().vr_accumulate_weights_rays(tree.handle, n, C.byref(rays), C.byref(o), int(fp_mode),
                                                     C.byref(out), _stream_ptr(stream)))
    return res


def render_backward_rays(tree, origins, dirs, options: RenderOptions, grad_accum, *, grad_data=None,
                         fp_mode: int = _abi.FP_STRICT, stream=None, n=None, touched=None):
    """``N3Tree.render_backward_rays`` (documented there)."""
    rays, n, dev = _ray_list(tree, origins, dirs, n)
    t_ptr = None if touched is None else _touched_ptr(tree, touched)
    grad_accum = _ray_buffer(grad_accum, "grad_accum", (n, 4), "float32")
    shape_d = (tree.capacity, tree.N, tree.N, tree.N, tree.data_dim)
    if grad_data is None:
        import torch
        grad_data = torch.zeros(shape_d, dtype=torch.float32, device=_tree_device(tree, dev))
    else:
        grad_data = _ray_buffer(grad_data, "grad_data", shape_d, "float32")
    g_ptr = _ptr(grad_accum)
    if n == 0:  # (as accumulate_weights_rays)
        rays.origins = rays.dirs = g_ptr = _ptr(grad_data)
    o = options.to_c()
    if t_ptr is None:
        _abi.check(_abi.lib().vr_render_backward_rays(tree.handle, n, C.byref(rays), C.byref(o), int(fp_mode), g_ptr,
                                                      _ptr(grad_data), _stream_ptr(stream)))
    else:
        _abi.check(_abi.lib().vr_render_backward_rays_touched(tree.handle, n, C.byref(rays), C.byref(o), int(fp_mode),
                                                              g_ptr, _ptr(grad_data), t_ptr, _stream_ptr(stream)))
    return grad_data


_DATA_DTYPES = {"float16": _abi.DATA_F16, "float32": _abi.DATA_F32}


def _data_dtype(dtype) -> int:
    """torch.float16 / torch.float32 (or their names, or a __cuda_array_interface__ typestr) -> VR_DATA_*."""
    name = {"<f2": "float16", "<f4": "float32"}.get(dtype) if isinstance(dtype, str) and dtype.startswith("<") \
        else str(dtype).replace("torch.", "")
    if name not in _DATA_DTYPES:
        raise ValueError(f"the tree's data must be float16 or float32, not {dtype}")
    return _DATA_DTYPES[name]


def _data_buffer(tree, x, what: str):
    """Checks a buffer of the tree's values: dtype, element count, contiguity, device -> (pointer, VR_DATA_*).
    Raises ValueError before any C call; a host tensor is refused before the tree is asked anything."""
    n = tree.capacity * tree.N ** 3 * tree.data_dim
    if hasattr(x, "is_contiguous") and hasattr(x, "data_ptr"):  # a torch tensor
        code = _data_dtype(x.dtype)
        if x.numel() != n:
            raise ValueError(f"{what} must have capacity * N^3 * data_dim = {n} elements, not {x.numel()}")
        if not x.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
        if not x.is_cuda:
            raise ValueError(f"{what} must be on the tree's device, not {x.device}")
        dev = tree.info()["device"]
        if x.device.index != dev:
            raise ValueError(f"{what} must be on the tree's device cuda:{dev}, not {x.device}")
        return int(x.data_ptr()), code
    cai = getattr(x, "__cuda_array_interface__", None)
    if cai is None:
        raise ValueError(f"{what} must be a torch CUDA tensor or expose __cuda_array_interface__, got {type(x)}")
    code = _data_dtype(cai["typestr"])
    count = int(np.prod(cai["shape"], dtype=np.int64))
    if count != n:
        raise ValueError(f"{what} must have capacity * N^3 * data_dim = {n} elements, not {count}")
    if cai.get("strides") is not None:
        raise ValueError(f"{what} must be contiguous")
    return int(cai["data"][0]), code


def update_data(tree, data, stream=None) -> None:
    """``N3Tree.update_data`` (documented there)."""
    ptr, code = _data_buffer(tree, data, "data")
    _abi.check(_abi.lib().vr_tree_update_data(tree.handle, ptr, code, _stream_ptr(stream)))


def read_data(tree, dtype=None, out=None, stream=None):
    """``N3Tree.read_data`` (documented there)."""
    if out is None:
        code = _data_dtype("float16" if dtype is None else dtype)
        import torch
        out = torch.empty((tree.capacity, tree.N, tree.N, tree.N, tree.data_dim),
                          dtype=torch.float32 if code == _abi.DATA_F32 else torch.float16,
                          device=torch.device("cuda", tree.info()["device"]))
    elif dtype is not None and _data_dtype(dtype) != _data_buffer(tree, out, "out")[1]:
        raise ValueError(f"out is not of dtype {dtype}")
    ptr, code = _data_buffer(tree, out, "out")
    _abi.check(_abi.lib().vr_tree_read_data(tree.handle, ptr, code, _stream_ptr(stream)))
    return out


def tree_step(tree, master, grad, touched, *, kind="sgd", lr, lr_sigma=None, m=None, v=None, betas=(0.9, 0.999),
              eps: float = 1e-8, step: int = 1, stream=None) -> None:
    """``N3Tree.step`` (documented there)."""
    if kind not in _abi.STEP_KINDS:
        raise ValueError(f"kind names 'sgd' or 'adam', not {kind!r}")
    s = _abi.VrStep()
    for name, x in (("master", master), ("grad", grad), ("m", m), ("v", v)):
        if x is None:
            if name in ("m", "v") and kind == "sgd":
                continue
            raise ValueError(f"{name} is missing" + (" (kind='adam' needs both moments)" if name in ("m", "v") else ""))
        if isinstance(x, int) and not isinstance(x, bool):   # a raw device pointer
            setattr(s, name, x)
            continue
        if hasattr(x, "is_contiguous") and str(x.dtype) != "torch.float32":
            raise ValueError(f"{name} must be float32, not {x.dtype}")
        ptr, code = _data_buffer(tree, x, name)
        if code != _abi.DATA_F32:
            raise ValueError(f"{name} must be float32")
        setattr(s, name, ptr)
    s.touched = _touched_ptr(tree, touched)
    s.kind = _abi.STEP_KINDS[kind]
    s.lr, s.lr_sigma = float(lr), float(lr if lr_sigma is None else lr_sigma)
    s.beta1, s.beta2, s.eps, s.step = float(betas[0]), float(betas[1]), float(eps), int(step)
    _abi.check(_abi.lib().vr_tree_step(tree.handle, C.byref(s), _stream_ptr(stream)))


def set_tuning(**kw) -> None:
    """DEFAULT knobs of trees uploaded from now on (vr_set_tuning), incl. the upload-time
    top_levels / brick_levels; an existing tree is changed with ``N3Tree.set_tuning``."""
    for k, v in kw.items():
        _abi.check(_abi.lib().vr_set_tuning(k.encode(), int(v)))


def compact_bytes(width: int, height: int, shard: TileShard) -> int:
    n = _abi.lib().vr_compact_bytes(width, height, shard.tile_w, shard.tile_h, shard.world)
    if n < 0:
        raise _abi.VolrendError(1, (_abi.lib().vr_last_error() or b"").decode())
    return int(n)


def assemble_tiles(frame, gathered, width: int, height: int, shard: TileShard, stream=None,
                   pitch: int = 0) -> None:
    _abi.check(_abi.lib().vr_assemble_tiles(_ptr(frame), pitch, _ptr(gathered), width, height,
                                            shard.tile_w, shard.tile_h, shard.world,
                                            _stream_ptr(stream)))


def assemble_tiles_batch(frames, gathered, n_frames: int, width: int, height: int,
                         shard: TileShard, stream=None) -> None:
    """``frames``: contiguous device [n, H, W, 4] uint8; ``gathered``: contiguous device
    [world, n_alloc, compact_bytes] (rank-major gather result, n_alloc >= n_frames).
    One launch de-interleaves all frames."""
    cb = compact_bytes(width, height, shard)
    n_alloc = int(gathered.shape[1]) if hasattr(gathered, "shape") else n_frames
    _abi.check(_abi.lib().vr_assemble_tiles_batch(
        _ptr(frames), width * height * 4, 0, _ptr(gathered), n_alloc * cb, cb, n_frames, width,
        height, shard.tile_w, shard.tile_h, shard.world, _stream_ptr(stream)))
