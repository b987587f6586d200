"""The frame path: options, camera, and the launches of whole frames over the C ABI (``launch_renderer``,
``PreparedBatch``), with the tile-shard helpers and the default tuning knobs."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import TYPE_CHECKING

import numpy as np

from . import _abi
from ._args import _ptr, _stream_ptr

if TYPE_CHECKING:
    from ._tree import N3Tree

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
