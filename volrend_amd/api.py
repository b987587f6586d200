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

This module only re-exports: ``_args`` checks buffer arguments, ``_frame`` renders frames, ``_ops`` holds the
operations on an uploaded tree (one function each, which ``N3Tree`` binds as methods), ``_tree`` the tree.
"""
from . import _abi  # noqa: F401
from ._args import _ptr, _stream_ptr  # noqa: F401
from ._frame import (CAMERA_DEFAULT_FOCAL_LENGTH, VOLREND_GLOBAL_BASIS_MAX, AovPlanes, Camera,  # noqa: F401
                     PreparedBatch, RenderOptions, TileShard, _aov_c, _cameras_c, _depth_units, _fill_frame,
                     assemble_tiles, assemble_tiles_batch, compact_bytes, launch_renderer, launch_renderer_batch,
                     set_tuning)
from ._ops import (_touched_ptr, accumulate_weights, accumulate_weights_rays, collapse, fit_rays, geometry, order_rays,  # noqa: F401
                   parent_depth, quantize, query_grid, query_points, read_data, refine, render_backward, render_backward_rays, render_rays, slot_points, touched_words, tree_step,
                   update_data)
from ._tree import N3Tree, _decode_arrays, _decode_quantised, _quant_arrays, parse_data_format  # noqa: F401
