"""Optimising a PlenOctree's values against rays with torch: the loop ``update_data`` -> ``render_rays`` ->
``render_backward_rays`` as a ``torch.autograd.Function``, and a module that owns the master parameters.

The tree on the device holds binary16 values.  ``TreeRays`` keeps a float32 master copy; every forward rounds
it into the tree (``update_data``: to nearest even) and renders with the HIP kernels.  The gradient is the
derivative with respect to THE BINARY16 VALUES THE TREE HOLDS and is handed straight through to the float32
master: the rounding is treated as the identity, as mixed-precision optimisers treat it.  A step smaller than
half a binary16 ulp of a value therefore moves the master but not yet the render.
"""
from __future__ import annotations

import torch

from . import _abi, api


class RenderRaysFunction(torch.autograd.Function):
    """accum [n, 4] = render_rays(tree with values ``data``, origins, dirs).  Differentiable in ``data`` only (the
    rays get no gradient).  Everything is enqueued on the current stream."""

    @staticmethod
    def forward(ctx, data, tree, origins, dirs, options, fp_mode):
        stream = torch.cuda.current_stream(data.device)
        api.update_data(tree, data.detach(), stream=stream)
        accum = api.render_rays(tree, origins, dirs, options, want=("accum",), fp_mode=fp_mode, stream=stream)["accum"]
        ctx.tree, ctx.options, ctx.fp_mode = tree, options, fp_mode
        ctx.save_for_backward(origins, dirs)
        ctx.data_shape = data.shape
        return accum

    @staticmethod
    def backward(ctx, grad_accum):
        origins, dirs = ctx.saved_tensors
        stream = torch.cuda.current_stream(grad_accum.device)
        grad = api.render_backward_rays(ctx.tree, origins, dirs, ctx.options,
                                        grad_accum.contiguous().to(torch.float32), fp_mode=ctx.fp_mode, stream=stream)
        return grad.reshape(ctx.data_shape), None, None, None, None, None


class TreeRays(torch.nn.Module):
    """Owns ``data``: a float32 parameter [capacity, N, N, N, data_dim] initialised from the values the device
    copy of ``tree`` holds (``read_data(float32)``).  ``forward(origins, dirs)`` writes the parameter into the
    tree and returns the accumulators [n, 4] of the rays; ``backward`` fills ``data.grad`` (see the module
    docstring for what that gradient is).  The tree's topology is fixed."""

    def __init__(self, tree: "api.N3Tree", options: "api.RenderOptions | None" = None,
                 fp_mode: int = _abi.FP_STRICT):
        super().__init__()
        self.tree = tree
        self.options = options or api.RenderOptions()
        self.fp_mode = int(fp_mode)
        self.data = torch.nn.Parameter(api.read_data(tree, dtype=torch.float32))

    def forward(self, origins, dirs):
        return RenderRaysFunction.apply(self.data, self.tree, origins, dirs, self.options, self.fp_mode)
