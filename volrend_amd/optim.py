"""Optimising a PlenOctree's values against rays with torch: the loop ``update_data`` -> ``render_rays`` ->
``render_backward_rays`` as a ``torch.autograd.Function``, and a module that owns the master parameters.

The tree on the device holds binary16 values.  ``TreeRays`` keeps a float32 master copy; every forward rounds
it into the tree (``update_data``: to nearest even) and renders with the HIP kernels.  The gradient is the
derivative with respect to THE BINARY16 VALUES THE TREE HOLDS and is handed straight through to the float32
master: the rounding is treated as the identity, as mixed-precision optimisers treat it.  A step smaller than
half a binary16 ulp of a value therefore moves the master but not yet the render.

``SparseTreeOptimizer`` is the loop whose cost follows the rays and not the size of the tree: ``render_rays`` ->
(the caller's loss) -> the marked ``render_backward_rays`` -> ``tree_step`` over the slots the rays hit, or
``fit_rays`` -> ``tree_step`` where the loss is L2 against target colours.  The tree
is always current, so nothing is rewritten whole, no dense gradient is zeroed and no dense optimiser pass runs.
"""
from __future__ import annotations

import torch

from . import _abi, api

# Whether the loops below order their batches with ``order_rays`` unless told otherwise: what tools/order_bench.py
# measured on the bench tree (README.md "Ordering ray batches").
REORDER_DEFAULT = False


def _ordered(tree, origins, dirs, options, fp_mode, stream, payload=None) -> dict:
    """The batch in the order of ``order_rays`` (the library's default key): "order", "origins", "dirs" and, with
    a ``payload`` [n, k], "payload"."""
    return api.order_rays(tree, origins, dirs, options, payload=payload, want=("order", "origins", "dirs"),
                          fp_mode=fp_mode, stream=stream)


def _caller_order(order, y):
    """A per-ray output ``y`` of a call on the ordered batch, back in the caller's order."""
    x = torch.empty_like(y)
    x[order.long()] = y
    return x


class RenderRaysFunction(torch.autograd.Function):
    """accum [n, 4] = render_rays(tree with values ``data``, origins, dirs).  Differentiable in ``data`` only (the
    rays get no gradient).  Everything is enqueued on the current stream."""

    @staticmethod
    def forward(ctx, data, tree, origins, dirs, options, fp_mode, reorder=False):
        stream = torch.cuda.current_stream(data.device)
        api.update_data(tree, data.detach(), stream=stream)
        order = None
        if reorder and origins.shape[0]:   # (march the batch in the coherent order; the caller sees its own)
            r = _ordered(tree, origins, dirs, options, fp_mode, stream)
            order, origins, dirs = r["order"], r["origins"], r["dirs"]
        accum = api.render_rays(tree, origins, dirs, options, want=("accum",), fp_mode=fp_mode, stream=stream)["accum"]
        ctx.tree, ctx.options, ctx.fp_mode, ctx.order = tree, options, fp_mode, order
        ctx.save_for_backward(origins, dirs)
        ctx.data_shape = data.shape
        return accum if order is None else _caller_order(order, accum)

    @staticmethod
    def backward(ctx, grad_accum):
        origins, dirs = ctx.saved_tensors
        stream = torch.cuda.current_stream(grad_accum.device)
        grad_accum = grad_accum.contiguous().to(torch.float32)
        if ctx.order is not None:
            grad_accum = grad_accum[ctx.order.long()]
        grad = api.render_backward_rays(ctx.tree, origins, dirs, ctx.options, grad_accum, fp_mode=ctx.fp_mode,
                                        stream=stream)
        return grad.reshape(ctx.data_shape), None, None, None, None, None, None


class TreeRays(torch.nn.Module):
    """Owns ``data``: a float32 parameter [capacity, N, N, N, data_dim] initialised from the values the device
    copy of ``tree`` holds (``read_data(float32)``).  ``forward(origins, dirs)`` writes the parameter into the
    tree and returns the accumulators [n, 4] of the rays; ``backward`` fills ``data.grad`` (see the module
    docstring for what that gradient is).  The tree's topology is fixed.  ``reorder``: march every batch in the
    order of ``order_rays``; what the caller passes and receives keeps its own order."""

    def __init__(self, tree: "api.N3Tree", options: "api.RenderOptions | None" = None,
                 fp_mode: int = _abi.FP_STRICT, reorder: bool = REORDER_DEFAULT):
        super().__init__()
        self.tree = tree
        self.options = options or api.RenderOptions()
        self.fp_mode = int(fp_mode)
        self.reorder = bool(reorder)
        self.data = torch.nn.Parameter(api.read_data(tree, dtype=torch.float32))

    def forward(self, origins, dirs):
        return RenderRaysFunction.apply(self.data, self.tree, origins, dirs, self.options, self.fp_mode, self.reorder)


class SparseTreeOptimizer:
    """SGD or Adam over only the leaf slots a batch of rays hits, with the tree on the device kept current.

    Owns ``master`` (float32, from ``read_data(float32)``), ``grad`` (float32, zero between steps), the bitmap
    ``touched`` and, for kind="adam", the moments ``m`` and ``v`` -- all in the file's indexing.  One iteration:
    ``accum = opt.render(origins, dirs)``; form dL/d accum; ``opt.backward(origins, dirs, grad_accum)``;
    ``opt.step()`` -- or, for the L2 loss against target colours, ``opt.fit(origins, dirs, target)``; ``opt.step()``,
    which is one launch where the former is two and a loss head in torch.  Several ``backward`` / ``fit`` calls
    before one ``step`` accumulate.  Everything is enqueued on the
    current stream.  The gradient is handed straight through the binary16 rounding, as ``TreeRays`` does; Adam's
    moments of slots a step does not touch stand still (sparse-Adam semantics).

    ``reorder``: ``render`` / ``backward`` / ``fit`` first put the batch into the order of ``order_rays`` (the
    targets and grad_accum travel as its payload) and hand ``accum`` / ``sq_err`` back in the caller's order.  The
    results are those of the unordered calls -- bit for bit but for the gradient's summation order."""

    def __init__(self, tree: "api.N3Tree", kind: str = "sgd", lr: float = 1e-2, lr_sigma: "float | None" = None,
                 betas=(0.9, 0.999), eps: float = 1e-8, options: "api.RenderOptions | None" = None,
                 fp_mode: int = _abi.FP_STRICT, reorder: bool = REORDER_DEFAULT):
        if kind not in _abi.STEP_KINDS:
            raise ValueError(f"kind names 'sgd' or 'adam', not {kind!r}")
        self.tree, self.kind = tree, kind
        self.lr, self.lr_sigma, self.betas, self.eps = lr, lr_sigma, tuple(betas), eps
        self.options = options or api.RenderOptions()
        self.fp_mode = int(fp_mode)
        self.reorder = bool(reorder)
        self.master = api.read_data(tree, dtype=torch.float32)
        self.grad = torch.zeros_like(self.master)
        self.touched = torch.zeros(api.touched_words(tree), dtype=torch.int32, device=self.master.device)
        self.m = torch.zeros_like(self.master) if kind == "adam" else None
        self.v = torch.zeros_like(self.master) if kind == "adam" else None
        self.steps = 0

    def _stream(self):
        return torch.cuda.current_stream(self.master.device)

    def _batch(self, origins, dirs, payload=None):
        """-> (order or None, origins, dirs, payload) as the march gets them."""
        if not self.reorder or not origins.shape[0]:
            return None, origins, dirs, payload
        r = _ordered(self.tree, origins, dirs, self.options, self.fp_mode, self._stream(), payload)
        return r["order"], r["origins"], r["dirs"], r.get("payload")

    def render(self, origins, dirs):
        """The accumulators [n, 4] of the rays, from the tree as it stands (no ``update_data``: it is current)."""
        order, origins, dirs, _ = self._batch(origins, dirs)
        accum = api.render_rays(self.tree, origins, dirs, self.options, want=("accum",), fp_mode=self.fp_mode,
                                stream=self._stream())["accum"]
        return accum if order is None else _caller_order(order, accum)

    def backward(self, origins, dirs, grad_accum) -> None:
        """Adds the rays' gradient into ``grad`` and marks the slots it lands in."""
        _, origins, dirs, grad_accum = self._batch(origins, dirs, grad_accum.contiguous().to(torch.float32))
        api.render_backward_rays(self.tree, origins, dirs, self.options, grad_accum,
                                 grad_data=self.grad, fp_mode=self.fp_mode, touched=self.touched,
                                 stream=self._stream())

    def fit(self, origins, dirs, target, grad_scale: "float | None" = None):
        """``render``, the L2 loss against ``target`` [n, 3] and ``backward`` in one launch (``fit_rays``): adds the
        gradient of grad_scale / 2 * sum r^2 into ``grad``, marks the slots and returns the squared error per ray
        [n].  ``grad_scale`` defaults to 2 / (3 n): the mean over rays and channels."""
        if grad_scale is None:
            grad_scale = 2.0 / (3 * max(int(target.shape[0]), 1))
        order, origins, dirs, target = self._batch(origins, dirs, target)
        sq_err = api.fit_rays(self.tree, origins, dirs, self.options, target, grad_scale=grad_scale,
                              grad_data=self.grad, touched=self.touched, want=("sq_err",), fp_mode=self.fp_mode,
                              stream=self._stream())["sq_err"]
        return sq_err if order is None else _caller_order(order, sq_err)

    def refine(self, sel):
        """Subdivides the selected leaves (``api.refine``) between ``step()`` and the next ``backward`` / ``fit``:
        ``self.tree`` becomes the refined tree, ``master`` grows by copies of the refined slots' values, ``m`` / ``v``
        keep the old slots and are zero in the new ones, ``grad`` and ``touched`` are zeros of the new size (after
        ``step()`` they were zero anyway).  Old slots keep their indices.  Returns ``src_slot`` (int32 [n_new]): the
        slot each new node came from.  The old tree stays valid for whoever still holds it."""
        pairs = [(self.master, "copy")] + ([(self.m, "zero"), (self.v, "zero")] if self.kind == "adam" else [])
        res = api.refine(self.tree, sel, pairs, stream=self._stream())
        self.tree = res["tree"]
        self.master = res["companions"][0]
        if self.kind == "adam":
            self.m, self.v = res["companions"][1:3]
        self.grad = torch.zeros_like(self.master)
        self.touched = torch.zeros(api.touched_words(self.tree), dtype=torch.int32, device=self.master.device)
        return res["src_slot"]

    def collapse(self, sel):
        """Merges the selected frontier nodes into their parent slots and compacts the tree (``api.collapse``; ``sel``
        is per NODE) between ``step()`` and the next ``backward`` / ``fit``: ``self.tree`` becomes the collapsed tree,
        ``master`` is gathered into the new numbering with the MEAN of a collapsed node's slots in its merged slot,
        ``m`` / ``v`` are gathered and zero in merged slots, ``grad`` and ``touched`` are zeros of the new size.  The
        new tree then takes ``update_data(master)``, so that it holds binary16(master) in every slot.  Returns
        ``node_map`` (int32 [old capacity]): the new index of an old node, -1 if it collapsed.  The old tree stays
        valid for whoever still holds it."""
        pairs = [(self.master, "mean")] + ([(self.m, "zero"), (self.v, "zero")] if self.kind == "adam" else [])
        res = api.collapse(self.tree, sel, pairs, values="mean", stream=self._stream())
        self.tree = res["tree"]
        self.master = res["companions"][0]
        if self.kind == "adam":
            self.m, self.v = res["companions"][1:3]
        self.grad = torch.zeros_like(self.master)
        self.touched = torch.zeros(api.touched_words(self.tree), dtype=torch.int32, device=self.master.device)
        api.update_data(self.tree, self.master, stream=self._stream())
        return res["node_map"]

    def step(self) -> None:
        """The optimiser step over the marked slots; afterwards ``grad`` and ``touched`` are zero again."""
        self.steps += 1
        api.tree_step(self.tree, self.master, self.grad, self.touched, kind=self.kind, lr=self.lr,
                      lr_sigma=self.lr_sigma, m=self.m, v=self.v, betas=self.betas, eps=self.eps, step=self.steps,
                      stream=self._stream())

    def save(self, path: str, quantize=None) -> None:
        """Writes ``self.tree`` as it stands on the device -- behind every step enqueued so far, which this waits
        for -- with ``N3Tree.save``: ``data`` from the device's values, or with ``quantize=dict(bits=, retain=,
        sigma_thresh=)`` the median-cut form."""
        self._stream().synchronize()
        self.tree.save(path, quantize=quantize, from_device=True)
