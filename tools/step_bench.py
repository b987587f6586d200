#!/usr/bin/env python3
"""What one optimiser iteration on an uploaded tree costs: the sparse step (vr_tree_step) against the dense update it
replaces, the marked backward against the unmarked one, and the whole iteration on both paths.

One process, the tree of a bench.py config, a batch of ``--rays`` rays drawn at random (seeded) from the pixels of
``--frames`` bench poses, two builds of the library loaded side by side: the parent commit's (``--parent-lib``) and
this tree's.

    (a)  step_sgd / step_adam   vr_tree_step over the slots the batch marked: values kernel + lookup refresh.  The step
                                clears its bitmap, so every timed call restores it first (a 4-bytes-per-32-slots
                                copy, timed alone as ``restore`` and subtracted).
         step_empty             vr_tree_step over an all-zero bitmap: the bitmap scan + the lookup refresh.  The
                                difference to step_sgd is what walking the touched slots costs.
         update_f32             vr_tree_update_data(VR_DATA_F32) of the same tree: what the dense loop pays.
         CONDITION: step_sgd and step_adam, refresh included, are faster than update_f32.
    (b)  bwd_parent             vr_render_backward_rays of the parent's library
         bwd_new_a / bwd_new_b  the same call of this build, twice (the A/A repeat)
         bwd_marked             vr_render_backward_rays_touched of this build
         bwd_marked_alt         the marked call of another build (``--alt-lib``: the mark set by the lane that adds a
                                hit's sigma element, inside the scatter loop, instead of once per march round)
         CONDITION: |bwd_new_a - bwd_parent| <= the A/A spread (the largest of |a - b| and the window spreads of the
         three): the unmarked code is unchanged (tools/kernel_digest.py).  bwd_marked / bwd_new_a is recorded.
    (c)  iter_dense_sgd / _adam   zero the dense gradient, vr_tree_update_data(master), vr_render_rays, the loss
                                  gradient, vr_render_backward_rays, torch.optim.SGD / Adam over the whole array
         iter_sparse_sgd / _adam  vr_render_rays, the loss gradient, vr_render_backward_rays_touched, vr_tree_step
         The ratio is recorded; none is promised.
All rates are 0 in the timed loops, so that the tree, and with it the march, stays what it is from window to window;
the arithmetic and the traffic of a step do not depend on the rate.

Figures, windows and spreads are those of tools/benchlib.py (``--window``, ``--reps``).  One JSON line per run, appended to ``--out``; ``--markdown`` prints the tables.  Exit status 1 when a condition fails.

    python -m volrend_amd.build                      # this tree
    (build the parent commit's library the same way) # e.g. from `git worktree add ../parent HEAD~1`
    python tools/step_bench.py --parent-lib ../parent/volrend_amd/libvolrend_hip.so --out profiles/sparse_step.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import benchlib as bl

ROOT = bl.ROOT
NEW_SYMBOLS = ("vr_tree_step", "vr_render_backward_touched", "vr_render_backward_rays_touched")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "volrend_amd", "libvolrend_hip_parent.so"))
    ap.add_argument("--alt-lib", default="", help="a build whose marked backward is measured next to this tree's")
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=64, help="bench poses the rays are drawn from")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timed window")
    ap.add_argument("--out", default="")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from volrend_amd import _abi, api

    sc = bl.scene(args.config)
    W, H, focal, stree, stream, sp = sc.W, sc.H, sc.focal, sc.stree, sc.stream, sc.sp
    fp_mode = _abi.FP_STRICT
    f32 = torch.float32
    n = args.rays

    # the batch: pixels drawn from the frames of the bench poses
    gen = torch.Generator(device="cuda").manual_seed(1)
    m = torch.from_numpy(np.stack(sc.transforms[:args.frames]).astype(np.float32)).cuda()
    pick = torch.randint(0, args.frames * H * W, (n,), device="cuda", generator=gen)
    origins, dirs = bl.pixel_rays(torch, m, W, H, focal, pick // (H * W), pick % (H * W))
    rays = _abi.VrRays()
    rays.origins, rays.dirs = origins.data_ptr(), dirs.data_ptr()
    opt = api.RenderOptions().to_c()

    libs = {"parent": bl.load_build(_abi, args.parent_lib, without=NEW_SYMBOLS),
            "new": bl.load_build(_abi, os.path.join(ROOT, "volrend_amd", "libvolrend_hip.so"))}
    if args.alt_lib:
        libs["alt"] = bl.load_build(_abi, args.alt_lib)
    trees = {}
    for name, L in libs.items():
        _abi._lib = L
        trees[name] = api.N3Tree.from_synth(stree)
        trees[name].reserve_rays(n, 1)
    _abi._lib = libs["new"]
    tree = trees["new"]
    info = tree.info()
    n_slots = stree.capacity * stree.N ** 3

    master = tree.read_data(dtype=f32)
    before = tree.read_data()
    grad = torch.zeros_like(master)
    mom = {k: torch.zeros_like(master) for k in ("m", "v")}
    touched = torch.zeros(api.touched_words(tree), dtype=torch.int32, device="cuda")
    accum = torch.zeros((n, 4), dtype=f32, device="cuda")
    target = torch.rand((n, 4), dtype=f32, device="cuda", generator=gen)
    g_accum = torch.randn((n, 4), dtype=f32, device="cuda", generator=gen)
    out = _abi.VrRayOut()
    out.accum = accum.data_ptr()

    # the marks of the batch, kept to restore the bitmap from; and what the marked call adds is what the unmarked adds
    _abi.check(libs["new"].vr_render_backward_rays_touched(tree.handle, n, C.byref(rays), C.byref(opt), fp_mode,
                                                           g_accum.data_ptr(), grad.data_ptr(), touched.data_ptr(), sp))
    marks = touched.clone()
    grad_marked = grad.clone()
    grad.zero_()
    _abi.check(libs["new"].vr_render_backward_rays(tree.handle, n, C.byref(rays), C.byref(opt), fp_mode,
                                                   g_accum.data_ptr(), grad.data_ptr(), sp))
    torch.cuda.synchronize()
    n_marked = int(sum(bin(w & 0xFFFFFFFF).count("1") for w in marks.cpu().tolist()))
    scale = float(grad.abs().max())
    marked_vs_unmarked = float((grad - grad_marked).abs().max()) / scale     # (float atomics: last bits only)
    hit_slots = int((grad.view(n_slots, -1) != 0).any(1).sum())
    del grad_marked
    grad.zero_()

    param = torch.nn.Parameter(master)    # the dense path: torch optimisers over the whole array
    param.grad = grad
    dense = {"sgd": torch.optim.SGD([param], lr=0.0), "adam": torch.optim.Adam([param], lr=0.0)}

    def step(kind, restore=True):
        if restore:
            touched.copy_(marks, non_blocking=True)
        tree.step(master, grad, touched, kind=kind, lr=0.0, m=mom["m"], v=mom["v"], step=1, stream=stream)

    def backward(which, marked=False, bits=None):
        L, t = libs[which], trees[which]
        if marked:
            _abi.check(L.vr_render_backward_rays_touched(t.handle, n, C.byref(rays), C.byref(opt), fp_mode,
                                                         g_accum.data_ptr(), grad.data_ptr(),
                                                         (touched if bits is None else bits).data_ptr(), sp))
        else:
            _abi.check(L.vr_render_backward_rays(t.handle, n, C.byref(rays), C.byref(opt), fp_mode, g_accum.data_ptr(),
                                                 grad.data_ptr(), sp))

    def render_and_loss():
        _abi.check(libs["new"].vr_render_rays(tree.handle, n, C.byref(rays), C.byref(opt), fp_mode, C.byref(out), sp))
        torch.sub(accum, target, out=g_accum).mul_(2.0)     # d/d accum of sum((accum - target)^2)

    def iteration(path, kind):
        if path == "dense":
            grad.zero_()
            tree.update_data(master, stream=stream)
            render_and_loss()
            backward("new")
            dense[kind].step()
        else:
            render_and_loss()
            backward("new", marked=True)
            step(kind, restore=False)

    calls = {
        "restore": lambda: touched.copy_(marks, non_blocking=True),
        "step_sgd": lambda: step("sgd"), "step_adam": lambda: step("adam"),
        "step_empty": lambda: (touched.zero_(), step("sgd", restore=False)),
        "zero_bits": lambda: touched.zero_(),
        "update_f32": lambda: tree.update_data(master, stream=stream),
        "bwd_parent": lambda: backward("parent"), "bwd_new_a": lambda: backward("new"),
        "bwd_new_b": lambda: backward("new"), "bwd_marked": lambda: backward("new", marked=True),
        "iter_dense_sgd": lambda: iteration("dense", "sgd"), "iter_dense_adam": lambda: iteration("dense", "adam"),
        "iter_sparse_sgd": lambda: iteration("sparse", "sgd"), "iter_sparse_adam": lambda: iteration("sparse", "adam"),
    }
    alt_marks_equal = None
    if args.alt_lib:
        alt_bits = torch.zeros_like(marks)
        backward("alt", marked=True, bits=alt_bits)
        torch.cuda.synchronize()
        alt_marks_equal = bool(torch.equal(alt_bits, marks))
        calls["bwd_marked_alt"] = lambda: backward("alt", marked=True)
    keys = tuple(calls)

    def window(key, n_calls):   # -> ms per call
        return bl.timed(torch, stream, n_calls, lambda _: calls[key]())

    # (the warm windows also make the tables and allocate torch's optimiser state)
    ms, n_calls, mean, spread = bl.measure(keys, window, warm=4, floor=4, window_s=args.window, reps=args.reps)
    # every rate was 0: the tree holds what it held
    unchanged = bool(torch.equal(before, tree.read_data()))   # (as values: x - 0 * g may turn a -0 into +0)
    status = {}
    for name, L in libs.items():
        _abi._lib = L
        status[name] = trees[name].status()
        trees[name].free_device()
    _abi._lib = None

    step_ms = {k: mean["step_" + k] - mean["restore"] for k in ("sgd", "adam")}
    step_ms["empty"] = mean["step_empty"] - mean["zero_bits"]
    aa = max(abs(mean["bwd_new_a"] - mean["bwd_new_b"]), spread["bwd_new_a"], spread["bwd_new_b"], spread["bwd_parent"])
    ok_step = all(mean["step_" + k] < mean["update_f32"] for k in ("sgd", "adam"))   # (the restore copy included)
    ok_unmarked = abs(mean["bwd_new_a"] - mean["bwd_parent"]) <= aa
    rec = {"config": args.config, "rays": n, "frames": args.frames, "capacity": stree.capacity,
           "data_dim": stree.data_dim, "n_slots": n_slots, "slots_marked": n_marked, "slots_with_gradient": hit_slots,
           "bitmap_bytes": int(touched.numel()) * 4, "device_bytes": info["device_bytes"],
           "top_levels": info["top_levels"], "brick_levels": info["brick_levels"],
           "calls_per_window": n_calls, "reps": args.reps,
           "ms": {k: round(mean[k], 4) for k in keys}, "spread_ms": {k: round(spread[k], 4) for k in keys},
           "step_ms_without_restore": {k: round(v, 4) for k, v in step_ms.items()},
           "touched_slot_work_ms": {k: round(step_ms[k] - step_ms["empty"], 4) for k in ("sgd", "adam")},
           "update_over_step": {k: round(mean["update_f32"] / step_ms[k], 2) for k in ("sgd", "adam")},
           "aa_spread_ms": round(aa, 4), "unmarked_new_minus_parent_ms": round(mean["bwd_new_a"] - mean["bwd_parent"], 4),
           "marked_over_unmarked": round(mean["bwd_marked"] / mean["bwd_new_a"], 4),
           "marked_minus_unmarked_max_over_scale": marked_vs_unmarked,
           "alt_marked_over_unmarked": round(mean["bwd_marked_alt"] / mean["bwd_new_a"], 4) if args.alt_lib else None,
           "alt_marks_equal": alt_marks_equal,
           "dense_over_sparse": {k: round(mean["iter_dense_" + k] / mean["iter_sparse_" + k], 2) for k in ("sgd", "adam")},
           "step_faster_than_dense_update": ok_step, "unmarked_within_aa_spread_of_parent": ok_unmarked,
           "tree_unchanged": unchanged, "status": status,
           "what": "a: step_* (restore + vr_tree_step), step_empty, update_f32; b: bwd_*; c: iter_*; ms per call"}
    bl.emit(rec, args.out)
    if args.markdown:
        print(f"| {args.config}, {n} rays, {n_marked} of {n_slots} slots marked | ms | spread |")
        print("|---|---|---|")
        rows = [("`vr_tree_step`, SGD (values + refresh)", step_ms["sgd"], spread["step_sgd"]),
                ("`vr_tree_step`, Adam (values + refresh)", step_ms["adam"], spread["step_adam"]),
                ("`vr_tree_step`, empty bitmap (scan + refresh)", step_ms["empty"], spread["step_empty"]),
                ("`vr_tree_update_data`, binary32", mean["update_f32"], spread["update_f32"]),
                ("`vr_render_backward_rays`, parent", mean["bwd_parent"], spread["bwd_parent"]),
                ("`vr_render_backward_rays`, this build (A)", mean["bwd_new_a"], spread["bwd_new_a"]),
                ("`vr_render_backward_rays`, this build (B)", mean["bwd_new_b"], spread["bwd_new_b"]),
                ("`vr_render_backward_rays_touched`", mean["bwd_marked"], spread["bwd_marked"]),
                *([("`vr_render_backward_rays_touched`, mark in the scatter loop (`--alt-lib`)", mean["bwd_marked_alt"],
                    spread["bwd_marked_alt"])] if args.alt_lib else []),
                ("iteration, dense path, SGD", mean["iter_dense_sgd"], spread["iter_dense_sgd"]),
                ("iteration, sparse path, SGD", mean["iter_sparse_sgd"], spread["iter_sparse_sgd"]),
                ("iteration, dense path, Adam", mean["iter_dense_adam"], spread["iter_dense_adam"]),
                ("iteration, sparse path, Adam", mean["iter_sparse_adam"], spread["iter_sparse_adam"])]
        for what, a, b in rows:
            print(f"| {what} | {a:.4f} | {b:.4f} |")
    return 0 if ok_step and ok_unmarked and unchanged and not any(status.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
