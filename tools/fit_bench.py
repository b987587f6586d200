#!/usr/bin/env python3
"""What vr_fit_rays saves over the sequence it fuses, on the tree of a bench.py config and a batch of ``--rays`` rays
drawn at random (seeded) from the pixels of ``--frames`` bench poses, in one process:

    (i)   unfused      vr_render_rays(accum) -> the L2 loss head in torch (composite over background_brightness,
                       residual, sq_err, grad_accum with g_3 = -bg sum g_ch) -> vr_render_backward_rays_touched
          unfused_b    the same again: the A/A pair that gives the spread
    (ii)  fused        vr_fit_rays with touched and sq_err
    each also with vr_tree_step (SGD) behind it: unfused_step, unfused_step_b, fused_step.

The rate of the step is 0, so that the tree, and with it the march, stays what it is from window to window; the
arithmetic and the traffic of a step do not depend on the rate.  No ratio is promised: (ii) is judged against (i) of
the same run with the A/A spread (the largest of |a - b| and the window spreads of a, b and the fused case) as the
margin.  Exit status 1 when (ii) is not faster than (i) beyond the spread, with or without the step.

Figures, windows and spreads are those of tools/benchlib.py (``--window``, ``--reps``).  One JSON line per case, appended to ``--out``; ``--markdown`` prints the table.

    python -m volrend_amd.build
    python tools/fit_bench.py --out profiles/fit_rays.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import benchlib as bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=64, help="bench poses the rays are drawn from")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of iterations per timed window")
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
    L = _abi.lib()

    # the batch: pixels drawn from the frames of the bench poses
    gen = torch.Generator(device="cuda").manual_seed(1)
    m = torch.from_numpy(np.stack(sc.transforms[:args.frames]).astype(np.float32)).cuda()
    pick = torch.randint(0, args.frames * H * W, (n,), device="cuda", generator=gen)
    origins, dirs = bl.pixel_rays(torch, m, W, H, focal, pick // (H * W), pick % (H * W))
    rays = _abi.VrRays()
    rays.origins, rays.dirs = origins.data_ptr(), dirs.data_ptr()
    options = api.RenderOptions()
    opt = options.to_c()
    bg = float(options.background_brightness)
    grad_scale = 2.0 / (3 * n)

    tree = api.N3Tree.from_synth(stree)
    tree.reserve_rays(n, 1)
    n_slots = stree.capacity * stree.N ** 3
    master = tree.read_data(dtype=f32)
    before = tree.read_data()
    grad = torch.zeros_like(master)
    touched = torch.zeros(api.touched_words(tree), dtype=torch.int32, device="cuda")
    accum = torch.zeros((n, 4), dtype=f32, device="cuda")
    target = torch.rand((n, 3), dtype=f32, device="cuda", generator=gen)
    g_accum = torch.zeros((n, 4), dtype=f32, device="cuda")
    sq_err = torch.zeros(n, dtype=f32, device="cuda")
    out = _abi.VrRayOut()
    out.accum = accum.data_ptr()
    fit = _abi.VrFit()
    fit.target, fit.grad_scale, fit.grad_data = target.data_ptr(), grad_scale, grad.data_ptr()
    fit.touched, fit.sq_err = touched.data_ptr(), sq_err.data_ptr()

    def head():
        """The header's loss head, operator by operator, into the preallocated sq_err / g_accum."""
        na = 1.0 - accum[:, 3]
        r = (accum[:, :3] + (bg * na)[:, None]) - target
        sq = r * r
        torch.add(sq[:, 0] + sq[:, 1], sq[:, 2], out=sq_err)
        torch.mul(r, grad_scale, out=g_accum[:, :3])
        g_accum[:, 3] = -(bg * ((g_accum[:, 0] + g_accum[:, 1]) + g_accum[:, 2]))

    def unfused():
        _abi.check(L.vr_render_rays(tree.handle, n, C.byref(rays), C.byref(opt), fp_mode, C.byref(out), sp))
        head()
        _abi.check(L.vr_render_backward_rays_touched(tree.handle, n, C.byref(rays), C.byref(opt), fp_mode,
                                                     g_accum.data_ptr(), grad.data_ptr(), touched.data_ptr(), sp))

    def fused():
        _abi.check(L.vr_fit_rays(tree.handle, n, C.byref(rays), C.byref(opt), fp_mode, C.byref(fit), sp))

    def step():
        tree.step(master, grad, touched, kind="sgd", lr=0.0, stream=stream)

    # both paths compute the same thing: sq_err bit for bit, the marks bit for bit, the gradient up to its order
    unfused()
    torch.cuda.synchronize()
    ref = dict(sq_err=sq_err.clone(), touched=touched.clone(), grad=grad.clone())
    grad.zero_()
    touched.zero_()
    fused()
    torch.cuda.synchronize()
    same_sq_err = bool(torch.equal(sq_err.view(torch.int32), ref["sq_err"].view(torch.int32)))
    same_marks = bool(torch.equal(touched, ref["touched"]))
    grad_diff = float((grad - ref["grad"]).abs().max()) / max(float(ref["grad"].abs().max()), 1e-30)
    n_marked = int(sum(bin(w & 0xFFFFFFFF).count("1") for w in touched.cpu().tolist()))
    step()
    del ref

    calls = {
        "unfused": unfused, "unfused_b": unfused, "fused": fused,
        "unfused_step": lambda: (unfused(), step()), "unfused_step_b": lambda: (unfused(), step()),
        "fused_step": lambda: (fused(), step()),
    }
    keys = tuple(calls)

    def window(key, n_calls):   # -> ms per iteration
        return bl.timed(torch, stream, n_calls, lambda _: calls[key]())

    ms, n_calls, mean, spread = bl.measure(keys, window, warm=4, floor=4, window_s=args.window, reps=args.reps)
    step()
    torch.cuda.synchronize()
    unchanged = bool(torch.equal(before, tree.read_data()))   # (as values: every rate was 0)
    status = tree.status()
    tree.free_device()

    def margin(a, b, c):
        return max(abs(mean[a] - mean[b]), spread[a], spread[b], spread[c])
    aa = {"": margin("unfused", "unfused_b", "fused"), "_step": margin("unfused_step", "unfused_step_b", "fused_step")}
    faster = {s: mean["fused" + s] < min(mean["unfused" + s], mean["unfused" + s + "_b"]) - aa[s] for s in aa}
    common = {"config": args.config, "rays": n, "frames": args.frames, "capacity": stree.capacity,
              "data_dim": stree.data_dim, "n_slots": n_slots, "slots_marked": n_marked, "reps": args.reps,
              "sq_err_bits_equal": same_sq_err, "marks_equal": same_marks, "grad_max_diff_over_scale": grad_diff,
              "tree_unchanged": unchanged, "status": status}
    lines = []
    for key in keys:
        s = "_step" if "_step" in key else ""
        rec = dict(common, case=key, ms=round(mean[key], 4), spread_ms=round(spread[key], 4),
                   calls_per_window=n_calls[key], aa_spread_ms=round(aa[s], 4))
        if key.startswith("fused"):
            rec.update(saved_ms=round(mean["unfused" + s] - mean[key], 4),
                       fused_over_unfused=round(mean[key] / mean["unfused" + s], 4),
                       faster_beyond_spread=bool(faster[s]))
        lines.append(rec)
    bl.emit(lines, args.out)
    if args.markdown:
        print(f"| {args.config}, {n} rays, {n_marked} of {n_slots} slots marked | ms | spread |")
        print("|---|---|---|")
        names = {"unfused": "`vr_render_rays` + torch head + `vr_render_backward_rays_touched` (A)",
                 "unfused_b": "the same (B)", "fused": "`vr_fit_rays`",
                 "unfused_step": "(A) + `vr_tree_step`", "unfused_step_b": "(B) + `vr_tree_step`",
                 "fused_step": "`vr_fit_rays` + `vr_tree_step`"}
        for key in keys:
            print(f"| {names[key]} | {mean[key]:.4f} | {spread[key]:.4f} |")
    ok = same_sq_err and same_marks and unchanged and status == 0
    return 0 if ok and all(faster.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
