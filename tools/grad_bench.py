#!/usr/bin/env python3
"""What vr_render_backward costs next to the colour launch of the same poses, and the float-atomic rate it
implies.

One process, the tree of a bench.py config at its frame size, ``--frames`` poses per launch over the
200-pose orbit (a pass = the launches that cover poses 0 .. 3 * frames - 1):

    (a)  vr_render_batch colour launches
    (b)  vr_render_backward into a buffer that has already seen the whole pass (steady state)

Figures, windows and spreads are those of tools/benchlib.py (``--window``, ``--reps``), a window a whole number
of passes.  Also reported: the bytes (b) adds per second -- hit samples per frame (the hits buffer of one
vr_accumulate_weights pass) x the floats a hit adds x 4 -- next to the 1.3 TB/s at which the chip's memory
side executes float atomic adds of the right shape.  A record, not a gate: one JSON line per run, appended to
``--out``; ``--markdown`` prints the rows of the DESIGN.md table.

    python tools/grad_bench.py --config C1 --out profiles/render_backward.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import benchlib as bl

KEYS = ("a", "b")
ATOMIC_RATE_TBS = 1.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of launches per timed window")
    ap.add_argument("--fp", default="strict")
    ap.add_argument("--out", default="")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()

    import torch
    from volrend_amd import _abi, api

    sc = bl.scene(args.config)
    W, H, focal, stree, transforms, stream, sp = sc.W, sc.H, sc.focal, sc.stree, sc.transforms, sc.stream, sc.sp
    nf, n_sets = args.frames, 3
    fp_mode = _abi.FP_FMA if args.fp == "fma" else _abi.FP_STRICT
    cam = api.Camera(W, H, focal, focal)
    L = _abi.lib()

    def poses(k):
        return [transforms[(k * nf + i) % 200] for i in range(nf)]

    tree = api.N3Tree.from_synth(stree)
    tree.reserve(W, H, nf)
    imgs = torch.zeros((nf, H, W, 4), dtype=torch.uint8, device="cuda")
    colour = [api.PreparedBatch(tree, cam, poses(k), api.RenderOptions(), list(imgs), True, fp_mode=fp_mode)
              for k in range(n_sets)]
    opt = api.RenderOptions().to_c()
    cams = []
    for k in range(n_sets):
        arr = (_abi.VrCamera * nf)()
        for i, tr in enumerate(poses(k)):
            cam.transform = tr
            arr[i] = cam.to_c()
        cams.append(arr)
    gen = torch.Generator(device="cuda").manual_seed(1)
    g = torch.randn((nf, H, W, 4), dtype=torch.float32, device="cuda", generator=gen)
    grad = torch.zeros((stree.capacity, stree.N, stree.N, stree.N, stree.data_dim), dtype=torch.float32, device="cuda")

    def launch(key, k):
        if key == "a":
            colour[k % n_sets].launch(stream)
            return
        _abi.check(L.vr_render_backward(tree.handle, nf, cams[k % n_sets], C.byref(opt), fp_mode, g.data_ptr(),
                                        grad.data_ptr(), sp))

    def window(key, n_launches):   # -> ms per launch of nf poses
        return bl.timed(torch, stream, n_launches, lambda k: launch(key, k))

    # hit samples per frame: the count buffer of one leaf-weight pass over the same poses
    hits = torch.zeros((stree.capacity, stree.N, stree.N, stree.N), dtype=torch.int32, device="cuda")
    for k in range(n_sets):
        tree.accumulate_weights(cam, poses(k), api.RenderOptions(), hits=hits, want=(), fp_mode=fp_mode)
    torch.cuda.synchronize()
    hits_per_frame = int(hits.view(-1).to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) / (n_sets * nf)
    del hits
    basis = stree.basis_dim
    run = 3 * basis + 1 if basis in (4, 9, 16, 25) else 4     # floats a hit adds (vr_dev_backward.h GradTraits::kRun)

    # the warm windows are two passes: the buffer has seen the whole pass before a timed window
    ms, n_launch, mean, spread = bl.measure(KEYS, window, warm=2 * n_sets, floor=n_sets, multiple=n_sets,
                                            window_s=args.window, reps=args.reps)
    status = tree.status()
    finite = bool(torch.isfinite(grad).all())
    tree.free_device()

    per_frame = {k: mean[k] / nf for k in KEYS}
    added_tbs = hits_per_frame * run * 4 / (per_frame["b"] * 1e-3) / 1e12
    rec = {"config": args.config, "fp": args.fp, "frames_per_launch": nf, "width": W, "height": H,
           "launches_per_window": n_launch, "reps": args.reps,
           "ms_per_frame": {k: round(per_frame[k], 5) for k in KEYS},
           "spread_ms_per_frame": {k: round(spread[k] / nf, 5) for k in KEYS},
           "windows_ms_per_launch": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "hit_samples_per_frame": round(hits_per_frame), "floats_per_hit": run,
           "added_TB_per_s": round(added_tbs, 4), "atomic_rate_TB_per_s": ATOMIC_RATE_TBS,
           "backward_over_colour": round(mean["b"] / mean["a"], 3), "finite": finite, "status": status,
           "what": "a colour, b vr_render_backward into a buffer that has seen the pass"}
    bl.emit(rec, args.out)
    if args.markdown:
        names = {"a": "colour launch (`vr_render_batch`)", "b": "`vr_render_backward`, steady state"}
        print(f"| {args.config} variant | ms / frame | spread | / colour |")
        print("|---|---|---|---|")
        for k in KEYS:
            print(f"| ({k}) {names[k]} | {per_frame[k]:.4f} | {spread[k] / nf:.4f} | {mean[k] / mean['a']:.2f} |")
        print(f"(b) adds {added_tbs:.3f} TB/s of float atomics ({hits_per_frame:.3g} hit samples x {run} floats per "
              f"frame); the chip's rate is ~{ATOMIC_RATE_TBS} TB/s")
    return 0 if finite and not status else 1


if __name__ == "__main__":
    sys.exit(main())
