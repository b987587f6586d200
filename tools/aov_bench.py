#!/usr/bin/env python3
"""What depth and transmittance cost: vr_render_aov against the only way to get any depth without it.

One process, two builds of the library -- the parent commit's (``--parent-lib``) and this tree's --
loaded side by side and measured ALTERNATELY (the way tools/quick_ab.py switches variants), on the
tree of a bench.py config at its frame size, ``--frames`` poses per launch:

    (a) parent: the colour launch (vr_render_batch)
    (b) parent: the colour launch + its render_depth launch of the same poses (two marches)
    (c) new:    vr_render_aov with both planes (one march)
    (d) new:    the colour launch (the same machine code as (a): tools/kernel_digest.py)

Figures, windows and spreads are those of tools/benchlib.py: ``--window`` seconds of launches per window,
``--reps`` windows per variant, interleaved a, b, c, d, a, b, ...  Conditions (exit status 1 when one fails):
    (c) < (b) by more than the largest spread;   |(d) - (a)| <= the largest spread.
(c) / (a) gets no threshold: it is recorded.  One JSON line per run, appended to ``--out``.

    python -m volrend_amd.build                      # this tree
    (build the parent commit's library the same way) # e.g. from `git worktree add ../parent HEAD~1`
    python tools/aov_bench.py --parent-lib ../parent/volrend_amd/libvolrend_hip.so --config C1

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import os
import sys

import benchlib as bl

ROOT = bl.ROOT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "volrend_amd", "libvolrend_hip_parent.so"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of launches per timed window")
    ap.add_argument("--fp", default="strict")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from volrend_amd import _abi, api

    sc = bl.scene(args.config)
    W, H, focal, stree, transforms, stream = sc.W, sc.H, sc.focal, sc.stree, sc.transforms, sc.stream
    nf = args.frames
    fp_mode = _abi.FP_FMA if args.fp == "fma" else _abi.FP_STRICT
    cam = api.Camera(W, H, focal, focal)
    imgs = torch.zeros((nf, H, W, 4), dtype=torch.uint8, device="cuda")
    dimgs = torch.zeros((nf, H, W, 4), dtype=torch.uint8, device="cuda")   # the depth visualisation of (b)
    dp = torch.zeros((nf, H, W), dtype=torch.float32, device="cuda")
    tp = torch.zeros((nf, H, W), dtype=torch.float32, device="cuda")

    libs = {"parent": bl.load_build(_abi, args.parent_lib, without=("vr_render_aov",)),
            "new": bl.load_build(_abi, os.path.join(ROOT, "volrend_amd", "libvolrend_hip.so"))}
    n_sets = 4   # launches of a window rotate over this many pose sets (as bench.py's timed region moves on)

    def poses(k):
        return [transforms[(64 + k * (nf + 7) + i) % 200] for i in range(nf)]

    trees, batches = {}, {}
    for name, L in libs.items():
        _abi._lib = L
        trees[name] = api.N3Tree.from_synth(stree)
        trees[name].reserve(W, H, nf)
        colour = [api.PreparedBatch(trees[name], cam, poses(k), api.RenderOptions(), list(imgs), True,
                                    fp_mode=fp_mode) for k in range(n_sets)]
        if name == "parent":
            depth = [api.PreparedBatch(trees[name], cam, poses(k), api.RenderOptions(render_depth=True), list(dimgs),
                                       True, fp_mode=fp_mode) for k in range(n_sets)]
            batches["a"] = (L, [[c] for c in colour])
            batches["b"] = (L, [[c, d] for c, d in zip(colour, depth)])
        else:
            aov = [api.PreparedBatch(trees[name], cam, poses(k), api.RenderOptions(), list(imgs), True,
                                     fp_mode=fp_mode, aov=[api.AovPlanes(dp[i], tp[i]) for i in range(nf)],
                                     depth_units="world") for k in range(n_sets)]
            batches["c"] = (L, [[x] for x in aov])
            batches["d"] = (L, [[c] for c in colour])

    def window(key, n_launches):   # -> ms per launch of nf poses
        L, sets = batches[key]
        _abi._lib = L

        def launch(k):
            for pb in sets[k % n_sets]:
                pb.launch(stream)
        return bl.timed(torch, stream, n_launches, launch)

    ms, n_launch, mean, spread = bl.measure("abcd", window, warm=8, floor=4, window_s=args.window, reps=args.reps)
    status = {}
    for name, L in libs.items():
        _abi._lib = L
        status[name] = trees[name].status()
        trees[name].free_device()
    _abi._lib = None

    worst = max(spread.values())
    ok_one_march = mean["c"] < mean["b"] - worst
    ok_colour = abs(mean["d"] - mean["a"]) <= worst
    rec = {"config": args.config, "fp": args.fp, "frames_per_launch": nf, "width": W, "height": H,
           "launches_per_window": n_launch, "reps": args.reps,
           "ms_per_frame": {k: round(mean[k] / nf, 5) for k in "abcd"},
           "spread_ms_per_frame": {k: round(spread[k] / nf, 5) for k in "abcd"},
           "windows_ms_per_launch": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "aov_over_colour": round(mean["c"] / mean["a"], 4),
           "aov_over_two_launches": round(mean["c"] / mean["b"], 4),
           "aov_below_two_launches_by_more_than_spread": ok_one_march,
           "colour_launch_unchanged_within_spread": ok_colour, "status": status,
           "what": "a parent colour, b parent colour + render_depth launch, c vr_render_aov (both planes), d new colour"}
    bl.emit(rec, args.out)
    return 0 if ok_one_march and ok_colour and not any(status.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
