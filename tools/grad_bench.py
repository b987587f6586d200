#!/usr/bin/env python3
"""What vr_render_backward costs next to the colour launch of the same poses, and the float-atomic rate it
implies.

One process, the tree of a bench.py config at its frame size, ``--frames`` poses per launch over the
200-pose orbit (a pass = the launches that cover poses 0 .. 3 * frames - 1):

    (a)  vr_render_batch colour launches
    (b)  vr_render_backward into a buffer that has already seen the whole pass (steady state)

Each figure is the mean over one warmed window of >= ``--window`` seconds of back-to-back launches between
two HIP events; ``--reps`` windows per variant, interleaved; the spread of a variant is max - min over its
windows.  Also reported: the bytes (b) adds per second -- hit samples per frame (the hits buffer of one
vr_accumulate_weights pass) x the floats a hit adds x 4 -- next to the 1.3 TB/s at which the chip's memory
side executes float atomic adds of the right shape.  A record, not a gate: one JSON line per run, appended to
``--out``; ``--markdown`` prints the rows of the DESIGN.md table.

    python tools/grad_bench.py --config C1 --out profiles/render_backward.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    from volrend_amd import _abi, api, synth
    import bench as B

    cfg = synth.CONFIGS[args.config]
    W, H, focal = cfg["width"], cfg["height"], cfg["focal"]
    stree = B.load_or_make_tree(synth, args.config, 0, lambda: None)
    transforms = [synth.c2w_to_transform(p) for p in synth.make_poses(200)]
    nf, n_sets = args.frames, 3
    stream = torch.cuda.current_stream()
    sp = api._stream_ptr(stream)
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

    def window(key, n_launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(n_launches):
            launch(key, k)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n_launches   # ms per launch of nf poses

    # hit samples per frame: the count buffer of one leaf-weight pass over the same poses
    hits = torch.zeros((stree.capacity, stree.N, stree.N, stree.N), dtype=torch.int32, device="cuda")
    for k in range(n_sets):
        tree.accumulate_weights(cam, poses(k), api.RenderOptions(), hits=hits, want=(), fp_mode=fp_mode)
    torch.cuda.synchronize()
    hits_per_frame = int(hits.view(-1).to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) / (n_sets * nf)
    del hits
    basis = stree.basis_dim
    run = 3 * basis + 1 if basis in (4, 9, 16, 25) else 4     # floats a hit adds (vr_dev_backward.h GradTraits::kRun)

    # clocks and caches up, the buffer sees the whole pass, launches per window
    for key in KEYS:
        window(key, 2 * n_sets)
    n_launch = {key: max(n_sets, (int(args.window * 1e3 / window(key, 2 * n_sets)) // n_sets + 1) * n_sets)
                for key in KEYS}
    ms = {key: [] for key in KEYS}
    for _ in range(args.reps):
        for key in KEYS:
            ms[key].append(window(key, n_launch[key]))
    status = tree.status()
    finite = bool(torch.isfinite(grad).all())
    tree.free_device()

    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
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
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
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
