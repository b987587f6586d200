#!/usr/bin/env python3
"""What vr_accumulate_weights costs next to the colour launch of the same poses, and what its per-hit
updates cost.

One process, the tree of a bench.py config at its frame size, ``--frames`` poses per launch over the
200-pose orbit (a pass = the launches that cover poses 0 .. 3 * frames - 1):

    (a)  vr_render_batch colour launches (the parent's machine code: tools/kernel_digest.py)
    (b)  max_weight only, into buffers that have already seen the whole pass (steady state)
    (c)  max_weight only, into buffers zeroed at the start of every pass (first touches; the memset is
         inside the window)
    (d)  max_weight + hits, steady state
    (b0) / (c0)  as (b) / (c) with the max issued unconditionally (tuning key weights_check = 0)

Figures, windows and spreads are those of tools/benchlib.py (``--window``, ``--reps``), a window a whole number
of passes.  Condition (exit status 1 when it fails): (b) < (a) by more than the largest spread.  (c), (d) and
the always-atomic forms get no threshold: they are recorded, with the atomics per second they imply
(hit samples per frame come from the hits buffer of one pass).  One JSON line per run, appended to
``--out``; ``--markdown`` prints the rows of the DESIGN.md table.

    python tools/weights_bench.py --config C1 --out profiles/leaf_weights.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import benchlib as bl

KEYS = ("a", "b", "c", "d", "b0", "c0")


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
    always = tree.clone_to(tree.info()["device"])     # the same arrays, the max without the checking load
    always.set_tuning(weights_check=0)
    always.reserve(W, H, nf)
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
    shape = (stree.capacity, stree.N, stree.N, stree.N)
    bufs = {k: torch.zeros(shape, dtype=torch.float32, device="cuda") for k in ("b", "c", "d", "b0", "c0")}
    hits = torch.zeros(shape, dtype=torch.int32, device="cuda")

    def outs(key):
        o = _abi.VrLeafWeights()
        o.max_weight = bufs[key].data_ptr()
        o.hits = hits.data_ptr() if key == "d" else None
        return o
    out = {k: outs(k) for k in bufs}

    def launch(key, k):
        if key == "a":
            colour[k % n_sets].launch(stream)
            return
        if key in ("c", "c0") and k % n_sets == 0:
            bufs[key].zero_()                          # a fresh pass: every first touch again
        t = always if key.endswith("0") else tree
        _abi.check(L.vr_accumulate_weights(t.handle, nf, cams[k % n_sets], C.byref(opt), fp_mode,
                                           C.byref(out[key]), sp))

    def window(key, n_launches):   # -> ms per launch of nf poses
        return bl.timed(torch, stream, n_launches, lambda k: launch(key, k))

    # hit samples per frame: the count buffer after exactly one pass
    tree.accumulate_weights(cam, [], api.RenderOptions(), want=("hits",))      # (the file-order tables)
    always.accumulate_weights(cam, [], api.RenderOptions(), want=("hits",))
    for k in range(n_sets):
        launch("d", k)
    torch.cuda.synchronize()
    hits_per_frame = int(hits.view(-1).to(torch.int64).bitwise_and(0xFFFFFFFF).sum().item()) / (n_sets * nf)
    slots_touched = int((hits != 0).sum().item())

    # the warm windows are two passes: the steady buffers (b, d, b0) have seen the whole pass before a timed window
    ms, n_launch, mean, spread = bl.measure(KEYS, window, warm=2 * n_sets, floor=n_sets, multiple=n_sets,
                                            window_s=args.window, reps=args.reps)
    status = {"tree": tree.status(), "always": always.status()}
    same = bool(torch.equal(bufs["b"], bufs["b0"]) and torch.equal(bufs["b"], bufs["d"]))
    tree.free_device()
    always.free_device()

    worst = max(spread.values())
    ok = mean["b"] < mean["a"] - worst
    per_frame = {k: mean[k] / nf for k in KEYS}

    def rate(key):   # G updates per second if every hit sample of the variant were one atomic
        return round(hits_per_frame / (per_frame[key] * 1e-3) / 1e9, 2)
    rec = {"config": args.config, "fp": args.fp, "frames_per_launch": nf, "width": W, "height": H,
           "launches_per_window": n_launch, "reps": args.reps,
           "ms_per_frame": {k: round(per_frame[k], 5) for k in KEYS},
           "spread_ms_per_frame": {k: round(spread[k] / nf, 5) for k in KEYS},
           "windows_ms_per_launch": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "hit_samples_per_frame": round(hits_per_frame), "slots_hit": slots_touched,
           "hits_added_G_per_s": {"d": rate("d")}, "max_issued_G_per_s": {"b0": rate("b0"), "c0": rate("c0")},
           "weights_over_colour": round(mean["b"] / mean["a"], 4),
           "steady_max_below_colour_by_more_than_spread": ok, "variants_agree": same, "status": status,
           "what": "a colour, b max steady, c max first pass, d max + hits steady, b0 / c0 the max always atomic"}
    bl.emit(rec, args.out)
    if args.markdown:
        names = {"a": "colour launch (`vr_render_batch`)", "b": "`max_weight`, steady state",
                 "c": "`max_weight`, first pass (zeroed buffers)", "d": "`max_weight` + `hits`, steady state",
                 "b0": "`max_weight` always atomic, steady state", "c0": "`max_weight` always atomic, first pass"}
        print(f"| {args.config} variant | ms / frame | spread | / colour |")
        print("|---|---|---|---|")
        for k in KEYS:
            print(f"| ({k}) {names[k]} | {per_frame[k]:.4f} | {spread[k] / nf:.4f} | {mean[k] / mean['a']:.2f} |")
    return 0 if ok and same and not any(status.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
