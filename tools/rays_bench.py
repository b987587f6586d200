#!/usr/bin/env python3
"""What a ray list costs next to the frames it was made from, and what the order of its rays costs.

One process, the tree of a bench.py config at its frame size, ``--frames`` poses of the 200-pose orbit per
launch; the rays of those frames are formed on the device as screen2worlddir forms them (strict model):

    (a)  vr_render_batch
    (b)  vr_render_rays, the frames' rays in scanline order, frame after frame
    (c)  the same rays in the order the frame launch marches them: 8 x 8 pixel blocks in 4 x 4 super-blocks,
         the frame the minor index of a block (vr_dev_rays.h locate())
    (d)  the same rays shuffled
    (e)  vr_render_backward
    (f)  vr_render_backward_rays in order (c)

All colour variants write RGBA8 only.  Figures, windows and spreads are those of tools/benchlib.py (``--window``,
``--reps``).

The one condition (exit status 1 when it fails): the march kernels of (c) are those of (a), byte for byte, and
its rays arrive in the same order, so (c) may exceed (a) only by what ray generation pays for reading 24 more
bytes per ray -- at half the chip's stream rate (``--stream-tbs`` / 2) -- plus the largest spread.  (b) and (d)
have no threshold: they are what an incoherent order costs.  One JSON line per run, appended to ``--out``;
``--markdown`` prints the rows of the DESIGN.md table.

    python tools/rays_bench.py --config C1 --out profiles/render_rays.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import numpy as np

import benchlib as bl

KEYS = ("a", "b", "c", "d", "e", "f")
NAMES = {"a": "`vr_render_batch`", "b": "`vr_render_rays`, scanline order", "c": "`vr_render_rays`, block order",
         "d": "`vr_render_rays`, shuffled", "e": "`vr_render_backward`", "f": "`vr_render_backward_rays`, block order"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of launches per timed window")
    ap.add_argument("--stream-tbs", type=float, default=6.3, help="the chip's measured stream rate, TB/s")
    ap.add_argument("--out", default="")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()

    import torch
    from volrend_amd import _abi, api

    sc = bl.scene(args.config)
    W, H, focal, stree, stream, sp = sc.W, sc.H, sc.focal, sc.stree, sc.stream, sc.sp
    if W % 32 or H % 32:
        raise SystemExit("order (c) is written for frames of whole 4 x 4 super-blocks")
    nf = args.frames
    transforms = sc.transforms[:nf]
    fp_mode = _abi.FP_STRICT
    cam = api.Camera(W, H, focal, focal)
    L = _abi.lib()
    n = nf * H * W

    # the frames' rays, scanline order, frame after frame
    f32 = torch.float32
    m = torch.from_numpy(np.stack(transforms).astype(np.float32)).cuda()        # [nf, 12]
    every = torch.arange(n, device="cuda")
    origins, dirs = bl.pixel_rays(torch, m, W, H, focal, every // (H * W), every % (H * W))
    del every
    pix = torch.arange(n, device="cuda").view(nf, H // 32, 4, 8, W // 32, 4, 8)   # f, sr, iy, ly, sc, ix, lx
    order = {"b": None, "c": pix.permute(1, 4, 2, 5, 0, 3, 6).reshape(-1),
             "d": torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))}
    rays = {k: ((origins, dirs) if o is None else (origins[o].contiguous(), dirs[o].contiguous()))
            for k, o in order.items()}
    del pix

    tree = api.N3Tree.from_synth(stree)
    tree.reserve(W, H, nf)
    tree.reserve_rays(n, 1)
    imgs = torch.zeros((nf, H, W, 4), dtype=torch.uint8, device="cuda")
    colour = api.PreparedBatch(tree, cam, transforms, api.RenderOptions(), list(imgs), True, fp_mode=fp_mode)
    out = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    opt = api.RenderOptions().to_c()
    cams = (_abi.VrCamera * nf)()
    for i, tr in enumerate(transforms):
        cam.transform = tr
        cams[i] = cam.to_c()
    g = torch.randn((n, 4), dtype=f32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    g_c = g[order["c"]].contiguous()
    grad = torch.zeros((stree.capacity, stree.N, stree.N, stree.N, stree.data_dim), dtype=f32, device="cuda")
    c_rays, c_out = {}, _abi.VrRayOut()
    c_out.rgba = out.data_ptr()
    for k, (o, d) in rays.items():
        c_rays[k] = _abi.VrRays()
        c_rays[k].origins, c_rays[k].dirs = o.data_ptr(), d.data_ptr()

    def launch(key):
        if key == "a":
            colour.launch(stream)
        elif key in "bcd":
            _abi.check(L.vr_render_rays(tree.handle, n, C.byref(c_rays[key]), C.byref(opt), fp_mode, C.byref(c_out), sp))
        elif key == "e":
            _abi.check(L.vr_render_backward(tree.handle, nf, cams, C.byref(opt), fp_mode, g.data_ptr(),
                                            grad.data_ptr(), sp))
        else:
            _abi.check(L.vr_render_backward_rays(tree.handle, n, C.byref(c_rays["c"]), C.byref(opt), fp_mode,
                                                 g_c.data_ptr(), grad.data_ptr(), sp))

    def window(key, n_launches):   # -> ms per launch of nf poses
        return bl.timed(torch, stream, n_launches, lambda _: launch(key))

    # the lists give the frames' bytes (and the clocks come up)
    launch("a")
    same = {}
    for key in "bcd":
        out.zero_()
        launch(key)
        torch.cuda.synchronize()
        want = imgs.view(n, 4) if order[key] is None else imgs.view(n, 4)[order[key]]
        same[key] = bool(torch.equal(out, want))
    ms, n_launch, mean, spread = bl.measure(KEYS, window, warm=2, floor=1, window_s=args.window, reps=args.reps)
    status = tree.status()
    tree.free_device()

    read_ms = n * 24 / (args.stream_tbs / 2 * 1e12) * 1e3            # per launch
    allowed = read_ms + max(spread.values())
    gap = mean["c"] - mean["a"]
    ok = gap <= allowed and all(same.values()) and not status
    rec = {"config": args.config, "fp": "strict", "frames_per_launch": nf, "width": W, "height": H, "rays": n,
           "launches_per_window": n_launch, "reps": args.reps,
           "ms_per_frame": {k: round(mean[k] / nf, 5) for k in KEYS},
           "spread_ms_per_frame": {k: round(spread[k] / nf, 5) for k in KEYS},
           "windows_ms_per_launch": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "c_minus_a_ms_per_frame": round(gap / nf, 5), "allowed_ms_per_frame": round(allowed / nf, 5),
           "ray_read_ms_per_frame": round(read_ms / nf, 5), "stream_TB_per_s": args.stream_tbs,
           "lists_equal_frames": same, "status": status, "condition_met": ok,
           "what": "a frames, b list scanline, c list block order, d list shuffled, e backward frames, "
                   "f backward list block order; colour variants write RGBA8 only"}
    bl.emit(rec, args.out)
    if args.markdown:
        print(f"| {args.config} variant | ms / frame | spread | / frames |")
        print("|---|---|---|---|")
        for k in KEYS:
            base = mean["a"] if k in "abcd" else mean["e"]
            print(f"| ({k}) {NAMES[k]} | {mean[k] / nf:.4f} | {spread[k] / nf:.4f} | {mean[k] / base:.2f} |")
        print(f"(c) - (a) = {gap / nf:.5f} ms per frame; allowed {allowed / nf:.5f} "
              f"({read_ms / nf:.5f} for 24 B per ray at {args.stream_tbs / 2:.2f} TB/s + the largest spread)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
