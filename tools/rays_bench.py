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

All colour variants write RGBA8 only.  Each figure is the mean over one warmed window of >= ``--window`` seconds
of back-to-back launches between two HIP events; ``--reps`` windows per variant, interleaved; the spread of a
variant is max - min over its windows.

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
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    from volrend_amd import _abi, api, synth
    import bench as B

    cfg = synth.CONFIGS[args.config]
    W, H, focal = cfg["width"], cfg["height"], cfg["focal"]
    if W % 32 or H % 32:
        raise SystemExit("order (c) is written for frames of whole 4 x 4 super-blocks")
    stree = B.load_or_make_tree(synth, args.config, 0, lambda: None)
    nf = args.frames
    transforms = [synth.c2w_to_transform(p) for p in synth.make_poses(200)][:nf]
    stream = torch.cuda.current_stream()
    sp = api._stream_ptr(stream)
    fp_mode = _abi.FP_STRICT
    cam = api.Camera(W, H, focal, focal)
    L = _abi.lib()
    n = nf * H * W

    # the frames' rays, scanline order: (m[i] x + m[3 + i] y) + m[6 + i] z in float32, as the strict kernel forms them
    f32 = torch.float32
    ix = torch.arange(W, dtype=f32, device="cuda")
    iy = torch.arange(H, dtype=f32, device="cuda")
    x = ((ix - 0.5 * W) / torch.tensor(focal, dtype=f32, device="cuda")).expand(H, W)
    y = (-(iy - 0.5 * H) / torch.tensor(focal, dtype=f32, device="cuda"))[:, None].expand(H, W)
    m = torch.from_numpy(np.stack(transforms).astype(np.float32)).cuda()        # [nf, 12]
    dirs = torch.stack([(m[:, i, None, None] * x + m[:, 3 + i, None, None] * y) - m[:, 6 + i, None, None]
                        for i in range(3)], dim=-1).reshape(n, 3).contiguous()
    origins = m[:, None, 9:12].expand(nf, H * W, 3).reshape(n, 3).contiguous()
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

    def window(key, n_launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n_launches):
            launch(key)
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n_launches   # ms per launch of nf poses

    # the lists give the frames' bytes (and the clocks come up)
    launch("a")
    same = {}
    for key in "bcd":
        out.zero_()
        launch(key)
        torch.cuda.synchronize()
        want = imgs.view(n, 4) if order[key] is None else imgs.view(n, 4)[order[key]]
        same[key] = bool(torch.equal(out, want))
    for key in KEYS:
        window(key, 2)
    n_launch = {key: max(1, int(args.window * 1e3 / window(key, 2)) + 1) for key in KEYS}
    ms = {key: [] for key in KEYS}
    for _ in range(args.reps):
        for key in KEYS:
            ms[key].append(window(key, n_launch[key]))
    status = tree.status()
    tree.free_device()

    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
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
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
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
