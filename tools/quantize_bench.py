#!/usr/bin/env python3
"""What quantising a tree on the device costs and what it does to the picture.

One process, the tree of a bench.py config uploaded and read back with vr_tree_read_data (what N3Tree.quantize does):

    q      vr_quantize of those values: ``--retain`` basis functions kept, ``--bits`` levels, sigma_thresh 2.0 -- the
           defaults of scripts/compress_octree.py -- with preallocated outputs and workspace; event-timed on the
           stream, following tools/benchlib.py's windowed protocol (``--window``, ``--reps``; the spread over the
           windows is the A/A spread)
    floor  the bare sorts inside it: n_quant * bits calls of rocprim::radix_sort_pairs over n_slots (uint32, uint32)
           pairs and the same key bits, with nothing around them (tools/ubench/sort_floor.hip, a process of its own,
           built here on first use)
    psnr   ``--frames`` frames of the config rendered from a quantised upload of q's outputs against the same frames
           of the original tree: 10 log10(255^2 / mean squared difference of the RGB bytes)

All three are recorded, none is gated: there is no host implementation of the cut to compare a time against, and the
PSNR of a synthetic scene says little about a trained one.  The tool fails only when the quantised upload does not
hold the decode of q's outputs.  One JSON line, appended to ``--out``.

    python tools/quantize_bench.py --config C1 --out profiles/quantize.jsonl

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import subprocess
import sys

import benchlib as bl

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR_SRC = os.path.join(HERE, "ubench", "sort_floor.hip")
FLOOR_EXE = os.path.join(HERE, "ubench", "sort_floor")


def sort_floor(n_slots, bits, reps):
    """-> ms per sort and level, from a fresh child process."""
    from volrend_amd import build as vb
    if not os.path.exists(FLOOR_EXE) or os.path.getmtime(FLOOR_EXE) < os.path.getmtime(FLOOR_SRC):
        subprocess.check_call([vb.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", FLOOR_SRC, "-o", FLOOR_EXE])
    out = subprocess.check_output([FLOOR_EXE, str(n_slots), str(bits), str(reps)], text=True, timeout=600)
    return [float(l.split()[2]) for l in out.splitlines() if l.startswith("level ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--bits", type=int, default=16)
    ap.add_argument("--retain", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of calls per timed window")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from volrend_amd import _abi, api

    sc = bl.scene(args.config)
    stree, stream, sp = sc.stree, sc.stream, sc.sp
    L = _abi.lib()
    t = api.N3Tree.from_synth(stree)
    data = t.read_data()
    dim, n_slots = t.data_dim, t.capacity * t.N ** 3
    n_quant = (dim - 1) // 3 - args.retain
    f16 = dict(dtype=torch.float16, device="cuda")
    out = {"quant_colors": torch.empty((n_quant, 65536, 3), **f16),
           "quant_map": torch.empty((n_quant, n_slots), dtype=torch.int16, device="cuda"),
           "sigma": torch.empty(n_slots, **f16), "data_retained": torch.empty((args.retain, n_slots, 3), **f16)}
    need = int(L.vr_quantize_workspace(n_slots, dim))
    work = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    q = _abi.VrQuantize()
    q.data = data.data_ptr()
    q.quant_colors, q.quant_map, q.sigma = (out[k].data_ptr() for k in ("quant_colors", "quant_map", "sigma"))
    q.data_retained = out["data_retained"].data_ptr() if args.retain else None
    q.workspace, q.workspace_bytes = (work.data_ptr() + 255) // 256 * 256, need
    q.n_slots, q.data_dim, q.n_retained, q.bits, q.sigma_thresh = n_slots, dim, args.retain, args.bits, 2.0
    torch.cuda.synchronize()

    def call(_):
        _abi.check(L.vr_quantize(C.byref(q), sp))
    ms, n_calls, mean, spread = bl.measure(("q",), lambda k, m: bl.timed(torch, stream, m, call), warm=1, floor=1,
                                           window_s=args.window, reps=args.reps)
    levels = sort_floor(n_slots, args.bits, 3)
    floor_ms = n_quant * sum(levels)

    host = {k: v.cpu().numpy() for k, v in out.items()}
    kept = int((host["sigma"].astype(np.float32) > 2.0).sum())
    tq = api.N3Tree()
    tq._set_arrays(stree.child, None, stree.offset, stree.invradius3, stree.data_format, stree.extra, data_dim=dim)
    tq.quant_ = {"quant_colors": host["quant_colors"], "quant_map": host["quant_map"].view(np.uint16),
                 "sigma": host["sigma"], "data_retained": host["data_retained"] if args.retain else None}
    tq.load_device()
    dec = api._decode_arrays(tq.quant_["quant_colors"], tq.quant_["quant_map"], tq.quant_["sigma"],
                             tq.quant_["data_retained"], dim)
    exact = bool(np.array_equal(tq.read_data().cpu().numpy().reshape(-1, dim).view(np.uint16), dec.view(np.uint16)))
    del dec

    cam = api.Camera(sc.W, sc.H, sc.focal, sc.focal)
    psnr = []
    for i in range(args.frames):
        cam.transform = np.asarray(sc.transforms[(i * 67) % len(sc.transforms)], dtype=np.float32)
        imgs = []
        for tree in (t, tq):
            img = torch.zeros((sc.H, sc.W, 4), dtype=torch.uint8, device="cuda")
            api.launch_renderer(tree, cam, api.RenderOptions(), img, None, stream, True)
            torch.cuda.synchronize()
            imgs.append(img[..., :3].to(torch.float32))
        mse = float(((imgs[0] - imgs[1]) ** 2).mean())
        psnr.append(round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None)
    t.free_device()
    tq.free_device()
    bl.emit({"config": args.config, "capacity": t.capacity, "n_slots": n_slots, "data_dim": dim, "kept": kept,
             "bits": args.bits, "retain": args.retain, "n_quant": n_quant, "workspace_mb": round(need / 2 ** 20, 1),
             "calls_per_window": n_calls, "reps": args.reps, "q_ms": round(mean["q"], 2),
             "q_spread_ms": round(spread["q"], 2), "sorts": n_quant * args.bits,
             "sort_ms_per_level": [round(x, 4) for x in levels], "floor_ms": round(floor_ms, 2),
             "q_over_floor": round(mean["q"] / floor_ms, 2), "psnr_db": psnr, "upload_holds_the_decode": exact,
             "what": "q vr_quantize (event-timed), floor n_quant * bits bare rocprim::radix_sort_pairs of n_slots pairs "
                     "over the same key bits, psnr frames of the quantised upload against the original tree"}, args.out)
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
