#!/usr/bin/env python3
"""What vr_tree_update_data and vr_tree_read_data cost, next to what a caller had to do before them and next to
a plain copy of the same bytes.

One process, the tree of a bench.py config:

    u16 / u32   vr_tree_update_data from a binary16 / binary32 array (values pass + lookup refresh)
    r16 / r32   vr_tree_read_data into a binary16 / binary32 array
    c_<key>     a device-to-device copy (torch ``copy_``) that moves the bytes <key> reads plus writes: half of
                them each way
    up          vr_tree_upload from the same device-resident arrays (VrTreeDesc.memory = 1) and vr_tree_free of
                the result: the only way to get new values into the renderer before; host wall clock, the call
                is synchronous

The bytes of a pass come from the shapes (bytes_of below): the file-side array, the padded records, the node
words (read, and written back for the update), the file-order table, and for the update's refresh every lookup
entry read and written plus the node words it gathers.  The GPU figures, their windows and spreads are those of
tools/benchlib.py (``--window``, ``--reps``); an upload is timed behind each round.  A record, not a gate: one JSON
line per run, appended to ``--out``; ``--markdown`` prints a table.

    python tools/update_bench.py --config C1 --out profiles/tree_update.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
import time

import benchlib as bl

PASSES = ("u16", "u32", "r16", "r32")


def bytes_of(info, capacity, n3, data_dim, lookup_bytes):
    """-> {pass: bytes read + bytes written}."""
    n_slots = capacity * n3
    nodes, leaves, table = 4 * n_slots, n_slots * info["leaf_stride"], 4 * capacity
    refresh = 2 * lookup_bytes + nodes if info["top_levels"] > 0 else 0
    out = {}
    for key, elem in (("16", 2), ("32", 4)):
        file_side = n_slots * data_dim * elem
        out["u" + key] = file_side + leaves + 2 * nodes + table + refresh
        out["r" + key] = file_side + leaves + nodes + table
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timed window")
    ap.add_argument("--uploads", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from volrend_amd import _abi, api

    sc = bl.scene(args.config)
    stree, stream = sc.stree, sc.stream
    L = _abi.lib()
    tree = api.N3Tree.from_synth(stree)
    info = tree.info()
    n3 = stree.N ** 3
    n_slots = stree.capacity * n3
    lookup_bytes = info["device_bytes"] - 4 * n_slots - n_slots * info["leaf_stride"] - 4
    moved = bytes_of(info, stree.capacity, n3, stree.data_dim, lookup_bytes)

    bufs = {"16": tree.read_data(), "32": tree.read_data(dtype=torch.float32)}   # the tree's own values, file order
    outs = {k: torch.empty_like(v) for k, v in bufs.items()}
    child_dev = torch.from_numpy(np.ascontiguousarray(stree.child)).cuda()
    half = max(moved.values()) // 2
    copy_src = torch.zeros(half, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty_like(copy_src)
    before = tree.read_data()
    torch.cuda.synchronize()

    def call(key):
        if key.startswith("c_"):
            n = moved[key[2:]] // 2
            copy_dst[:n].copy_(copy_src[:n], non_blocking=True)
        elif key[0] == "u":
            tree.update_data(bufs[key[1:]], stream=stream)
        else:
            tree.read_data(out=outs[key[1:]], stream=stream)

    def window(key, n_calls):   # -> ms per call
        return bl.timed(torch, stream, n_calls, lambda _: call(key))

    def upload_ms():
        d = _abi.VrTreeDesc()
        L.vr_default_tree_desc(C.byref(d))
        d.child, d.data, d.memory = child_dev.data_ptr(), bufs["16"].data_ptr(), 1
        for i in range(3):
            d.offset[i], d.scale[i] = float(stree.offset[i]), float(stree.invradius3[i])
        d.N, d.capacity, d.data_dim = stree.N, stree.capacity, stree.data_dim
        d.format, d.basis_dim, d.ndc_width = _abi.FORMATS[stree.format_name], stree.basis_dim, -1.0
        h = C.c_void_p()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _abi.check(L.vr_tree_upload(C.byref(d), C.byref(h)))
        ms = (time.perf_counter() - t0) * 1e3
        L.vr_tree_free(h)
        return ms

    keys = PASSES + tuple("c_" + k for k in PASSES)
    upload_ms()        # its code objects loaded; the warm windows make the two tables
    ups = []

    def upload_behind(rep):
        if rep < args.uploads:
            ups.append(upload_ms())
    ms, n_calls, mean, spread = bl.measure(keys, window, warm=8, floor=8, window_s=args.window, reps=args.reps,
                                           after_round=upload_behind)
    while len(ups) < args.uploads:
        ups.append(upload_ms())
    # every update wrote the tree's own values: nothing may have changed, and the read-backs return them
    unchanged = bool(torch.equal(before.view(torch.int16), tree.read_data().view(torch.int16)))
    exact = bool(torch.equal(outs["16"].view(torch.int16), before.view(torch.int16))) and \
        bool(torch.equal(outs["32"].view(torch.int32), before.float().view(torch.int32)))
    status = tree.status()
    tree.free_device()

    rec = {"config": args.config, "capacity": stree.capacity, "data_dim": stree.data_dim,
           "device_bytes": info["device_bytes"], "lookup_bytes": lookup_bytes, "top_levels": info["top_levels"],
           "brick_levels": info["brick_levels"], "brick_blocked": info["brick_blocked"],
           "bytes_moved": moved, "calls_per_window": n_calls, "reps": args.reps,
           "ms": {k: round(mean[k], 4) for k in keys}, "spread_ms": {k: round(spread[k], 4) for k in keys},
           "TB_per_s": {k: round(moved[k[-3:]] / (mean[k] * 1e-3) / 1e12, 3) for k in keys},
           "over_copy": {k: round(mean[k] / mean["c_" + k], 3) for k in PASSES},
           "upload_from_device_ms": [round(x, 2) for x in ups],
           "upload_over_update": {k: round(min(ups) / mean[k], 1) for k in ("u16", "u32")},
           "unchanged": unchanged, "read_back_exact": exact, "status": status,
           "what": "u update, r read-back, c_ a device copy of the same bytes, up vr_tree_upload from device arrays"}
    bl.emit(rec, args.out)
    if args.markdown:
        names = {"u16": "`vr_tree_update_data`, binary16", "u32": "`vr_tree_update_data`, binary32",
                 "r16": "`vr_tree_read_data`, binary16", "r32": "`vr_tree_read_data`, binary32"}
        print(f"| {args.config} pass | MB moved | ms | spread | copy of the same bytes, ms | / copy |")
        print("|---|---|---|---|---|---|")
        for k in PASSES:
            print(f"| {names[k]} | {moved[k] / 1e6:.0f} | {mean[k]:.3f} | {spread[k]:.3f} | {mean['c_' + k]:.3f} | "
                  f"{mean[k] / mean['c_' + k]:.2f} |")
        print(f"`vr_tree_upload` from the same device arrays: {min(ups):.1f}-{max(ups):.1f} ms")
    return 0 if unchanged and exact and not status else 1


if __name__ == "__main__":
    sys.exit(main())
