#!/usr/bin/env python3
"""What refining a tree on the device costs, next to plain copies of the same arrays and next to the host round trip
that was the only way before vr_refine_plan / vr_refine_apply.

One process, the tree of a bench.py config, a seeded selection of ``--fractions`` of its leaves:

    a   vr_refine_plan + vr_refine_apply with two companion arrays: the binary16 values (COPY) and a float32 master
        (COPY); GPU time between two events (the plan's wait is inside)
    b   device-to-device copies (torch ``copy_``) of arrays of the OUTPUT sizes: child_out, the binary16 values, the
        master -- the floor of any restatement that writes new arrays
    c   a + vr_tree_upload from the refined device arrays (VrTreeDesc.memory = 1) + vr_tree_free; host wall clock
    d   vr_tree_read_data -> host -> the numpy restatement of child and data -> vr_tree_upload from the host arrays
        + vr_tree_free: what a caller had to do before (the master is not even rebuilt here); host wall clock

a and b follow tools/benchlib.py's windowed protocol (``--window``, ``--reps``); c and d are timed ``--trips`` times
each, alternating.  The tool FAILS when c is not faster than d beyond the larger of their spreads, or when the device
result is not the numpy restatement bit for bit; a / b is reported, with no threshold.  One JSON line per fraction,
appended to ``--out``.

    python tools/refine_bench.py --config C1 --out profiles/refine.jsonl

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
import time

import benchlib as bl


def restate(np, child, sel, data):
    """The semantics of include/volrend_hip.h in numpy: child [capacity, N^3], sel bool [capacity * N^3], data
    [capacity * N^3, dim] -> (child_out, src_slot, data_out)."""
    cap, n3 = child.shape
    src_slot = np.flatnonzero(sel & (child.reshape(-1) == 0))
    child_out = np.zeros((cap + src_slot.size, n3), np.int32)
    child_out[:cap] = child
    child_out.reshape(-1)[src_slot] = cap + np.arange(src_slot.size) - src_slot // n3
    return child_out, src_slot, np.concatenate([data, np.repeat(data[src_slot], n3, axis=0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--fractions", default="0.01,0.1", help="fractions of the leaves to refine")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timed window")
    ap.add_argument("--trips", type=int, default=3, help="timed runs of c and of d")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from volrend_amd import _abi, _ops, api

    sc = bl.scene(args.config)
    stree, stream, sp = sc.stree, sc.stream, sc.sp
    L = _abi.lib()
    tree = api.N3Tree.from_synth(stree)
    N, cap, dd = stree.N, stree.capacity, stree.data_dim
    n3 = N ** 3
    n_slots = cap * n3
    child_host = np.array(stree.child, np.int32).reshape(cap, n3)
    child = torch.from_numpy(child_host).cuda()
    data = tree.read_data()
    master = tree.read_data(dtype=torch.float32)
    ws = torch.empty(int(L.vr_refine_workspace(N, cap)), dtype=torch.uint8, device="cuda")
    leaves = np.flatnonzero(child_host.reshape(-1) == 0)
    ok = True
    for frac in [float(x) for x in args.fractions.split(",")]:
        flags = np.zeros(n_slots, bool)
        flags[np.random.default_rng(17).choice(leaves, int(frac * leaves.size), replace=False)] = True
        sel = _ops._pack_bits(torch.from_numpy(flags).cuda())
        torch.cuda.synchronize()
        r = _abi.VrRefine()
        r.child, r.sel, r.workspace, r.workspace_bytes = child.data_ptr(), sel.data_ptr(), ws.data_ptr(), ws.numel()
        r.capacity, r.N = cap, N
        n_new = C.c_int64(0)
        _abi.check(L.vr_refine_plan(C.byref(r), C.byref(n_new), sp))
        n_new = int(n_new.value)
        out_slots = (cap + n_new) * n3
        child_out = torch.empty(out_slots, dtype=torch.int32, device="cuda")
        src_slot = torch.empty(max(n_new, 1), dtype=torch.int32, device="cuda")
        data_out = torch.empty(out_slots * dd, dtype=torch.float16, device="cuda")
        master_out = torch.empty(out_slots * dd, dtype=torch.float32, device="cuda")
        arrays = (_abi.VrRefineArray * 2)()
        for a, s, d_, eb in zip(arrays, (data, master), (data_out, master_out), (2, 4)):
            a.src, a.dst, a.elem_bytes, a.dim, a.fill = s.data_ptr(), d_.data_ptr(), eb, dd, _abi.REFINE_COPY
        r.child_out, r.src_slot, r.n_new, r.arrays, r.n_arrays = child_out.data_ptr(), src_slot.data_ptr(), n_new, arrays, 2
        copies = [(torch.empty_like(x), x) for x in (child_out, data_out, master_out)]

        def refine():
            planned = C.c_int64(0)
            _abi.check(L.vr_refine_plan(C.byref(r), C.byref(planned), sp))
            _abi.check(L.vr_refine_apply(C.byref(r), sp))

        def call(key):
            if key == "a":
                refine()
            else:
                for dst, src in copies:
                    dst.copy_(src, non_blocking=True)

        def upload(child_ptr, data_ptr, capacity, memory):
            d = _abi.VrTreeDesc()
            L.vr_default_tree_desc(C.byref(d))
            d.child, d.data, d.memory = child_ptr, data_ptr, memory
            for i in range(3):
                d.offset[i], d.scale[i] = float(stree.offset[i]), float(stree.invradius3[i])
            d.N, d.capacity, d.data_dim = N, capacity, dd
            d.format, d.basis_dim, d.ndc_width = _abi.FORMATS[stree.format_name], stree.basis_dim, -1.0
            h = C.c_void_p()
            _abi.check(L.vr_tree_upload(C.byref(d), C.byref(h)))
            L.vr_tree_free(h)

        def trip_c():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            refine()
            _abi.check(L.vr_stream_sync(sp))
            upload(child_out.data_ptr(), data_out.data_ptr(), cap + n_new, 1)
            return (time.perf_counter() - t0) * 1e3

        def trip_d():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = tree.read_data(stream=stream).cpu().numpy().reshape(n_slots, dd)
            c_out, _, d_out = restate(np, child_host, flags, host)
            upload(c_out.ctypes.data, d_out.ctypes.data, c_out.shape[0], 0)
            return (time.perf_counter() - t0) * 1e3, c_out, d_out

        ms, n_calls, mean, spread = bl.measure(("a", "b"), lambda k, n: bl.timed(torch, stream, n, lambda _: call(k)),
                                               warm=3, floor=3, window_s=args.window, reps=args.reps)
        trip_c()
        cs, ds = [], []
        for _ in range(args.trips):
            cs.append(trip_c())
            t, c_want, d_want = trip_d()
            ds.append(t)
        exact = bool(np.array_equal(child_out.cpu().numpy(), c_want.reshape(-1))) and \
            bool(np.array_equal(data_out.cpu().numpy().view(np.uint16), d_want.view(np.uint16).reshape(-1)))
        mc, md = sum(cs) / len(cs), sum(ds) / len(ds)
        faster = md - mc > max(max(cs) - min(cs), max(ds) - min(ds))
        ok = ok and exact and faster
        moved = n_slots * (4 + 6 * dd) + out_slots * (4 + 6 * dd)
        bl.emit({"config": args.config, "fraction": frac, "capacity": cap, "data_dim": dd, "n_new": n_new,
                 "bytes_read_plus_written": moved, "calls_per_window": n_calls, "reps": args.reps,
                 "ms": {k: round(mean[k], 3) for k in mean}, "spread_ms": {k: round(spread[k], 3) for k in spread},
                 "a_over_b": round(mean["a"] / mean["b"], 3), "c_ms": [round(x, 1) for x in cs],
                 "d_ms": [round(x, 1) for x in ds], "d_over_c": round(md / mc, 2), "c_faster_than_d": bool(faster),
                 "exact": exact,
                 "what": "a plan + apply (f16 values + f32 master), b device copies of the output arrays, c a + upload "
                         "from device arrays, d read_data -> host -> numpy -> upload from host"}, args.out)
    tree.free_device()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
