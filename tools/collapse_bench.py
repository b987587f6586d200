#!/usr/bin/env python3
"""What collapsing nodes and compacting a tree on the device costs, next to plain copies of arrays of the output
sizes and next to the host round trip that was the only way before vr_collapse_plan / vr_collapse_apply.

One process.  The tree of a bench.py config is refined (in numpy, not timed) at a seeded ``--fractions`` of its
leaves and uploaded; the selection is then every NEW node plus a seeded ``--old`` of the original frontier nodes --
the refine / collapse cycle of an optimiser that keeps its node count within a budget:

    a   vr_collapse_plan + vr_collapse_apply with the three maps and two companion arrays: the binary16 values (MEAN)
        and a float32 master (MEAN); GPU time between two events (the plan's wait is inside)
    b   device-to-device copies (torch ``copy_``) of arrays of the OUTPUT sizes: child_out, the binary16 values, the
        master -- the floor of any restatement that writes new arrays
    c   a + vr_tree_upload from the collapsed device arrays (VrTreeDesc.memory = 1) + vr_tree_free; host wall clock
    d   vr_tree_read_data -> host -> the numpy restatement of child and data -> vr_tree_upload from the host arrays
        + vr_tree_free: what a caller had to do before (the master is not even rebuilt here); host wall clock

a and b follow tools/benchlib.py's windowed protocol (``--window``, ``--reps``); c and d are timed ``--trips`` times
each, alternating.  The tool FAILS when c is not faster than d beyond the larger of their spreads, or when the device
result is not the numpy restatement bit for bit; a / b is reported, with no threshold.  One JSON line per fraction,
appended to ``--out``.

    python tools/collapse_bench.py --config C1 --out profiles/collapse.jsonl

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
import time

import benchlib as bl


def refined(np, child, flags, data):
    """vr_refine's semantics in numpy (COPY): -> (child_out, data_out)."""
    cap, n3 = child.shape
    src_slot = np.flatnonzero(flags & (child.reshape(-1) == 0))
    child_out = np.zeros((cap + src_slot.size, n3), np.int32)
    child_out[:cap] = child
    child_out.reshape(-1)[src_slot] = cap + np.arange(src_slot.size) - src_slot // n3
    return child_out, np.concatenate([data, np.repeat(data[src_slot], n3, axis=0)])


def restate(np, child, sel, data):
    """The semantics of include/volrend_hip.h in numpy, MEAN: child [capacity, N^3], sel bool [capacity] over nodes,
    data float16 [capacity * N^3, dim] -> (child_out, data_out)."""
    cap, n3 = child.shape
    col = sel & ~(child != 0).any(axis=1)
    col[0] = False
    src_node = np.flatnonzero(~col)
    node_map = np.full(cap, -1, np.int64)
    node_map[src_node] = np.arange(src_node.size)
    n, j = np.nonzero(child)
    m = n + child[n, j].astype(np.int64)
    keep = ~col[n]
    n, j, m = n[keep], j[keep], m[keep]
    p, gone = node_map[n], col[m]
    child_out = np.zeros((src_node.size, n3), np.int32)
    child_out[p[~gone], j[~gone]] = node_map[m[~gone]] - p[~gone]
    data_out = data.reshape(cap, n3, -1)[src_node].reshape(src_node.size * n3, -1).copy()
    rec = data.reshape(cap, n3, -1)[m[gone]].astype(np.float32)
    total = rec[:, 0].copy()
    for k in range(1, n3):        # binary32, ascending slot order, one rounding per add
        total = total + rec[:, k]
    data_out[p[gone] * n3 + j[gone]] = (total / np.float32(n3)).astype(np.float16)
    return child_out, data_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--fractions", default="0.01,0.1", help="fractions of the leaves refined beforehand")
    ap.add_argument("--old", type=float, default=0.05, help="fraction of the original frontier nodes selected too")
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
    N, cap0, dd = stree.N, stree.capacity, stree.data_dim
    n3 = N ** 3
    child0 = np.array(stree.child, np.int32).reshape(cap0, n3)
    data0 = np.ascontiguousarray(stree.data, np.float16).reshape(cap0 * n3, dd)
    leaves = np.flatnonzero(child0.reshape(-1) == 0)
    frontier0 = np.flatnonzero(~(child0 != 0).any(axis=1))
    ok = True
    for frac in [float(x) for x in args.fractions.split(",")]:
        rng = np.random.default_rng(17)
        flags = np.zeros(cap0 * n3, bool)
        flags[rng.choice(leaves, int(frac * leaves.size), replace=False)] = True
        child_host, data_host = refined(np, child0, flags, data0)
        cap = child_host.shape[0]
        n_slots = cap * n3
        tree = api.N3Tree.from_arrays(child_host.reshape(cap, N, N, N), data_host.reshape(cap, N, N, N, dd),
                                      stree.offset, stree.invradius3, stree.data_format, stree.extra)
        sel_host = np.arange(cap) >= cap0
        sel_host[rng.choice(frontier0[frontier0 > 0], int(args.old * frontier0.size), replace=False)] = True
        child = torch.from_numpy(child_host).cuda()
        data = tree.read_data()
        master = tree.read_data(dtype=torch.float32)
        ws = torch.empty(int(L.vr_collapse_workspace(N, cap)), dtype=torch.uint8, device="cuda")
        sel = _ops._pack_bits(torch.from_numpy(sel_host).cuda())
        torch.cuda.synchronize()
        r = _abi.VrCollapse()
        r.child, r.sel, r.workspace, r.workspace_bytes = child.data_ptr(), sel.data_ptr(), ws.data_ptr(), ws.numel()
        r.capacity, r.N = cap, N
        n_keep = C.c_int64(0)
        _abi.check(L.vr_collapse_plan(C.byref(r), C.byref(n_keep), sp))
        n_keep = int(n_keep.value)
        out_slots = n_keep * n3
        child_out = torch.empty(out_slots, dtype=torch.int32, device="cuda")
        node_map, into_slot = (torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2))
        src_node = torch.empty(n_keep, dtype=torch.int32, device="cuda")
        data_out = torch.empty(out_slots * dd, dtype=torch.float16, device="cuda")
        master_out = torch.empty(out_slots * dd, dtype=torch.float32, device="cuda")
        arrays = (_abi.VrCollapseArray * 2)()
        for a, s, d_, eb in zip(arrays, (data, master), (data_out, master_out), (2, 4)):
            a.src, a.dst, a.elem_bytes, a.dim, a.rule = s.data_ptr(), d_.data_ptr(), eb, dd, _abi.COLLAPSE_MEAN
        r.child_out, r.node_map, r.src_node, r.into_slot = (x.data_ptr() for x in (child_out, node_map, src_node,
                                                                                    into_slot))
        r.n_keep, r.arrays, r.n_arrays = n_keep, arrays, 2
        copies = [(torch.empty_like(x), x) for x in (child_out, data_out, master_out)]

        def collapse():
            planned = C.c_int64(0)
            _abi.check(L.vr_collapse_plan(C.byref(r), C.byref(planned), sp))
            _abi.check(L.vr_collapse_apply(C.byref(r), sp))

        def call(key):
            if key == "a":
                collapse()
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
            collapse()
            _abi.check(L.vr_stream_sync(sp))
            upload(child_out.data_ptr(), data_out.data_ptr(), n_keep, 1)
            return (time.perf_counter() - t0) * 1e3

        def trip_d():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = tree.read_data(stream=stream).cpu().numpy().reshape(n_slots, dd)
            c_out, d_out = restate(np, child_host, sel_host, host)
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
        exact = c_want.shape[0] == n_keep and \
            bool(np.array_equal(child_out.cpu().numpy(), c_want.reshape(-1))) and \
            bool(np.array_equal(data_out.cpu().numpy().view(np.uint16), d_want.view(np.uint16).reshape(-1)))
        mc, md = sum(cs) / len(cs), sum(ds) / len(ds)
        faster = md - mc > max(max(cs) - min(cs), max(ds) - min(ds))
        ok = ok and exact and faster
        moved = n_slots * (4 + 6 * dd) + out_slots * (4 + 6 * dd)
        bl.emit({"config": args.config, "fraction": frac, "old": args.old, "capacity": cap, "data_dim": dd,
                 "n_keep": n_keep, "n_collapsed": cap - n_keep,
                 "bytes_read_plus_written": moved, "calls_per_window": n_calls, "reps": args.reps,
                 "ms": {k: round(mean[k], 3) for k in mean}, "spread_ms": {k: round(spread[k], 3) for k in spread},
                 "a_over_b": round(mean["a"] / mean["b"], 3), "c_ms": [round(x, 1) for x in cs],
                 "d_ms": [round(x, 1) for x in ds], "d_over_c": round(md / mc, 2), "c_faster_than_d": bool(faster),
                 "exact": exact,
                 "what": "a plan + apply (maps, f16 values + f32 master, MEAN), b device copies of the output arrays, "
                         "c a + upload from device arrays, d read_data -> host -> numpy -> upload from host"}, args.out)
        tree.free_device()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
