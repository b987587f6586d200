#!/usr/bin/env python3
"""What slot geometry on the device costs, next to plain device writes of the same output bytes and next to the host
round trip that was the only way before vr_tree_geometry / vr_slot_points.

One process, the tree of a bench.py config, its child array on the device:

    g    vr_tree_geometry, all three outputs (parent_slot, node_depth, node_origin: 20 bytes per node)
    gd   vr_tree_geometry with node_depth and node_origin only: the parent links then live in capacity * 4 bytes of
         the device's stream-ordered pool, taken and returned inside the call (what N3Tree.slot_points(geometry=None)
         runs); the event-timed figure is GPU time, ``gd_host_ms`` the host time of one call + wait, next to g's
    gf   a device fill (torch ``fill_``) of the same 20 bytes per node -- the floor of writing the outputs
    p1   vr_slot_points over ALL leaves, k = 1, CENTER, all three outputs (20 bytes per leaf)
    c1   a device-to-device copy (torch ``copy_``) of the same output bytes
    p8   the same with k = 8, JITTER (104 bytes per leaf)
    c8   its copy
    t    g + p1 on the stream and a wait; host wall clock
    h    the host path they replace: child -> host, a level-by-level numpy walk, the k = 1 points in numpy, the points
         and depths back to the device; host wall clock

g .. c8 follow tools/benchlib.py's windowed protocol (``--window``, ``--reps``; the spread of a case over its windows
is its A/A spread); t and h are timed ``--trips`` times each, alternating.  The tool FAILS when t is not faster than h
beyond the larger of their spreads, or when the device results are not the host path's bit for bit; the ratios to the
fills and copies are reported, with no threshold.  One JSON line, appended to ``--out``.

    python tools/geometry_bench.py --config C1 --out profiles/geometry.jsonl

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
import time

import benchlib as bl


def host_geometry(np, child, N):
    """The numpy walk a caller had to write: level by level from the root -> (parent_slot, node_depth, node_origin)."""
    cap, n3 = child.shape
    parent, depth = np.full(cap, -1, np.int32), np.full(cap, -1, np.int32)
    origin = np.zeros((cap, 3), np.uint64)
    frontier = np.zeros(1, np.int64)
    depth[0] = 0
    while frontier.size:
        rows = child[frontier]
        f, j = np.nonzero(rows)
        n = frontier[f]
        m = n + rows[f, j]
        parent[m], depth[m] = n * n3 + j, depth[n] + 1
        origin[m] = origin[n] * np.uint64(N) + np.stack([j // (N * N), j // N % N, j % N], axis=1).astype(np.uint64)
        frontier = m
    return parent, depth, origin.astype(np.uint32)


def host_centres(np, depth, origin, N, slots):
    """The CENTER points of include/volrend_hip.h in numpy -> (points float32 [n, 1, 3], depth, side)."""
    n3 = N ** 3
    m, j = slots // n3, slots % n3
    D = np.cumprod(np.full(66, float(N)))[depth[m]]
    I = origin[m].astype(np.uint64) * np.uint64(N) + np.stack([j // (N * N), j // N % N, j % N], 1).astype(np.uint64)
    x = (I.astype(np.float64) + 0.5) / D[:, None]
    f = x.astype(np.float32)
    up = f.astype(np.float64) > x
    f[up] = np.nextafter(f[up], np.float32(0))
    return f[:, None, :], depth[m], (1.0 / D).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of calls per timed window")
    ap.add_argument("--trips", type=int, default=3, help="timed runs of t and of h")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from volrend_amd import _abi

    sc = bl.scene(args.config)
    stree, stream, sp = sc.stree, sc.stream, sc.sp
    L = _abi.lib()
    N, cap = stree.N, stree.capacity
    n3 = N ** 3
    child_host = np.ascontiguousarray(np.array(stree.child, np.int32).reshape(cap, n3))
    child = torch.from_numpy(child_host).cuda()
    i32 = dict(dtype=torch.int32, device="cuda")
    parent, node_depth, node_origin = torch.empty(cap, **i32), torch.empty(cap, **i32), torch.empty((cap, 3), **i32)
    fill = torch.empty(5 * cap, **i32)
    leaves = torch.nonzero(child.reshape(-1) == 0).reshape(-1).to(torch.int32)
    n = leaves.numel()
    g = _abi.VrGeometry()
    g.child, g.capacity, g.N = child.data_ptr(), cap, N
    g.parent_slot, g.node_depth, g.node_origin = parent.data_ptr(), node_depth.data_ptr(), node_origin.data_ptr()
    calls = {}
    for key, k, mode in (("1", 1, _abi.POINTS_CENTER), ("8", 8, _abi.POINTS_JITTER)):
        out = (torch.empty((n, k, 3), dtype=torch.float32, device="cuda"), torch.empty(n, **i32),
               torch.empty(n, dtype=torch.float32, device="cuda"))
        p = _abi.VrSlotPoints()
        p.node_depth, p.node_origin, p.slots = node_depth.data_ptr(), node_origin.data_ptr(), leaves.data_ptr()
        p.points, p.depth, p.side = (x.data_ptr() for x in out)
        p.capacity, p.n, p.N, p.k, p.mode, p.seed = cap, n, N, k, mode, 1
        copies = [(torch.empty_like(x), x) for x in out]
        calls["p" + key] = lambda p=p: _abi.check(L.vr_slot_points(C.byref(p), sp))
        calls["c" + key] = lambda copies=copies: [dst.copy_(src, non_blocking=True) for dst, src in copies]
        calls["out" + key] = out
    calls["g"] = lambda: _abi.check(L.vr_tree_geometry(C.byref(g), sp))
    gd = _abi.VrGeometry()
    gd.child, gd.capacity, gd.N = child.data_ptr(), cap, N
    gd.node_depth, gd.node_origin = node_depth.data_ptr(), node_origin.data_ptr()
    calls["gd"] = lambda: _abi.check(L.vr_tree_geometry(C.byref(gd), sp))
    calls["gf"] = lambda: fill.fill_(-1)
    keys = ("g", "gd", "gf", "p1", "c1", "p8", "c8")
    calls["g"]()
    torch.cuda.synchronize()
    ms, n_calls, mean, spread = bl.measure(keys, lambda k, m: bl.timed(torch, stream, m, lambda _: calls[k]()),
                                           warm=3, floor=3, window_s=args.window, reps=args.reps)

    def host_ms(key):
        """One call and a wait on the host clock, out of a synchronised device: a pool allocation shows here."""
        out = []
        for _ in range(max(args.trips, 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[key]()
            _abi.check(L.vr_stream_sync(sp))
            out.append(round((time.perf_counter() - t0) * 1e3, 3))
        return out

    def trip_t():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calls["g"]()
        calls["p1"]()
        _abi.check(L.vr_stream_sync(sp))
        return (time.perf_counter() - t0) * 1e3

    def trip_h():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = child.cpu().numpy()
        geo = host_geometry(np, host, N)
        slots = np.flatnonzero(host.reshape(-1) == 0)
        pts, d, side = host_centres(np, geo[1], geo[2], N, slots)
        dev = [torch.from_numpy(x).cuda() for x in (pts, d, side)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, geo, dev

    trip_t()
    ts, hs = [], []
    for _ in range(args.trips):
        ts.append(trip_t())
        t, geo, dev = trip_h()
        hs.append(t)
    reach = geo[1] >= 0
    exact = bool(np.array_equal(parent.cpu().numpy(), geo[0]) and np.array_equal(node_depth.cpu().numpy(), geo[1]) and
                 np.array_equal(node_origin.cpu().numpy().view(np.uint32)[reach], geo[2][reach]) and
                 all(torch.equal(a, b) for a, b in zip(calls["out1"], dev)))
    mt, mh = sum(ts) / len(ts), sum(hs) / len(hs)
    faster = mh - mt > max(max(ts) - min(ts), max(hs) - min(hs))
    bl.emit({"config": args.config, "capacity": cap, "N": N, "leaves": n, "max_depth": int(geo[1].max()),
             "calls_per_window": n_calls, "reps": args.reps,
             "ms": {k: round(mean[k], 4) for k in keys}, "spread_ms": {k: round(spread[k], 4) for k in keys},
             "g_host_ms": host_ms("g"), "gd_host_ms": host_ms("gd"), "g_over_gf": round(mean["g"] / mean["gf"], 2), "p1_over_c1": round(mean["p1"] / mean["c1"], 2),
             "p8_over_c8": round(mean["p8"] / mean["c8"], 2), "t_ms": [round(x, 2) for x in ts],
             "h_ms": [round(x, 1) for x in hs], "h_over_t": round(mh / mt, 1), "t_faster_than_h": bool(faster),
             "exact": exact,
             "what": "g vr_tree_geometry (3 outputs), gd the same without parent_slot (links in the stream-ordered "
                     "pool), gf fill of the same bytes, p1 / p8 vr_slot_points over all leaves "
                     "(k = 1 CENTER / k = 8 JITTER), c1 / c8 device copies of their output bytes, t g + p1 + wait, "
                     "h child -> host, numpy walk and points, points -> device"}, args.out)
    return 0 if exact and faster else 1


if __name__ == "__main__":
    sys.exit(main())
