#!/usr/bin/env python3
"""Throughput of the bulk point queries (vr_query_points / vr_query_grid) on the bench tree.

    python tools/query_bench.py [--config C1] [--log2n 24] [--grid 256] [--seconds 0.5]
                                [--out profiles/query_points.jsonl]

Three point sets -- uniform random, jittered centres of occupied leaves (+- 0.6 of the leaf's size), a
grid^3 box through vr_query_grid -- times three output sets -- sigma, sigma + coeffs, sigma + rgb -- one JSON line each,
appended to --out.  Per line: points/s from HIP events around a warmed window of at least
--seconds of launches that ends in a synchronise; bytes in and out per point computed from the
shapes; the distinct records (leaves) the point set falls in, counted with a torch restatement of
the descent on the device; and the larger of two lower bounds with the fraction of it reached:
  lines : the distinct 128-byte record lines of the point set / 53.5 G random lines/s
          (profiles/r01_gather_ceiling.txt) -- every distinct record is fetched at least once; 0 when no
          record is read (the lookup structure is small enough to be served from the caches)
  stream: bytes in + out / 6.3 TB/s (the chip's measured copy rate)
A tenth line passes the grid's points as an array (sigma only): the grid query should not be slower.
A record, not a gate.  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

import benchlib as bl

ROOT = bl.ROOT

GATHER_LINES_PER_S = 53.5e9
STREAM_BYTES_PER_S = 6.3e12
OUTPUT_SETS = {"sigma": ("sigma",), "sigma+coeffs": ("sigma", "coeffs"), "sigma+rgb": ("sigma", "rgb")}


def occupied_leaves(child, data):
    """(centre float64 [m, 3], size float64 [m]) of the leaves with sigma > 0 of an N = 2 tree, in
    tree coordinates -- level by level, vectorised."""
    child = np.asarray(child).reshape(-1, 8)
    sigma = np.asarray(data).reshape(child.shape[0], 8, -1)[..., -1]
    offs = np.array([[k >> 2 & 1, k >> 1 & 1, k & 1] for k in range(8)], np.float64)
    nodes, corner, size = np.zeros(1, np.int64), np.zeros((1, 3)), 1.0
    centres, sizes = [], []
    while nodes.size:
        ch = child[nodes]
        size *= 0.5
        cor = corner[:, None, :] + size * offs[None, :, :]
        occ = (ch == 0) & (sigma[nodes] > 0)
        centres.append(cor[occ] + 0.5 * size)
        sizes.append(np.full(int(occ.sum()), size))
        inner = ch != 0
        nodes = (nodes[:, None] + ch)[inner]
        corner = cor[inner]
    return np.concatenate(centres), np.concatenate(sizes)


def distinct_leaves(torch, child_dev, pts_dev, chunk=1 << 22):
    """Number of distinct leaves the tree coordinates ``pts_dev`` [n, 3] fall in: the float descent of
    n3tree_query.hpp:13-48 (N = 2) in torch, on the device."""
    hi = 1.0 - 1e-6
    leaves = []
    for s in range(0, pts_dev.shape[0], chunk):
        x = pts_dev[s:s + chunk].clamp(0.0, hi)
        ptr = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
        leaf = torch.zeros_like(ptr)
        live = torch.arange(x.shape[0], device=x.device)
        while live.numel():
            x = x * 2
            k = x.floor()
            x = x - k
            sub = ptr + (k[:, 0] * 4 + k[:, 1] * 2 + k[:, 2]).long()
            skip = child_dev[sub].long()
            done = skip == 0
            leaf[live[done]] = sub[done]
            keep = ~done
            live, x, ptr = live[keep], x[keep], ptr[keep] + skip[keep] * 8
        leaves.append(torch.unique(leaf))
    return int(torch.unique(torch.cat(leaves)).numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_points.jsonl"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("query_bench needs a GPU")
    from volrend_amd import _abi, api
    L = _abi.lib()

    tree = bl.scene(args.config).stree
    t = api.N3Tree.from_synth(tree)
    n = 1 << args.log2n
    rng = np.random.default_rng(7)
    cen, size = occupied_leaves(tree.child, tree.data)
    pick = rng.integers(cen.shape[0], size=n)
    sets = {
        "uniform": rng.random((n, 3), dtype=np.float32),
        "occupied_leaves": (cen[pick] + size[pick, None] * (rng.random((n, 3)) * 1.2 - 0.6)).astype(np.float32),
    }
    del cen, size, pick
    child_dev = torch.from_numpy(np.array(tree.child).reshape(-1)).cuda()   # (a copy: the cached tree is a read-only map)
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    d_dev = torch.from_numpy(dirs).cuda()
    g = args.grid
    k = t.data_dim - 1
    record_lines = -(-2 * k // 128)  # 128-byte lines one record spans
    axis = (torch.arange(g, device="cuda", dtype=torch.float32) + 0.5) * (1.0 / g)
    grid_pts = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3).contiguous()
    stream = torch.cuda.Stream()
    lines = []
    for set_name in ("uniform", "occupied_leaves", "grid", "grid_as_array"):
        if set_name == "grid":
            npts, p_dev, distinct = g ** 3, None, distinct_leaves(torch, child_dev, grid_pts)
        elif set_name == "grid_as_array":
            npts, p_dev = g ** 3, grid_pts
        else:
            npts, p_dev = n, torch.from_numpy(sets[set_name]).cuda()
            distinct = distinct_leaves(torch, child_dev, p_dev)
        for out_name, want in OUTPUT_SETS.items():
            if set_name == "grid_as_array" and out_name != "sigma":
                continue
            # the C calls with their arguments marshalled once and the outputs allocated once: a launch
            # of the small shapes takes ~50 us, which the allocations of N3Tree.query would double
            outs = {w: torch.empty((npts, {"sigma": 1, "coeffs": k, "rgb": 3}[w]), device="cuda") for w in want}
            vo = _abi.VrQueryOut()
            for w in want:
                setattr(vo, w, outs[w].data_ptr())
            f3 = C.c_float * 3
            lo, hi, res = f3(0, 0, 0), f3(1, 1, 1), (C.c_int32 * 3)(g, g, g)
            gdir = C.byref(f3(0.0, 0.0, -1.0)) if "rgb" in want else None
            sp = stream.cuda_stream

            def launch():
                if p_dev is None:
                    rc = L.vr_query_grid(t.handle, C.byref(lo), C.byref(hi), C.byref(res), gdir, _abi.SPACE_TREE,
                                         C.byref(vo), sp)
                else:
                    rc = L.vr_query_points(t.handle, npts, p_dev.data_ptr(), d_dev.data_ptr() if "rgb" in want else None,
                                           _abi.SPACE_TREE, C.byref(vo), sp)
                _abi.check(rc)

            for _ in range(3):
                launch()
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                launch()
            stream.synchronize()
            reps = max(20, int(1.2 * args.seconds * 20 / (time.perf_counter() - t0)) + 1)
            sec = bl.timed(torch, stream, reps, lambda _: launch()) * 1e-3
            bytes_in = 0 if p_dev is None else 12 + (12 if "rgb" in want else 0)
            bytes_out = 4 + (4 * k if "coeffs" in want else 0) + (12 if "rgb" in want else 0)
            n_lines = distinct * record_lines if len(want) > 1 else 0
            t_lines = n_lines / GATHER_LINES_PER_S
            t_stream = npts * (bytes_in + bytes_out) / STREAM_BYTES_PER_S
            bound = "lines" if t_lines >= t_stream else "stream"
            row = dict(config=args.config, format=tree.data_format, points=set_name, outputs=out_name, n=npts,
                       launches=reps, window_s=round(sec * reps, 4), ms_per_launch=round(sec * 1e3, 4),
                       Gpoints_per_s=round(npts / sec / 1e9, 4), bytes_in_per_point=bytes_in,
                       bytes_out_per_point=bytes_out, distinct_records=distinct, distinct_record_lines=n_lines,
                       bound=bound,
                       bound_ms=round(max(t_lines, t_stream) * 1e3, 4),
                       fraction_of_bound=round(max(t_lines, t_stream) / sec, 4),
                       device=torch.cuda.get_device_name(0))
            lines.append(row)
        del p_dev, outs
        torch.cuda.empty_cache()
    assert t.status() == 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    bl.emit(lines, args.out)


if __name__ == "__main__":
    main()
