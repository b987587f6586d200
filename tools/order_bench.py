#!/usr/bin/env python3
"""What ordering a ray batch with vr_order_rays costs and brings back, on the tree of a bench.py config and the
batch of tools/fit_bench.py -- ``--rays`` rays drawn at random (seeded) from the pixels of ``--frames`` bench poses
-- in one process.  For vr_fit_rays (with touched and sq_err) and for vr_render_rays (accum), per batch:

    (a)  a, a_b     the call on the batch as drawn: the path without the feature, and the yardstick; twice, the A/A
                    pair that gives the spread
    (b)  order_k    vr_order_rays alone, bits = k in 2..5 (order, origins, dirs and -- fit -- the targets as payload)
    (c)  ordered_k  (b) followed by the call on the ordered batch
    (d)  d          the call on the same rays in the frame launch's block order (8 x 8 pixel blocks in 4 x 4
                    super-blocks, the frame the minor index of a block: vr_dev_rays.h locate()), which the tool can
                    form because it knows each ray's frame and pixel: the floor an ordering can approach

Nothing is promised.  The default ``bits`` is the k with the smallest (c) of vr_fit_rays; ordering pays -- and the
tool exits 0 -- only if that (c) is below both (a) by more than the A/A spread (the largest of |a - a_b| and the
window spreads of a, a_b and that c).  The (a) / (d) ratio is the size of the prize for this batch size.

Figures, windows and spreads are those of tools/benchlib.py (``--window``, ``--reps``).  One JSON line per case, appended to ``--out``; ``--markdown`` prints the tables.

    python -m volrend_amd.build
    python tools/order_bench.py --out profiles/order_rays.jsonl --markdown

Measurement tooling, not the product.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys

import benchlib as bl

BITS = (2, 3, 4, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--frames", type=int, default=64, help="bench poses the rays are drawn from")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of iterations per timed window")
    ap.add_argument("--out", default="")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from volrend_amd import _abi, api

    sc = bl.scene(args.config)
    W, H, focal, stree, stream, sp = sc.W, sc.H, sc.focal, sc.stree, sc.stream, sc.sp
    if W % 32 or H % 32:
        raise SystemExit("order (d) is written for frames of whole 4 x 4 super-blocks")
    fp_mode = _abi.FP_STRICT
    f32 = torch.float32
    n, nf = args.rays, args.frames
    L = _abi.lib()

    # the batch of tools/fit_bench.py: pixels drawn from the frames of the bench poses
    gen = torch.Generator(device="cuda").manual_seed(1)
    m = torch.from_numpy(np.stack(sc.transforms[:nf]).astype(np.float32)).cuda()
    pick = torch.randint(0, nf * H * W, (n,), device="cuda", generator=gen)
    fr, px = pick // (H * W), pick % (H * W)
    ix, iy = px % W, px // W
    origins, dirs = bl.pixel_rays(torch, m, W, H, focal, fr, px)
    target = torch.rand((n, 3), dtype=f32, device="cuda", generator=gen)
    # (d): the rank of each ray in the frame launch's order -- super-block row, column, block row, column, frame, pixel
    block_key = ((((((iy // 32) * (W // 32) + ix // 32) * 4 + (iy // 8) % 4) * 4 + (ix // 8) % 4) * nf + fr) * 8
                 + iy % 8) * 8 + ix % 8
    block_order = torch.argsort(block_key, stable=True)
    options = api.RenderOptions()
    opt = options.to_c()
    grad_scale = 2.0 / (3 * n)

    tree = api.N3Tree.from_synth(stree)
    tree.reserve_rays(n, 1)
    grad = torch.zeros((stree.capacity, stree.N, stree.N, stree.N, stree.data_dim), dtype=f32, device="cuda")
    touched = torch.zeros(api.touched_words(tree), dtype=torch.int32, device="cuda")
    sq_err = torch.zeros(n, dtype=f32, device="cuda")
    accum = torch.zeros((n, 4), dtype=f32, device="cuda")
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    o_out, d_out, t_out = torch.zeros_like(origins), torch.zeros_like(dirs), torch.zeros_like(target)
    ws_bytes = int(L.vr_order_rays_workspace(n))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")

    def rays_c(o, d):
        r = _abi.VrRays()
        r.origins, r.dirs = o.data_ptr(), d.data_ptr()
        return r

    lists = {"drawn": (origins, dirs, target), "ordered": (o_out, d_out, t_out),
             "block": tuple(a[block_order].contiguous() for a in (origins, dirs, target))}
    rays = {k: rays_c(v[0], v[1]) for k, v in lists.items()}
    out = _abi.VrRayOut()
    out.accum = accum.data_ptr()

    def fit(which):
        f = _abi.VrFit()
        f.target, f.grad_scale, f.grad_data = lists[which][2].data_ptr(), grad_scale, grad.data_ptr()
        f.touched, f.sq_err = touched.data_ptr(), sq_err.data_ptr()
        _abi.check(L.vr_fit_rays(tree.handle, n, C.byref(rays[which]), C.byref(opt), fp_mode, C.byref(f), sp))

    def render(which):
        _abi.check(L.vr_render_rays(tree.handle, n, C.byref(rays[which]), C.byref(opt), fp_mode, C.byref(out), sp))

    def order_rays(bits, payload):
        ro = _abi.VrRayOrder()
        ro.bits, ro.order, ro.origins_out, ro.dirs_out = bits, order.data_ptr(), o_out.data_ptr(), d_out.data_ptr()
        if payload:
            ro.payload, ro.payload_out, ro.payload_dim = target.data_ptr(), t_out.data_ptr(), 3
        _abi.check(L.vr_order_rays(tree.handle, n, C.byref(rays["drawn"]), C.byref(opt), fp_mode, C.byref(ro),
                                   ws.data_ptr(), ws_bytes, sp))

    # the ordered call computes what the call on the batch as drawn computes: sq_err bit for bit through `order`
    fit("drawn")
    torch.cuda.synchronize()
    ref_sq, ref_marks = sq_err.clone(), touched.clone()
    touched.zero_()
    order_rays(0, True)
    fit("ordered")
    torch.cuda.synchronize()
    back = torch.empty_like(sq_err)
    back[order.long()] = sq_err
    same_sq_err = bool(torch.equal(back.view(torch.int32), ref_sq.view(torch.int32)))
    same_marks = bool(torch.equal(touched, ref_marks))
    del ref_sq, ref_marks, back

    calls = {}
    for op, fn, payload in (("fit", fit, True), ("render", render, False)):
        calls[f"{op}_a"] = lambda fn=fn: fn("drawn")
        calls[f"{op}_a_b"] = lambda fn=fn: fn("drawn")
        for k in BITS:
            calls[f"{op}_order_{k}"] = lambda k=k, payload=payload: order_rays(k, payload)
            calls[f"{op}_ordered_{k}"] = lambda fn=fn, k=k, payload=payload: (order_rays(k, payload), fn("ordered"))
        calls[f"{op}_d"] = lambda fn=fn: fn("block")
    keys = tuple(calls)

    def window(key, n_calls):   # -> ms per batch
        return bl.timed(torch, stream, n_calls, lambda _: calls[key]())

    ms, n_calls, mean, spread = bl.measure(keys, window, warm=4, floor=4, window_s=args.window, reps=args.reps)
    status = tree.status()
    tree.free_device()

    common = {"config": args.config, "rays": n, "frames": nf, "capacity": stree.capacity, "data_dim": stree.data_dim,
              "reps": args.reps, "workspace_bytes": ws_bytes, "sq_err_bits_equal": same_sq_err,
              "marks_equal": same_marks, "status": status}
    lines, verdict = [], {}
    for op in ("fit", "render"):
        best = min(BITS, key=lambda k: mean[f"{op}_ordered_{k}"])
        c = f"{op}_ordered_{best}"
        aa = max(abs(mean[f"{op}_a"] - mean[f"{op}_a_b"]), spread[f"{op}_a"], spread[f"{op}_a_b"], spread[c])
        pays = mean[c] < min(mean[f"{op}_a"], mean[f"{op}_a_b"]) - aa
        verdict[op] = dict(best_bits=best, pays=bool(pays), aa_spread_ms=round(aa, 4),
                           a_over_d=round(mean[f"{op}_a"] / mean[f"{op}_d"], 4),
                           c_over_a=round(mean[c] / mean[f"{op}_a"], 4))
        for key in keys:
            if key.startswith(op + "_"):
                lines.append(dict(common, op=op, case=key[len(op) + 1:], ms=round(mean[key], 4),
                                  spread_ms=round(spread[key], 4), calls_per_window=n_calls[key], **verdict[op]))
    bl.emit(lines, args.out)
    if args.markdown:
        for op, name in (("fit", "`vr_fit_rays`"), ("render", "`vr_render_rays`")):
            v = verdict[op]
            print(f"| {name}, {args.config}, {n} rays of {nf} frames | ms | spread |")
            print("|---|---|---|")
            rows = [("a", "(a) as drawn (A)"), ("a_b", "(a) as drawn (B)")]
            rows += [(f"order_{k}", f"(b) `vr_order_rays`, bits = {k}") for k in BITS]
            rows += [(f"ordered_{k}", f"(c) (b) + the call on the ordered batch, bits = {k}") for k in BITS]
            rows += [("d", "(d) frame launch's block order")]
            for key, text in rows:
                print(f"| {text} | {mean[op + '_' + key]:.4f} | {spread[op + '_' + key]:.4f} |")
            print(f"\nbest bits {v['best_bits']}, (c) / (a) = {v['c_over_a']}, (a) / (d) = {v['a_over_d']}, A/A spread "
                  f"{v['aa_spread_ms']} ms: ordering {'pays' if v['pays'] else 'does not pay'}\n")
    ok = same_sq_err and same_marks and status == 0
    return 0 if ok and verdict["fit"]["pays"] else 1


if __name__ == "__main__":
    sys.exit(main())
