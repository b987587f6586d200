"""What the feature benchmarks (tools/*_bench.py) share: the windowed A/B protocol of DESIGN.md section 7, stated once.

A figure is the mean over one warmed window of >= ``--window`` seconds of back-to-back calls between two HIP events
(``timed``); ``--reps`` windows per case, interleaved over the cases; the spread of a case is max - min over its
windows (``measure``).  Beside the protocol: a second library build (``load_build``), the scene of a bench.py config
(``scene``), the rays of its pixels (``pixel_rays``) and the JSON record (``emit``).  torch and the library are
imported inside the functions that need them, so that a tool's ``--help`` needs neither.

Measurement tooling, not the product.
"""
from __future__ import annotations

import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(torch, stream, n, call):
    """``call(k)`` for k in range(n) between two HIP events on ``stream``, then a synchronise -> ms per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for k in range(n):
        call(k)
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure(keys, window, *, warm, floor, window_s, reps, multiple=1, after_round=None):
    """The interleaved protocol over ``window(key, n) -> ms per call`` (no torch here: a test hands it a fake).

    ``warm`` calls per key bring clocks and caches up (an MI355X out of idle needs tens of ms of work) and load the
    code objects; a second window of ``warm`` calls per key sizes that key's windows: the calls that fill
    ``window_s`` seconds, plus one, rounded up to a whole multiple of ``multiple`` (the pose sets a tool's calls
    rotate over), at least ``floor``.  Then ``reps`` rounds over ``keys`` in order, so that a drift of the box lands
    on every case alike; ``after_round(rep)`` runs behind each round (what a tool times on the host clock).
    -> (ms: the windows per key, n: calls per window, mean, spread = max - min)."""
    for key in keys:
        window(key, warm)
    n = {key: max(floor, (int(window_s * 1e3 / window(key, warm)) // multiple + 1) * multiple) for key in keys}
    ms = {key: [] for key in keys}
    for rep in range(reps):
        for key in keys:
            ms[key].append(window(key, n[key]))
        if after_round is not None:
            after_round(rep)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    return ms, n, mean, spread


def load_build(_abi, path, without=()):
    """A library build with the prototypes of _abi (minus the symbols an older build lacks)."""
    import ctypes as C
    L = C.CDLL(path)
    for name, (res, args) in _abi.PROTOTYPES.items():
        if name in without:
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    assert L.vr_abi_version() == _abi.ABI_VERSION
    return L


def scene(config):
    """The scene of a bench.py config -> W, H, focal, stree (bench.load_or_make_tree), transforms (the 200-pose
    orbit), stream (torch's current one) and sp, its pointer."""
    import torch
    from volrend_amd import api, synth
    import bench as B
    cfg = synth.CONFIGS[config]
    stree = B.load_or_make_tree(synth, config, 0, lambda: None)
    transforms = [synth.c2w_to_transform(p) for p in synth.make_poses(200)]
    stream = torch.cuda.current_stream()
    return types.SimpleNamespace(W=cfg["width"], H=cfg["height"], focal=cfg["focal"], stree=stree,
                                 transforms=transforms, stream=stream, sp=api._stream_ptr(stream))


def pixel_rays(torch, transforms_f32, W, H, focal, frame, pixel):
    """(origins, dirs) [n, 3] float32 on the device: the ray of pixel ``pixel[k]`` (scanline index) of the camera
    ``transforms_f32[frame[k]]`` ([frames, 12] on the device), formed in float32 as screen2worlddir forms it in the
    strict model: (m[i] x + m[3 + i] y) + m[6 + i] z with z = -1.  Not normalised (the library normalises)."""
    f32, m = torch.float32, transforms_f32
    f = torch.tensor(focal, dtype=f32, device=m.device)
    x = ((pixel % W).to(f32) - 0.5 * W) / f
    y = -((pixel // W).to(f32) - 0.5 * H) / f
    dirs = torch.stack([(m[frame, i] * x + m[frame, 3 + i] * y) - m[frame, 6 + i] for i in range(3)], dim=-1)
    return m[frame, 9:12].contiguous(), dirs.contiguous()


def emit(recs, out=""):
    """Print a record, or a list of records, as one JSON line each, and append the same lines to ``out`` if given."""
    text = "\n".join(json.dumps(r) for r in (recs if isinstance(recs, list) else [recs]))
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")
