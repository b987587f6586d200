"""tools/benchlib.py, the measurement protocol under the feature benchmarks of DESIGN.md section 7 -- the order of
its windows, the sizing rule with every constant set a tool passes, the statistics, the record file -- and that
every tools/*_bench.py still answers ``--help`` without torch or the library.  No device."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib as bl  # noqa: E402

TOOLS = ["aov", "weights", "grad", "update", "rays", "query", "step", "fit", "order"]


def fake_window(ms_of, log):
    def window(key, n):
        log.append((key, n))
        return ms_of[key]
    return window


def test_protocol_order():
    """All keys at `warm`, all keys at `warm` again (the sizing pass), then `reps` rounds over the keys in order at
    the sized n; the hook runs behind each round.  0.5 s windows: 100 ms -> 5 + 1, 50 ms -> 10 + 1, 1000 ms -> the
    floor."""
    log = []
    window = fake_window({"a": 100.0, "b": 50.0, "c": 1000.0}, log)
    ms, n, mean, spread = bl.measure(("a", "b", "c"), window, warm=4, floor=4, window_s=0.5, reps=3,
                                     after_round=lambda rep: log.append(("round", rep)))
    warm = [("a", 4), ("b", 4), ("c", 4)]
    rounds = [("a", 6), ("b", 11), ("c", 4)]
    assert log == warm + warm + rounds + [("round", 0)] + rounds + [("round", 1)] + rounds + [("round", 2)]
    assert n == {"a": 6, "b": 11, "c": 4}
    assert ms == {"a": [100.0] * 3, "b": [50.0] * 3, "c": [1000.0] * 3}
    assert list(ms) == list(n) == list(mean) == list(spread) == ["a", "b", "c"]


# (warm, floor, multiple), window_s, {ms per call of the sizing window: calls per window} -- by hand:
# multiple == 1: max(floor, int(window_s * 1e3 / ms) + 1); else max(floor, (int(window_s * 1e3 / ms) // multiple + 1) * multiple).
# 1000 ms sizes below (or, where nothing can, on) the floor; the middle one divides the window exactly; 0.5 ms is well
# above.  Every duration and quotient is exact in binary floating point.
SIZING = [
    ((8, 4, 1), 0.5, {1000.0: 4, 50.0: 11, 0.5: 1001}),        # aov:  0 + 1 -> 4;  10 + 1;  1000 + 1
    ((8, 8, 1), 0.5, {1000.0: 8, 50.0: 11, 0.5: 1001}),        # update
    ((4, 4, 1), 0.5, {1000.0: 4, 50.0: 11, 0.5: 1001}),        # step, fit, order
    ((2, 1, 1), 0.5, {1000.0: 1, 50.0: 11, 0.5: 1001}),        # rays
    ((6, 3, 3), 0.5, {1000.0: 3, 50.0: 12, 0.5: 1002}),        # weights, grad: (0 + 1) 3;  (10 // 3 + 1) 3;  (333 + 1) 3
    ((6, 3, 3), 0.75, {1000.0: 3, 125.0: 9, 62.5: 15}),        # 750 / 125 = 6, a whole multiple: (2 + 1) 3;  (12 // 3 + 1) 3
]


@pytest.mark.parametrize("consts,window_s,want", SIZING, ids=[f"{c[0]}-{c[1]}" for c in SIZING])
def test_sizing_rule(consts, window_s, want):
    warm, floor, multiple = consts
    log = []
    keys = tuple(want)
    _, n, _, _ = bl.measure(keys, fake_window({k: k for k in keys}, log), warm=warm, floor=floor, multiple=multiple,
                            window_s=window_s, reps=1)
    assert n == want
    assert log[:2 * len(keys)] == [(k, warm) for k in keys] * 2
    assert log[2 * len(keys):] == [(k, want[k]) for k in keys]


def test_mean_and_spread():
    series = {"a": iter([9.0, 10.0, 3.0, 5.0, 4.0]), "b": iter([1.0, 1.0, 2.0, 2.0, 8.0])}   # warm, sizing, windows
    ms, _, mean, spread = bl.measure(("a", "b"), lambda key, n: next(series[key]), warm=1, floor=1, window_s=0.01,
                                     reps=3)
    assert ms == {"a": [3.0, 5.0, 4.0], "b": [2.0, 2.0, 8.0]}
    assert mean == {"a": 4.0, "b": 4.0} and spread == {"a": 2.0, "b": 6.0}


def test_emit_appends_one_line_per_record(tmp_path, capsys):
    out = tmp_path / "record.jsonl"
    out.write_text("kept\n")
    bl.emit({"a": 1, "nested": {"b": [1, 2]}}, str(out))
    bl.emit([{"c": 2}, {"d": 3}], str(out))
    bl.emit({"e": 4})                                         # no file named: printed only
    lines = out.read_text().split("\n")
    assert lines[0] == "kept" and lines[-1] == "" and len(lines) == 5
    assert [json.loads(x) for x in lines[1:4]] == [{"a": 1, "nested": {"b": [1, 2]}}, {"c": 2}, {"d": 3}]
    printed = capsys.readouterr().out.splitlines()
    assert printed == lines[1:4] + [json.dumps({"e": 4})]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["record.jsonl"]


@pytest.mark.parametrize("name", TOOLS)
def test_help_exits_0(name):
    """(The imports of torch and of the library stay inside main(), behind the argument parser.)"""
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name + "_bench.py"), "--help"],
                         capture_output=True, text=True, cwd=ROOT)
    assert got.returncode == 0, got.stderr
    assert "--config" in got.stdout
