"""The scheduling rules of a march launch (plan_launch, volrend_amd/csrc/vr_launch_plan.cpp) on their own: which
chunk cap, block order, ray-generation workgroup, record hint, frame group and queue count a launch of a kind and
size gets.  None of them changes a pixel or a gradient, so no parity test sees one move.
tests/cpp/launch_plan_check.cpp is built with plain g++ against that one source -- no HIP, no library -- and
answers every query of this module in one run."""
import subprocess

import pytest

from tests import build_util

KINDS = ("colour", "aov", "weights", "backward")
COLOUR, GUIDED = ("colour", "aov"), ("weights", "backward")
MIB = 1 << 20
FIELDS = ("chunk_max", "super_block", "raygen_waves", "records_nt", "frame_group", "n_queues")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.csrc_program("launch_plan_check", "vr_launch_plan", tmp_path_factory.mktemp("bin"))


def plans(exe, queries):
    """queries: (kind, source, n_frames, list_rays, lookup_bytes, {knob: value}) -> one dict of FIELDS each."""
    text = "".join(" ".join(map(str, q[:5])) + "".join(f" {k}={v}" for k, v in q[5].items()) + "\n" for q in queries)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(queries)
    return [dict(zip(FIELDS, map(int, line.split()))) for line in out]


def frames(kind, n_frames, lookup=0, **knobs):
    return (kind, "frames", n_frames, 0, lookup, knobs)


def rays(kind, n, lookup=0, **knobs):
    return (kind, "list", 1, n, lookup, knobs)         # a list is one pseudo-frame


def check(exe, field, cases):
    """cases: (query, expected value of `field`)."""
    got = plans(exe, [q for q, _ in cases])
    for (q, want), g in zip(cases, got):
        assert g[field] == want, (field, q, g)


def test_chunk_max(exe):
    cases = []
    for shape in (lambda k, **kw: frames(k, 1, **kw), lambda k, **kw: frames(k, 64, **kw),
                  lambda k, **kw: rays(k, 300, **kw), lambda k, **kw: rays(k, 5_000_000, **kw)):
        cases += [(shape(k), 256) for k in COLOUR]
        cases += [(shape(k), 4096) for k in GUIDED]
        cases += [(shape(k, chunk_max=v), v) for k in KINDS for v in (64, 1024, 8192)]
    check(exe, "chunk_max", cases)


def test_super_block(exe):
    cases = []
    for k in COLOUR:
        cases += [(frames(k, 1), 1), (frames(k, 2), 1), (frames(k, 3), 4), (frames(k, 64), 4), (frames(k, 512), 4)]
    for k in GUIDED:
        cases += [(frames(k, n), 1) for n in (1, 2, 3, 64, 512)]
    for k in KINDS:
        cases += [(rays(k, n), 1) for n in (1, 300, 5_000_000)]
        cases += [(frames(k, n, super_block=v), v) for n in (1, 64) for v in (1, 2, 8)]
        cases += [(rays(k, 300, super_block=2), 2)]
    check(exe, "super_block", cases)


def test_raygen_waves_of_frames(exe):
    cases = []
    for k in KINDS:
        cases += [(frames(k, 1), 4), (frames(k, 2), 4), (frames(k, 3), 16), (frames(k, 4), 16), (frames(k, 512), 16)]
        cases += [(frames(k, n, raygen_waves=v), v) for n in (1, 64) for v in (1, 4, 15, 16, 64)]   # as it is
    check(exe, "raygen_waves", cases)


def test_raygen_waves_of_a_list(exe):
    cases = []
    for k in KINDS:
        cases += [(rays(k, 1), 4), (rays(k, 300), 4), (rays(k, 1_280_000), 4), (rays(k, 1_280_001), 16),
                  (rays(k, (1 << 30) - 1), 16)]
        for n in (300, 5_000_000):                           # list ray generation has no one-wave flavour
            cases += [(rays(k, n, raygen_waves=v), 4) for v in (1, 4, 15)]
            cases += [(rays(k, n, raygen_waves=v), 16) for v in (16, 64)]
    check(exe, "raygen_waves", cases)


def test_records_nt(exe):
    cases = []
    for shape in (lambda k, **kw: frames(k, 64, **kw), lambda k, **kw: rays(k, 300, **kw)):
        for k in KINDS:
            cases += [(shape(k, lookup=0), 0), (shape(k, lookup=128 * MIB), 0), (shape(k, lookup=128 * MIB + 1), 1),
                      (shape(k, lookup=5 << 30), 1)]          # (beyond 32 bits)
            cases += [(shape(k, lookup=b, records_nt=v), v) for b in (0, 128 * MIB + 1) for v in (0, 1)]
    check(exe, "records_nt", cases)


def test_frame_group(exe):
    cases = []
    for k in KINDS:
        for n in (1, 5, 64):
            cases += [(frames(k, n), n), (frames(k, n, frame_group=0), n), (frames(k, n, frame_group=-1), n),
                      (frames(k, n, frame_group=n + 1), n), (frames(k, n, frame_group=n), n),
                      (frames(k, n, frame_group=1), 1)]
        cases += [(frames(k, 64, frame_group=8), 8), (frames(k, 64, frame_group=63), 63)]
        cases += [(rays(k, 300), 1), (rays(k, 300, frame_group=4), 1)]
    check(exe, "frame_group", cases)


def test_n_queues(exe):
    cases = []
    for k in KINDS:
        cases += [(frames(k, 64), 8), (frames(k, 64, xcd_queues=1), 8), (frames(k, 64, xcd_queues=0), 1),
                  (rays(k, 300), 8), (rays(k, 300, xcd_queues=0), 1)]
    check(exe, "n_queues", cases)


def test_one_knob_moves_one_rule(exe):
    """A forced knob leaves the other rules on auto."""
    base = plans(exe, [frames("colour", 64)])[0]
    assert base == dict(chunk_max=256, super_block=4, raygen_waves=16, records_nt=0, frame_group=64, n_queues=8)
    forced = dict(chunk_max=1024, super_block=2, raygen_waves=4, records_nt=1, frame_group=8, n_queues=1)
    knob_of = dict(n_queues="xcd_queues")
    for field, v in forced.items():
        got = plans(exe, [frames("colour", 64, **{knob_of.get(field, field): 0 if field == "n_queues" else v})])[0]
        assert got == dict(base, **{field: v}), field
