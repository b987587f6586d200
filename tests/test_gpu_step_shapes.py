"""vr_tree_step over every record shape and over the bitmaps a marked backward never happens to make.

The step lays a wave's lanes across a record, and the record length picks the layout: several slots per wave
instruction with the remainder lanes idle (2 * data_dim <= 64), one slot per instruction (up to 64), or a slot
walked in 64-lane chunks with sigma in the last one.  The scenes here stand at data_dim 4, 10, 13, 22, 28, 31, 34,
49, 64, 67 and 76 (tests/update_util.py): sixteen, six, four and two slots per instruction, both edges of the
one-slot form, and the chunked form with three and with twelve lanes in its second chunk.  The bitmaps and gradients
are made up -- the marked backward refuses SG / ASG, and the step does not care where its bits came from.

Everything is bit-exact: the expected side is the numpy binary32 restatement (tests/step_util.py) and
update_util.stored(step_util.mixture(...)).  That the tree is a fresh upload's for these shapes:
tests/test_gpu_step.py::test_the_tree_is_a_fresh_uploads.

Not covered: the second trip of the kernel's grid-stride loop over 2048-slot groups.  It needs more groups than
16 workgroups per CU times four waves, about 33 million slots on an MI355X -- larger than the benchmark's tree and
far beyond a test of a few seconds."""
import numpy as np
import pytest

from tests import step_util as su
from tests import update_util as uu
from tests.update_util import upload

pytestmark = pytest.mark.gpu
LR, LR_SIGMA = 0.5, 3.0      # (both exact in binary32; large enough to move binary16 values)
ADAM = dict(lr=0.05, lr_sigma=0.5, betas=(0.9, 0.999), eps=1e-8)
SHAPES = ["rgba", "basis1", "n3", "asg7", "sh9", "sg10", "sg11", "sh16", "sg21", "sg22", "sh25"]
PATTERN_SCENES = ["rgba", "basis1", "sh9", "sh16", "sh25"]   # 16, 6, 2 and 1 slots per instruction, and two chunks


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def n_slots(tree):
    return tree.capacity * tree.N ** 3


def gradients(rng, shape):
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 0, shape)).astype(np.float32)


@pytest.mark.parametrize("name", SHAPES)
def test_sgd_and_adam_are_the_restatement(torch_cuda, name):
    """One SGD call, then Adam steps 1 and 2 (the second mask another draw), on one upload; after each call the five
    arrays and the read-back are the restatement's."""
    torch = torch_cuda
    tree = uu.case(name)["tree"]
    slots, dd, shape = n_slots(tree), tree.data_dim, tree.data.shape
    rng = np.random.default_rng(300 + dd)
    extra0 = None if tree.extra is None else np.array(tree.extra, copy=True)
    t = upload(name)
    try:
        old16 = t.read_data().cpu().numpy()
        state = dict(master=t.read_data(dtype=torch.float32).cpu().numpy(), m=np.zeros(shape, np.float32),
                     v=np.zeros(shape, np.float32))
        assert np.array_equal(old16.view(np.uint16), uu.stored(tree, tree.data).view(np.uint16))
        calls = [("sgd", dict(lr=LR, lr_sigma=LR_SIGMA)), ("adam", dict(step=1, **ADAM)), ("adam", dict(step=2, **ADAM))]
        for kind, kw in calls:
            mask = rng.random(slots) < 0.4
            assert 50 < mask.sum() < slots
            host = dict(state, grad=gradients(rng, shape))
            want = su.restate(kind, host["master"], host["grad"], mask, m=host["m"] if kind == "adam" else None,
                              v=host["v"] if kind == "adam" else None, **kw)
            got = su.device_call(torch, t, kind, host, mask, su.pack_bits(mask), **kw)
            expected16 = uu.stored(tree, su.mixture(old16, want["master"], mask))
            what = f"{name} {kind} {kw.get('step', '')}"
            if dd > 64:   # name the chunk first
                for key in ("master", "m", "v"):
                    if want[key] is not None:
                        w = want[key] if key == "master" else su.with_sentinel(want[key], mask)
                        bad = su.chunk_mismatches(got[key], w)
                        assert not any(bad.values()), (what, key, bad)
                bad = su.chunk_mismatches(got["read"], expected16)
                assert not any(bad.values()), (what, "tree", bad)
            su.assert_call(got, want, mask, expected16, what)
            assert not np.array_equal(got["master"], host["master"]), "the step moved nothing"
            assert not np.array_equal(got["read"].view(np.uint16), old16.view(np.uint16))
            old16 = expected16
            state = {k: want[k] if want[k] is not None else state[k] for k in ("master", "m", "v")}
        assert t.status() == 0
    finally:
        t.free_device()
    assert extra0 is None or np.array_equal(np.asarray(tree.extra), extra0)


@pytest.mark.parametrize("name", PATTERN_SCENES)
def test_bitmap_patterns(torch_cuda, name):
    """One SGD step per pattern of step_util.bitmap_patterns, all on one upload, each compared when it is done."""
    torch = torch_cuda
    tree = uu.case(name)["tree"]
    slots, shape = n_slots(tree), tree.data.shape
    rng = np.random.default_rng(17)
    kw = dict(lr=LR, lr_sigma=LR_SIGMA)
    t = upload(name)
    try:
        old16 = t.read_data().cpu().numpy()
        master = t.read_data(dtype=torch.float32).cpu().numpy()
        for label, words, groups in su.bitmap_patterns(slots):
            mask = su.unpack_bits(words, slots)
            for g in groups:
                assert mask[g * su.GROUP:(g + 1) * su.GROUP].any(), (label, g)
            host = dict(master=master, grad=rng.standard_normal(shape).astype(np.float32))
            want = su.restate("sgd", master, host["grad"], mask, **kw)
            got = su.device_call(torch, t, "sgd", host, mask, words, **kw)
            expected16 = uu.stored(tree, su.mixture(old16, want["master"], mask))
            su.assert_call(got, want, mask, expected16, f"{name}, {label}")
            assert not np.array_equal(got["master"], master), (label, "the step moved nothing")
            old16, master = expected16, want["master"]
        assert t.status() == 0
    finally:
        t.free_device()
