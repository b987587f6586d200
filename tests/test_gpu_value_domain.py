"""-m gpu: the kernel against the CPU oracle on data values at the edges of their domains
(tests/common.py VALUE_CASES: NaN / inf / subnormal / negative densities and coefficients, sigmoid
arguments in exp's subnormal band and beyond its clamp, RGBA colours outside [0, 1], SG / ASG lobes
with NaN / inf / 0 / huge lambda, options outside [0, 1]) and on fog (tests/common.py FOG_CASES:
every sample of ~90 per ray a hit, so the deferred shading runs under full pressure), every flavour:
FAST (SH1-25, RGBA), FULL (SG / ASG, depth mode, access counters), GENERIC (N = 3, a 26-level N = 2
chain), the probe overlay and vr_probe_coeffs.

The comparator is NaN-aware (tests/common.py assert_same_values): RGBA8 bytes equal, fp32 words
bit-equal or NaN in both, the NaNs in the same places."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests.common import assert_same_values, gpu_frame, ob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def counted_frame(torch, tree, tr, w, h, f, fp_mode=0, **kw):
    """Kernel frame through the instrumented flavour -> (rgba, accum, counters dict)."""
    from volrend_amd import _abi, api
    t = api.N3Tree.from_synth(tree)
    cam = api.Camera(w, h, f, f)
    cam.transform = np.asarray(tr, np.float32)
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    counters = torch.zeros(7, dtype=torch.int64, device="cuda")
    api.launch_renderer(t, cam, api.RenderOptions(**kw), img, None, None, True, accum=acc,
                        counters=counters, fp_mode=fp_mode)
    torch.cuda.synchronize()
    assert t.status() == 0
    t.free_device()
    return img.cpu().numpy(), acc.cpu().numpy(), dict(zip(_abi.COUNTER_FIELDS, [int(v) for v in counters.cpu().tolist()]))


@pytest.mark.parametrize("fp_mode", [0, 1])
@pytest.mark.parametrize("case", list(common.VALUE_CASES))
def test_special_values_match_oracle(torch_cuda, case, fp_mode):
    tree, tr, w, h, f, kw = common.value_case(case)
    rgba_o, acc_o, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode, **kw)
    assert np.isfinite(acc_o).any() and (np.isnan(acc_o).any() or kw.get("render_depth"))
    rgba_g, acc_g = gpu_frame(torch_cuda, tree, tr, w, h, f, fp_mode, **kw)
    assert_same_values(rgba_g, acc_g, rgba_o, acc_o, f"{case} fp_mode={fp_mode}")


@pytest.mark.parametrize("case", ["SH16", "RGBA", "SG7", "ASG4", "SH4_negative_thresh", "SH16_stop_ge_1",
                                  "SH16_depth"])
def test_special_values_access_counters(torch_cuda, case):
    """The instrumented flavour on special values: counters equal the oracle's to the integer."""
    tree, tr, w, h, f, kw = common.value_case(case)
    rgba_o, acc_o, cnt_o = common.oracle_frame(tree, tr, w, h, f, **kw)
    rgba_g, acc_g, cnt_g = counted_frame(torch_cuda, tree, tr, w, h, f, **kw)
    assert cnt_g == cnt_o
    assert_same_values(rgba_g, acc_g, rgba_o, acc_o, case)


@pytest.mark.parametrize("fp_mode", [0, 1])
@pytest.mark.parametrize("kind", ["N3", "chain26"])
def test_special_values_generic_flavour(torch_cuda, kind, fp_mode):
    """The GENERIC flavour (float descent): an N = 3 tree and a 26-level N = 2 chain with special
    values in the leaves around the camera -- images, accumulators and counters."""
    if kind == "N3":
        tree = common.apply_value_edges(common.random_tree_general_n(3, 3, 4, "SH", seed=703), 704, frac=0.15)
        tr, w, h, f = common.camera_for(pose_idx=3, size=48)
        kw = {}
    else:
        tree, T = common.deep_chain_tree_n2(depth=26, basis_dim=4, seed=705)
        tree = common.apply_value_edges(tree, 706, frac=0.3)
        tr, w, h, f = common.camera_at(T)
        kw = dict(step_size=1e-8)
    rgba_o, acc_o, cnt_o = common.oracle_frame(tree, tr, w, h, f, fp_mode, **kw)
    assert np.isnan(acc_o).any() and np.isfinite(acc_o).any()
    rgba_g, acc_g, cnt_g = counted_frame(torch_cuda, tree, tr, w, h, f, fp_mode, **kw)
    assert cnt_g == cnt_o
    assert_same_values(rgba_g, acc_g, rgba_o, acc_o, kind)
    rgba_g, acc_g = gpu_frame(torch_cuda, tree, tr, w, h, f, fp_mode, **kw)   # uninstrumented
    assert_same_values(rgba_g, acc_g, rgba_o, acc_o, kind)


@pytest.mark.parametrize("fp_mode", [0, 1])
@pytest.mark.parametrize("fmt,bd", [("SH", 9), ("SH", 16), ("SG", 4)])
def test_special_values_probe(torch_cuda, fmt, bd, fp_mode):
    """Probe overlay and vr_probe_coeffs at a leaf that holds a non-finite coefficient."""
    from volrend_amd import _abi, api
    torch = torch_cuda
    tree = common.value_edge_tree(fmt, bd, seed=710 + bd)
    p = common.edge_probe_point(tree, seed=bd)
    tr, w, h, f = common.camera_for(pose_idx=5, size=48)
    kw = dict(enable_probe=1, probe=p, probe_disp_size=30, basis_minmax=(0, bd - 1))
    rgba_o, acc_o, _ = common.oracle_frame(tree, tr, w, h, f, fp_mode, **kw)
    rgba_g, acc_g = gpu_frame(torch, tree, tr, w, h, f, fp_mode, **kw)
    assert_same_values(rgba_g, acc_g, rgba_o, acc_o, "overlay")
    th = ob.TreeHandle(tree)
    n = tree.data_dim - 1
    want = np.zeros(n, np.float32)
    ob.lib().or_probe_coeffs(C.byref(th.struct), C.byref(ob.default_options(**kw)), want.ctypes.data)
    assert not np.isfinite(want).all()
    t = api.N3Tree.from_synth(tree)
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    o = api.RenderOptions(enable_probe=True, probe=p).to_c()
    _abi.check(_abi.lib().vr_probe_coeffs(t.handle, C.byref(o), out.data_ptr(), None))
    torch.cuda.synchronize()
    t.free_device()
    got = out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])


@pytest.mark.parametrize("fp_mode", [0, 1])
@pytest.mark.parametrize("case", list(common.FOG_CASES))
def test_fog_bit_exact(torch_cuda, case, fp_mode):
    """Fog: every sample a hit for the whole ray (SH16: the staged-LDS path, SG7: the runtime basis)."""
    tree, tr, w, h, f, kw = common.fog_case(case)
    rgba_o, acc_o, cnt = common.oracle_frame(tree, tr, w, h, f, fp_mode, **kw)
    assert cnt["hit_samples"] > 80 * cnt["rays"] and cnt["early_stops"] == 0
    rgba_g, acc_g = gpu_frame(torch_cuda, tree, tr, w, h, f, fp_mode, **kw)
    common.assert_same_values(rgba_g, acc_g, rgba_o, acc_o, case)
    assert np.array_equal(acc_g.view(np.uint32), acc_o.view(np.uint32))


FOG_TUNINGS = [dict(refill_min=1), dict(refill_min=64), dict(drain_flush=0), dict(drain_flush=64),
               dict(march_max=1), dict(march_max=12), dict(frame_group=1), dict(frame_group=2, super_block=4),
               dict(xcd_queues=0), dict(xcd_queues=1), dict(raygen_waves=1), dict(raygen_waves=4),
               dict(raygen_waves=16)]


def test_fog_scheduling_knobs(torch_cuda):
    """One fog scene, a batch of 3 poses and a 3-way tile shard, under every scheduling knob of
    vr_tree_set_tuning: output bit-identical to the default tuning and to the oracle, status 0."""
    torch = torch_cuda
    from volrend_amd import api, tiles
    tree, _, _, _, f, _ = common.fog_case("SH16")
    w, h = 61, 43
    trs = [common.camera_for(pose_idx=i, size=48)[0] for i in (0, 3, 6)]
    want = [common.oracle_frame(tree, tr, w, h, f)[0] for tr in trs]
    cam = api.Camera(w, h, f, f)
    world, tw, th = 3, 16, 8

    def render(tuning):
        t = api.N3Tree.from_synth(tree)
        t.set_tuning(**tuning)
        imgs = torch.zeros((3, h, w, 4), dtype=torch.uint8, device="cuda")
        api.launch_renderer_batch(t, cam, trs, api.RenderOptions(), [imgs[i] for i in range(3)], None, True)
        parts = []
        for rank in range(world):
            shard = api.TileShard(tw, th, rank, world, compact=True)
            buf = torch.zeros((3, api.compact_bytes(w, h, shard)), dtype=torch.uint8, device="cuda")
            api.launch_renderer_batch(t, cam, trs, api.RenderOptions(), [buf[i] for i in range(3)], None, True,
                                      shard=shard)
            parts.append(buf)
        torch.cuda.synchronize()
        status = t.status()
        t.free_device()
        sharded = [tiles.assemble_tiles(np.stack([parts[r][i].cpu().numpy().reshape(-1, 4) for r in range(world)]),
                                        w, h, tw, th, world) for i in range(3)]
        return imgs.cpu().numpy(), sharded, status

    base, base_sh, st = render({})
    assert st == 0
    for i in range(3):
        assert np.array_equal(base[i], want[i]), ("default tuning", i)
        assert np.array_equal(base_sh[i], want[i]), ("default tuning, sharded", i)
    for tuning in FOG_TUNINGS:
        got, got_sh, st = render(tuning)
        assert st == 0, tuning
        for i in range(3):
            assert np.array_equal(got[i], base[i]), (tuning, i)
            assert np.array_equal(got_sh[i], base[i]), (tuning, "sharded", i)
