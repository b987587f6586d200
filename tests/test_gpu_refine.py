"""-m gpu: vr_refine_plan / vr_refine_apply against the numpy restatement of tests/refine_util.py, bit for bit: the
raw C calls over trees, selections and array sets (every output sized exactly, poisoned beforehand, with a guard band
behind it that must keep its bits), then through the library -- the refined tree uploaded from device memory renders,
answers point queries and optimises as a host upload of the restated arrays does."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import common, query_util
from tests import refine_util as ru
from tests import update_util as uu
from volrend_amd import _abi

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 512


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


# name -> (child [capacity, N^3], N, data_dim)
@functools.lru_cache(maxsize=None)
def tree_of(name):
    if name.startswith("n2_dd"):                 # N = 2, records of 4, 28 and 49 (odd: 98 bytes) elements
        dd = int(name[5:])
        t = common.small_scene(depth=4, basis_dim=(dd - 1) // 3, seed=40 + dd)
    elif name == "n4_dd4":
        t = common.random_tree_general_n(N=4, depth=3, basis_dim=1, seed=2)
    elif name == "n3_ragged":                    # 27 * capacity slots: the last mask word is partial
        t = common.random_tree_general_n(N=3, depth=3, basis_dim=1, seed=9)
        assert (t.capacity * 27) % 32 != 0
    elif name == "full6":                        # 8^6 leaf slots, 9,363 mask words: the scan spans several blocks
        return ru.full_tree_n2(5), 2, 4
    child = common.rows_of(t).astype(np.int32)
    assert t.data_dim == (int(name[5:]) if name.startswith("n2_dd") else 4)
    return child, t.N, t.data_dim


class Guarded:
    """A device buffer of exactly ``nbytes`` bytes, poisoned, with a poisoned guard band behind it."""

    def __init__(self, torch, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.ptr = self.raw.data_ptr()

    def bits(self, dtype):
        host = self.raw.cpu().numpy()
        assert (host[self.nbytes:] == POISON).all(), "a store went beyond the end of an output"
        return host[:self.nbytes].view(dtype)


def run(torch, child, N, sel_words, arrays, want_src_slot=True, n_new_override=None):
    """plan + apply on the null stream -> (n_new, child_out [cap + n_new, N^3], src_slot or None, list of dst)."""
    L = _abi.lib()
    cap, N3 = child.shape
    child_dev = torch.from_numpy(child.copy()).cuda()
    sel_dev = torch.from_numpy(np.ascontiguousarray(sel_words).view(np.int32).copy()).cuda()
    srcs = [torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.itemsize == 2 else np.int32).copy()).cuda()
            for a, _ in arrays]
    ws = torch.full((int(L.vr_refine_workspace(N, cap)),), POISON, dtype=torch.uint8, device="cuda")
    r = _abi.VrRefine()
    r.child, r.sel, r.workspace, r.workspace_bytes = child_dev.data_ptr(), sel_dev.data_ptr(), ws.data_ptr(), ws.numel()
    r.capacity, r.N = cap, N
    n_new = C.c_int64(-1)
    _abi.check(L.vr_refine_plan(C.byref(r), C.byref(n_new), None))
    n_new = int(n_new.value)
    child_out = Guarded(torch, (cap + n_new) * N3 * 4)
    src_slot = Guarded(torch, n_new * 4)
    dsts = [Guarded(torch, (cap + n_new) * N3 * a.shape[1] * a.itemsize) for a, _ in arrays]
    c_arrays = (_abi.VrRefineArray * max(len(arrays), 1))()
    for ca, (a, fill), s, d in zip(c_arrays, arrays, srcs, dsts):
        ca.src, ca.dst, ca.elem_bytes, ca.dim, ca.fill = s.data_ptr(), d.ptr, a.itemsize, a.shape[1], fill
    r.child_out, r.src_slot = child_out.ptr, src_slot.ptr if want_src_slot else None
    r.arrays, r.n_arrays = (c_arrays, len(arrays)) if arrays else (None, 0)
    r.n_new = n_new if n_new_override is None else n_new_override
    _abi.check(L.vr_refine_apply(C.byref(r), None))
    torch.cuda.synchronize()
    slots = src_slot.bits(np.int32)
    if not want_src_slot:
        assert (slots.view(np.uint8) == POISON).all()
    return (n_new, child_out.bits(np.int32).reshape(-1, N3), slots if want_src_slot else None,
            [d.bits(a.dtype).reshape(-1, a.shape[1]) for d, (a, _) in zip(dsts, arrays)])


def check_against_restatement(torch, name, sel, sel_words=None, **kw):
    child, N, dd = tree_of(name)
    arrays = ru.companions(child.size, dd, seed=len(name))
    want_child, want_slots, want_dsts = ru.restate(child, sel, arrays)
    n_new, got_child, got_slots, got_dsts = run(torch, child, N, ru.pack_bits(sel) if sel_words is None else sel_words,
                                                arrays, **kw)
    assert n_new == want_slots.size
    assert np.array_equal(got_child, want_child)
    if got_slots is not None:
        assert np.array_equal(got_slots, want_slots)
    for i, (g, w) in enumerate(zip(got_dsts, want_dsts)):
        assert g.shape == w.shape and np.array_equal(g, w), f"array {i}"
    return n_new


SMALL = ["n2_dd4", "n3_ragged"]
CASES = [(t, s) for t in SMALL for s in ("empty", "all_leaves", "random30", "internal_only", "last_bit")]
CASES += [(t, "random30") for t in ("n2_dd28", "n2_dd49", "n4_dd4", "full6")] + [("n2_dd49", "all_leaves"),
                                                                                  ("full6", "all_leaves")]


@pytest.mark.parametrize("name,sel_name", CASES, ids=[f"{t}-{s}" for t, s in CASES])
def test_outputs_are_the_restatement(torch_cuda, name, sel_name):
    child = tree_of(name)[0]
    sel = ru.selections(child, seed=1)[sel_name]
    n_new = check_against_restatement(torch_cuda, name, sel)
    if sel_name in ("empty", "internal_only"):
        assert n_new == 0                        # (and the outputs equal the inputs: that is the restatement)
    else:
        assert n_new > 0


@pytest.mark.parametrize("name", SMALL)
def test_junk_bits_beyond_the_end_are_ignored(torch_cuda, name):
    child = tree_of(name)[0]
    sel = ru.selections(child, seed=2)["random30"]
    check_against_restatement(torch_cuda, name, sel, sel_words=ru.pack_bits(sel, extra_words=3, junk=1))


def test_no_arrays_and_no_src_slot(torch_cuda):
    child, N, _ = tree_of("n2_dd28")
    sel = ru.selections(child, seed=3)["random30"]
    want_child, want_slots, _ = ru.restate(child, sel)
    n_new, got_child, got_slots, dsts = run(torch_cuda, child, N, ru.pack_bits(sel), [], want_src_slot=False)
    assert n_new == want_slots.size > 0 and got_slots is None and dsts == []
    assert np.array_equal(got_child, want_child)
    check_against_restatement(torch_cuda, "n2_dd28", sel, want_src_slot=False)


def test_a_smaller_n_new_than_planned_stays_inside_its_outputs(torch_cuda):
    """apply told fewer new nodes than plan counted (a caller's mistake): ranks at or beyond n_new write nothing --
    every output is sized for the SMALLER count and its guard band keeps its bits."""
    child, N, dd = tree_of("n2_dd49")
    sel = ru.selections(child, seed=4)["random30"]
    arrays = ru.companions(child.size, dd)
    n_planned = ru.restate(child, sel)[1].size
    L = _abi.lib()
    torch = torch_cuda
    cap, N3 = child.shape
    child_dev = torch.from_numpy(child.copy()).cuda()
    sel_dev = torch.from_numpy(ru.pack_bits(sel).view(np.int32).copy()).cuda()
    ws = torch.empty(int(L.vr_refine_workspace(N, cap)), dtype=torch.uint8, device="cuda")
    r = _abi.VrRefine()
    r.child, r.sel, r.workspace, r.workspace_bytes = child_dev.data_ptr(), sel_dev.data_ptr(), ws.data_ptr(), ws.numel()
    r.capacity, r.N = cap, N
    n_new = C.c_int64(-1)
    _abi.check(L.vr_refine_plan(C.byref(r), C.byref(n_new), None))
    assert n_new.value == n_planned > 10
    told = n_planned // 2
    a, fill = arrays[0]
    src = torch.from_numpy(a.view(np.int16).copy()).cuda()
    child_out, src_slot = Guarded(torch, (cap + told) * N3 * 4), Guarded(torch, told * 4)
    dst = Guarded(torch, (cap + told) * N3 * dd * 2)
    ca = (_abi.VrRefineArray * 1)()
    ca[0].src, ca[0].dst, ca[0].elem_bytes, ca[0].dim, ca[0].fill = src.data_ptr(), dst.ptr, 2, dd, fill
    r.child_out, r.src_slot, r.arrays, r.n_arrays, r.n_new = child_out.ptr, src_slot.ptr, ca, 1, told
    _abi.check(L.vr_refine_apply(C.byref(r), None))
    torch.cuda.synchronize()
    want_child, want_slots, (want_dst,) = ru.restate(child, sel, [arrays[0]])
    assert np.array_equal(src_slot.bits(np.int32), want_slots[:told])          # (the guards are checked in bits())
    assert np.array_equal(dst.bits(np.uint16).reshape(-1, dd), want_dst[:(cap + told) * N3])
    got_child = child_out.bits(np.int32).reshape(-1, N3)
    later = want_slots[told:]                                                  # slots of the ranks that were cut off
    expect = want_child[:cap + told].copy()
    expect.reshape(-1)[later] = 0                                              # they stay the leaves they were
    assert np.array_equal(got_child, expect)


# ---- through the library ----
def frames(torch, t, fp_mode, size=32):
    from volrend_amd import api
    tr, w, h, f = common.camera_for(size=size)
    cam = api.Camera(w, h, f, f)
    cam.transform = np.asarray(tr, np.float32)
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    api.launch_renderer(t, cam, api.RenderOptions(), img, None, torch.cuda.current_stream(), True, accum=acc,
                        fp_mode=fp_mode)
    torch.cuda.synchronize()
    return img.cpu().numpy(), acc.cpu().numpy()


@pytest.mark.parametrize("as_bitmap", [False, True])
def test_the_refined_tree_is_the_host_upload_of_the_restated_arrays(torch_cuda, as_bitmap):
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=4, basis_dim=9, seed=77)
    N3, cap = 8, tree.capacity
    sel = ru.selections(common.rows_of(tree), seed=6)["random30"]
    want, want_slots = ru.refined_synth(tree, sel)
    t = api.N3Tree.from_synth(tree)
    weights = torch.from_numpy(np.random.default_rng(3).random((cap, 2, 2, 2), np.float32)).cuda()
    try:
        sel_dev = torch.from_numpy(ru.pack_bits(sel).view(np.int32).copy() if as_bitmap else sel).cuda()
        res = t.refine(sel_dev, [(weights, "zero")], stream=torch.cuda.current_stream())
        new = res["tree"]
        try:
            assert res["n_new"] == want_slots.size > 0 and new.capacity == cap + res["n_new"]
            assert np.array_equal(res["src_slot"].cpu().numpy(), want_slots)
            assert np.array_equal(new.child_.reshape(-1, N3), common.rows_of(want))
            assert new.data_ is None and new.info()["capacity"] == want.capacity
            assert new.data_format == t.data_format and np.array_equal(new.scale, t.scale)
            w_new = res["companions"][0].cpu().numpy()
            assert w_new.shape == (want.capacity, 2, 2, 2) and not w_new[cap:].any()
            assert np.array_equal(w_new[:cap], weights.cpu().numpy())
            # the values the device holds: those of the restated file, the sigma of internal slots +0 (read_data's rule)
            assert np.array_equal(new.read_data().cpu().numpy().view(np.uint16), uu.stored(want, want.data).view(np.uint16))
            host = api.N3Tree.from_synth(want)
            try:
                for fp_mode in (0, 1):
                    rgba_o, acc_o, _ = common.oracle_frame(want, *common.camera_for(size=32), fp_mode=fp_mode)
                    rgba_g, acc_g = frames(torch, new, fp_mode)
                    rgba_h, acc_h = frames(torch, host, fp_mode)
                    assert acc_o.any()
                    assert np.array_equal(rgba_g, rgba_o) and np.array_equal(acc_g.view(np.uint32), acc_o.view(np.uint32))
                    assert np.array_equal(rgba_g, rgba_h) and np.array_equal(acc_g.view(np.uint32), acc_h.view(np.uint32))
            finally:
                host.free_device()
            # point queries: one level deeper inside refined leaves, the record unchanged
            pts = np.random.default_rng(8).random((2000, 3), np.float32)
            q_old = t.query(torch.from_numpy(pts).cuda(), want=("depth", "coeffs", "sigma"), space="tree")
            q_new = new.query(torch.from_numpy(pts).cuda(), want=("depth", "coeffs", "sigma"), space="tree")
            from oracle import binding as ob
            hit = np.isin(query_util.oracle_query(ob.TreeHandle(tree), pts)["leaf"], want_slots)
            assert 50 < hit.sum() < pts.shape[0] - 50
            d_old, d_new = q_old["depth"].cpu().numpy(), q_new["depth"].cpu().numpy()
            assert np.array_equal(d_new, d_old + hit)
            for k in ("coeffs", "sigma"):
                assert np.array_equal(q_new[k].cpu().numpy().view(np.uint32), q_old[k].cpu().numpy().view(np.uint32)), k
            assert new.status() == 0 and t.status() == 0
        finally:
            new.free_device()
    finally:
        t.free_device()


def test_optimizer_refine(torch_cuda):
    """SparseTreeOptimizer("adam").refine(sel) after two steps: master / m / v are the restatement of what they
    were, grad / touched are zero; a following fit + step runs, and the tree then holds what update_data(master)
    puts into a fresh upload of the refined arrays."""
    torch = torch_cuda
    from volrend_amd import api, optim
    name = "sh9"
    c = uu.case(name)
    tree = c["tree"]
    N3, cap, dd = 8, tree.capacity, tree.data_dim
    from tests import rays_util
    parts = [rays_util.rays_of_camera(tr, c["w"], c["h"], c["f"]) for tr in c["trs"]]
    o = uu.dev(torch, np.concatenate([p[0] for p in parts]))
    d = uu.dev(torch, np.concatenate([p[1] for p in parts]))
    target = torch.full((o.shape[0], 3), 0.25, dtype=torch.float32, device="cuda")
    t = uu.upload(name)
    fresh = None
    try:
        opt = optim.SparseTreeOptimizer(t, "adam", lr=0.02, lr_sigma=0.3)
        for _ in range(2):
            opt.fit(o, d, target)
            opt.step()
        torch.cuda.synchronize()
        before = {k: getattr(opt, k).cpu().numpy().reshape(-1, dd) for k in ("master", "m", "v")}
        assert before["m"].any() and before["v"].any()
        sel = ru.selections(common.rows_of(tree), seed=12)["random30"]
        src_slot = opt.refine(torch.from_numpy(sel).cuda())
        torch.cuda.synchronize()
        assert opt.tree is not t
        want_child, want_slots, (w_master, w_m, w_v) = ru.restate(
            common.rows_of(tree), sel, [(before["master"], ru.COPY), (before["m"], ru.ZERO), (before["v"], ru.ZERO)])
        n_new = want_slots.size
        assert n_new > 0 and np.array_equal(src_slot.cpu().numpy(), want_slots)
        for key, w in (("master", w_master), ("m", w_m), ("v", w_v)):
            got = getattr(opt, key)
            assert tuple(got.shape) == (cap + n_new, 2, 2, 2, dd), key
            assert np.array_equal(got.cpu().numpy().reshape(-1, dd).view(np.uint32), w.view(np.uint32)), key
        assert tuple(opt.grad.shape) == tuple(opt.master.shape) and not bool(opt.grad.any())
        assert opt.touched.numel() == ((cap + n_new) * N3 + 31) // 32 and not bool(opt.touched.any())
        assert np.array_equal(opt.tree.child_.reshape(-1, N3), want_child)

        sq = opt.fit(o, d, target)
        opt.step()
        torch.cuda.synchronize()
        assert opt.tree.status() == 0 and opt.steps == 3 and bool(torch.isfinite(sq).all())
        assert not bool(opt.grad.any()) and not bool(opt.touched.any())
        master = opt.master.cpu().numpy()
        assert not np.array_equal(master.reshape(-1, dd).view(np.uint32), w_master.view(np.uint32))   # (it moved)
        # the tree holds binary16(master) in every slot -- the step rounded the touched ones in, the others' master is
        # the widening of what they hold -- so a fresh upload of the refined child array that takes its values from
        # update_data(master) is the same tree: the same values, the same frame
        refined_child = want_child.reshape(cap + n_new, 2, 2, 2)
        fresh = api.N3Tree.from_arrays(refined_child, np.zeros(master.shape, np.float16), tree.offset, tree.invradius3,
                                       tree.data_format, tree.extra)
        fresh.update_data(opt.master)
        assert np.array_equal(opt.tree.read_data().cpu().numpy().view(np.uint16),
                              fresh.read_data().cpu().numpy().view(np.uint16))
        (rgba_a, acc_a), (rgba_b, acc_b) = frames(torch, opt.tree, 0), frames(torch, fresh, 0)
        assert acc_a.any() and np.array_equal(rgba_a, rgba_b) and np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    finally:
        t.free_device()
        if fresh is not None:
            fresh.free_device()
