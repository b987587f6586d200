"""-m gpu: vr_collapse_plan / vr_collapse_apply against the numpy restatement of tests/collapse_util.py, bit for bit:
the raw C calls over trees, selections and array sets (every output sized exactly, poisoned beforehand, with a guard
band behind it that must keep its bits), then through the library -- the collapsed tree uploaded from device memory
renders, answers point queries and optimises as a host upload of the restated arrays does."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import collapse_util as cu
from tests import common, query_util
from tests import refine_util as ru
from tests import update_util as uu
from volrend_amd import _abi

pytestmark = pytest.mark.gpu
POISON32 = np.frombuffer(bytes([cu.POISON] * 4), np.int32)[0]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


# name -> (child [capacity, N^3], N, data_dim, number of frontier nodes)
@functools.lru_cache(maxsize=None)
def tree_of(name):
    if name.startswith("n2_dd"):                 # N = 2, records of 4, 28 and 49 (odd: 98 bytes) elements
        dd = int(name[5:])
        t = common.small_scene(depth=4, basis_dim=(dd - 1) // 3, seed=40 + dd)
        assert (t.capacity, t.data_dim) == {4: (403, 4), 28: (479, 28), 49: (483, 49)}[dd]
    elif name == "n4_dd4":
        t = common.random_tree_general_n(N=4, depth=3, basis_dim=1, seed=2)
        assert t.capacity == 491
    elif name == "n3_ragged":                    # 68 nodes: the last collapse word is partial
        t = common.random_tree_general_n(N=3, depth=3, basis_dim=1, seed=9)
        assert t.capacity == 68
    elif name == "full6":                        # 299,593 nodes, 9,363 collapse words: the scan spans several blocks
        child = ru.full_tree_n2(6).astype(np.int32)
        assert child.shape[0] == 299593 and (child.shape[0] + 31) // 32 == 9363
        return child, 2, 1, int(cu.frontier(child).sum())
    child = common.rows_of(t).astype(np.int32)
    return child, t.N, t.data_dim, int(cu.frontier(child).sum())


def test_the_trees_are_the_ones_the_cases_were_chosen_for():
    assert [tree_of(f"n2_dd{dd}")[3] for dd in (4, 28, 49)] == [339, 407, 413]
    assert tree_of("full6")[3] == 8 ** 6


@functools.lru_cache(maxsize=None)
def arrays_of(name):
    child, _, dd, _ = tree_of(name)
    return cu.companions(child.size, dd, seed=len(name))


def run(torch, child, N, sel_words, arrays, maps=True, n_keep_told=None, misalign=False):
    """plan + apply on the null stream -> dict(n_keep, child_out [told, N^3], node_map, src_node, into_slot (None
    where not asked for), dsts).  Outputs are sized for the n_keep apply is TOLD.  misalign: every dst starts one
    element (2 or 4 bytes) behind a 16-byte boundary."""
    L = _abi.lib()
    cap, N3 = child.shape
    child_dev = torch.from_numpy(child.copy()).cuda()
    sel_dev = torch.from_numpy(np.ascontiguousarray(sel_words).view(np.int32).copy()).cuda()
    srcs = [torch.from_numpy(np.ascontiguousarray(a).view(np.int16 if a.itemsize == 2 else np.int32).copy()).cuda()
            for a, _ in arrays]
    ws = torch.full((int(L.vr_collapse_workspace(N, cap)),), cu.POISON, dtype=torch.uint8, device="cuda")
    r = _abi.VrCollapse()
    r.child, r.sel, r.workspace, r.workspace_bytes = child_dev.data_ptr(), sel_dev.data_ptr(), ws.data_ptr(), ws.numel()
    r.capacity, r.N = cap, N
    n_keep = C.c_int64(-1)
    _abi.check(L.vr_collapse_plan(C.byref(r), C.byref(n_keep), None))
    n_keep = int(n_keep.value)
    told = n_keep if n_keep_told is None else n_keep_told
    child_out = cu.Guarded(torch, told * N3 * 4)
    node_map, src_node, into_slot = cu.Guarded(torch, cap * 4), cu.Guarded(torch, told * 4), cu.Guarded(torch, cap * 4)
    dsts = [cu.Guarded(torch, told * N3 * a.shape[1] * a.itemsize, offset=a.itemsize if misalign else 0)
            for a, _ in arrays]
    c_arrays = (_abi.VrCollapseArray * max(len(arrays), 1))()
    for ca, (a, rule), s, d in zip(c_arrays, arrays, srcs, dsts):
        ca.src, ca.dst, ca.elem_bytes, ca.dim, ca.rule = s.data_ptr(), d.ptr, a.itemsize, a.shape[1], rule
    r.child_out = child_out.ptr
    if maps:
        r.node_map, r.src_node, r.into_slot = node_map.ptr, src_node.ptr, into_slot.ptr
    r.arrays, r.n_arrays = (c_arrays, len(arrays)) if arrays else (None, 0)
    r.n_keep = told
    _abi.check(L.vr_collapse_apply(C.byref(r), None))
    torch.cuda.synchronize()
    if not maps:                                  # the optional outputs were not passed: their buffers keep the poison
        assert node_map.untouched() and src_node.untouched() and into_slot.untouched()
    return dict(n_keep=n_keep, child_out=child_out.bits(np.int32).reshape(-1, N3),
                node_map=node_map.bits(np.int32) if maps else None, src_node=src_node.bits(np.int32) if maps else None,
                into_slot=into_slot.bits(np.int32) if maps else None,
                dsts=[d.bits(a.dtype).reshape(-1, a.shape[1]) for d, (a, _) in zip(dsts, arrays)])


def check_against_restatement(torch, name, sel, sel_words=None, arrays=None, **kw):
    child, N, dd, _ = tree_of(name)
    arrays = arrays_of(name) if arrays is None else arrays
    want = cu.restate(child, sel, arrays)
    got = run(torch, child, N, cu.pack_bits(sel) if sel_words is None else sel_words, arrays, **kw)
    assert got["n_keep"] == want["n_keep"]
    assert np.array_equal(got["child_out"], want["child_out"])
    for key in ("node_map", "src_node", "into_slot"):
        if got[key] is not None:
            assert np.array_equal(got[key], want[key]), key
    for i, (g, w, (_, rule)) in enumerate(zip(got["dsts"], want["dsts"], arrays)):
        cu.assert_array(g, w, rule, want["into_slot"], f"array {i}")
    return want


SMALL = ["n2_dd4", "n3_ragged"]
SELECTIONS = ("empty", "all", "random50", "non_frontier_only", "root_only", "last_node")
CASES = [(t, s) for t in SMALL for s in SELECTIONS]
CASES += [(t, "random50") for t in ("n2_dd28", "n2_dd49", "n4_dd4", "full6")] + [("n2_dd49", "all"), ("full6", "all")]


@pytest.mark.parametrize("name,sel_name", CASES, ids=[f"{t}-{s}" for t, s in CASES])
def test_outputs_are_the_restatement(torch_cuda, name, sel_name):
    child, _, _, n_frontier = tree_of(name)
    sel = cu.selections(child, seed=1)[sel_name]
    want = check_against_restatement(torch_cuda, name, sel)
    n_col = child.shape[0] - want["n_keep"]
    if sel_name in ("empty", "non_frontier_only", "root_only"):
        assert n_col == 0                        # (and the outputs equal the inputs: that is the restatement)
    elif sel_name == "all":
        assert n_col == n_frontier
    elif sel_name == "last_node":
        assert n_col == 1 and want["collapsed"][-1]
    else:
        assert 0 < n_col < n_frontier
    if n_col:                                    # every collapsed node of these trees has the one slot it goes into
        assert (want["into_slot"] >= 0).sum() == n_col


@pytest.mark.parametrize("name", ["n2_dd4", "n2_dd49", "n3_ragged"])
def test_outputs_that_start_off_a_16_byte_boundary(torch_cuda, name):
    child = tree_of(name)[0]
    check_against_restatement(torch_cuda, name, cu.selections(child, seed=5)["random50"], misalign=True)


@pytest.mark.parametrize("name", SMALL)
def test_junk_bits_beyond_the_end_are_ignored(torch_cuda, name):
    child = tree_of(name)[0]
    sel = cu.selections(child, seed=2)["random50"]
    check_against_restatement(torch_cuda, name, sel, sel_words=cu.pack_bits(sel, extra_words=3, junk=1))


def test_no_arrays_and_no_optional_outputs(torch_cuda):
    child = tree_of("n2_dd28")[0]
    sel = cu.selections(child, seed=3)["random50"]
    want = check_against_restatement(torch_cuda, "n2_dd28", sel, arrays=[], maps=False)
    assert want["n_keep"] < child.shape[0]
    check_against_restatement(torch_cuda, "n2_dd28", sel, maps=False)        # (ZERO / MEAN without the caller's into_slot)


def test_a_smaller_n_keep_than_planned_stays_inside_its_outputs(torch_cuda):
    """apply told fewer kept nodes than plan counted (a caller's mistake): new indices at or beyond n_keep write
    nothing -- every output is sized for the SMALLER count and its guard band keeps its bits."""
    child, N, dd, _ = tree_of("n2_dd49")
    N3 = child.shape[1]
    sel = cu.selections(child, seed=4)["random50"]
    arrays = arrays_of("n2_dd49")
    want = cu.restate(child, sel, arrays)
    told = want["n_keep"] // 6                        # (breadth-first numbering: the merged slots sit in early nodes)
    assert told > 10
    got = run(torch_cuda, child, N, cu.pack_bits(sel), arrays, n_keep_told=told)
    assert got["n_keep"] == want["n_keep"]
    assert np.array_equal(got["child_out"], want["child_out"][:told])
    assert np.array_equal(got["src_node"], want["src_node"][:told])
    cut = want["node_map"] >= told
    assert cut.any() and np.array_equal(got["node_map"], np.where(cut, POISON32, want["node_map"]))
    beyond = want["into_slot"] >= told * N3
    assert beyond.any() and np.array_equal(got["into_slot"], np.where(beyond, -1, want["into_slot"]))
    for i, (g, w, (_, rule)) in enumerate(zip(got["dsts"], want["dsts"], arrays)):
        cu.assert_array(g, w[:told * N3], rule, np.where(beyond, -1, want["into_slot"]), f"array {i}")


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
def test_the_collapsed_tree_is_the_host_upload_of_the_restated_arrays(torch_cuda, as_bitmap):
    torch = torch_cuda
    from volrend_amd import api
    tree = common.small_scene(depth=4, basis_dim=9, seed=77)
    N3, cap = 8, tree.capacity
    sel = cu.selections(common.rows_of(tree), seed=6)["random50"]
    held = uu.stored(tree, tree.data)                 # what read_data gives: the sigma of internal slots +0
    want, res = cu.collapsed_synth(tree, sel, cu.MEAN, data=held)
    t = api.N3Tree.from_synth(tree)
    hits = torch.from_numpy(np.random.default_rng(3).integers(1, 100, (cap, 2, 2, 2), dtype=np.int32)).cuda()
    try:
        sel_dev = torch.from_numpy(cu.pack_bits(sel).view(np.int32).copy() if as_bitmap else sel).cuda()
        out = t.collapse(sel_dev, [(hits, "zero")], stream=torch.cuda.current_stream())
        new = out["tree"]
        try:
            assert out["n_keep"] == res["n_keep"] < cap and new.capacity == res["n_keep"]
            for key in ("node_map", "src_node", "into_slot"):
                assert np.array_equal(out[key].cpu().numpy(), res[key]), key
            assert np.array_equal(new.child_.reshape(-1, N3), common.rows_of(want))
            assert new.data_ is None and new.info()["capacity"] == want.capacity
            assert new.data_format == t.data_format and np.array_equal(new.scale, t.scale)
            h_new = out["companions"][0].cpu().numpy()
            want_hits = cu.restate(common.rows_of(tree), sel, [(hits.cpu().numpy().reshape(-1, 1), cu.ZERO)])["dsts"][0]
            assert h_new.shape == (want.capacity, 2, 2, 2) and np.array_equal(h_new.reshape(-1, 1), want_hits)
            assert np.array_equal(new.read_data().cpu().numpy().view(np.uint16), uu.stored(want, want.data).view(np.uint16))
            pts = np.random.default_rng(8).random((2000, 3), np.float32)
            host = api.N3Tree.from_synth(want)
            try:
                for fp_mode in (0, 1):
                    rgba_o, acc_o, _ = common.oracle_frame(want, *common.camera_for(size=32), fp_mode=fp_mode)
                    rgba_g, acc_g = frames(torch, new, fp_mode)
                    rgba_h, acc_h = frames(torch, host, fp_mode)
                    assert acc_o.any()
                    assert np.array_equal(rgba_g, rgba_o) and np.array_equal(acc_g.view(np.uint32), acc_o.view(np.uint32))
                    assert np.array_equal(rgba_g, rgba_h) and np.array_equal(acc_g.view(np.uint32), acc_h.view(np.uint32))
                # point queries: one level higher inside collapsed nodes; everything as the host upload answers
                names = ("depth", "coeffs", "sigma")
                q_old = t.query(torch.from_numpy(pts).cuda(), want=names, space="tree")
                q_new = new.query(torch.from_numpy(pts).cuda(), want=names, space="tree")
                q_host = host.query(torch.from_numpy(pts).cuda(), want=names, space="tree")
                from oracle import binding as ob
                hit = res["collapsed"][query_util.oracle_query(ob.TreeHandle(tree), pts)["leaf"] // N3]
                assert 50 < hit.sum() < pts.shape[0] - 50
                assert np.array_equal(q_new["depth"].cpu().numpy(), q_old["depth"].cpu().numpy() - hit)
                for k in names:
                    assert np.array_equal(q_new[k].cpu().numpy().view(np.uint32), q_host[k].cpu().numpy().view(np.uint32)), k
                for k in ("coeffs", "sigma"):       # outside collapsed nodes the record is what it was
                    assert np.array_equal(q_new[k].cpu().numpy()[~hit].view(np.uint32),
                                          q_old[k].cpu().numpy()[~hit].view(np.uint32)), k
                assert new.status() == 0 and t.status() == 0 and host.status() == 0
            finally:
                host.free_device()
        finally:
            new.free_device()
    finally:
        t.free_device()


def test_optimizer_collapse(torch_cuda):
    """SparseTreeOptimizer("adam"): two steps, refine, collapse, then a further fit + step.  master / m / v are the
    restatement of what they were, grad / touched are zero and of the new size, and the tree is a fresh upload of the
    collapsed child array plus update_data(master) -- right after the collapse and after the further step."""
    torch = torch_cuda
    from volrend_amd import api, optim
    name = "sh9"
    c = uu.case(name)
    tree = c["tree"]
    N3, dd = 8, tree.data_dim
    from tests import rays_util
    parts = [rays_util.rays_of_camera(tr, c["w"], c["h"], c["f"]) for tr in c["trs"]]
    o = uu.dev(torch, np.concatenate([p[0] for p in parts]))
    d = uu.dev(torch, np.concatenate([p[1] for p in parts]))
    target = torch.full((o.shape[0], 3), 0.25, dtype=torch.float32, device="cuda")
    t = uu.upload(name)
    trees = [t]
    try:
        opt = optim.SparseTreeOptimizer(t, "adam", lr=0.02, lr_sigma=0.3)
        for _ in range(2):
            opt.fit(o, d, target)
            opt.step()
        opt.refine(torch.from_numpy(ru.selections(common.rows_of(tree), seed=12)["random30"]).cuda())
        refined = opt.tree
        trees.append(refined)
        torch.cuda.synchronize()
        cap = refined.capacity
        assert cap > tree.capacity
        child = refined.child_.reshape(cap, N3).astype(np.int32)
        before = {k: getattr(opt, k).cpu().numpy().reshape(-1, dd).view(np.uint32) for k in ("master", "m", "v")}
        assert before["m"].any() and before["v"].any()
        sel = cu.selections(child, seed=13)["random50"]
        node_map = opt.collapse(torch.from_numpy(sel).cuda())
        torch.cuda.synchronize()
        assert opt.tree is not refined
        trees.append(opt.tree)
        want = cu.restate(child, sel, [(before["master"], cu.MEAN), (before["m"], cu.ZERO), (before["v"], cu.ZERO)])
        n_keep = want["n_keep"]
        assert n_keep < cap and np.array_equal(node_map.cpu().numpy(), want["node_map"])
        for key, w, rule in zip(("master", "m", "v"), want["dsts"], (cu.MEAN, cu.ZERO, cu.ZERO)):
            got = getattr(opt, key)
            assert tuple(got.shape) == (n_keep, 2, 2, 2, dd), key
            cu.assert_array(got.cpu().numpy().reshape(-1, dd).view(np.uint32), w, rule, want["into_slot"], key)
        assert tuple(opt.grad.shape) == tuple(opt.master.shape) and not bool(opt.grad.any())
        assert opt.touched.numel() == (n_keep * N3 + 31) // 32 and not bool(opt.touched.any())
        assert np.array_equal(opt.tree.child_.reshape(-1, N3), want["child_out"])

        # the tree holds binary16(master) in every slot: a fresh upload of the collapsed child array that takes its
        # values from update_data(master) is the same tree
        fresh = api.N3Tree.from_arrays(want["child_out"].reshape(n_keep, 2, 2, 2),
                                       np.zeros((n_keep, 2, 2, 2, dd), np.float16), tree.offset, tree.invradius3,
                                       tree.data_format, tree.extra)
        trees.append(fresh)

        def same_as_fresh():
            fresh.update_data(opt.master)
            assert np.array_equal(opt.tree.read_data().cpu().numpy().view(np.uint16),
                                  fresh.read_data().cpu().numpy().view(np.uint16))
            (rgba_a, acc_a), (rgba_b, acc_b) = frames(torch, opt.tree, 0), frames(torch, fresh, 0)
            assert acc_a.any() and np.array_equal(rgba_a, rgba_b)
            assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
        same_as_fresh()

        sq = opt.fit(o, d, target)
        opt.step()
        torch.cuda.synchronize()
        assert opt.tree.status() == 0 and opt.steps == 3 and bool(torch.isfinite(sq).all())
        assert not bool(opt.grad.any()) and not bool(opt.touched.any())
        moved = opt.master.cpu().numpy().reshape(-1, dd).view(np.uint32)
        assert not np.array_equal(moved, want["dsts"][0])
        same_as_fresh()
    finally:
        for x in trees:
            x.free_device()
