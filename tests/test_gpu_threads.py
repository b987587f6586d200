"""-m gpu: the C ABI from concurrent host threads (tests/cpp/threads_check.cpp, which says what each mode does).

include/volrend_hip.h promises that any number of launches on any number of streams AND HOST THREADS is safe (more
than 8 unfinished launches of one tree serialise), the same for the point queries and vr_order_rays, and per-tree
calls that run on the tree's device whatever the calling thread's device is.  Every other test drives the library
from one host thread.  Here the program's threads each own a stream, their inputs and their outputs, and every
output is held to the yardstick the single-threaded tests use -- the oracle's frames, the restatements of the AOV
planes, the leaf weights, the queries and the ray order bit for bit, the float64 gradient formulas with the bound
k = 148 units of tests/grad_util.py -- so a frame table, ray buffer, probe buffer or status word taken from another
thread's launch slot shows as a wrong output.

  cold     12 threads > 8 slots, a fresh tree without vr_reserve*: every launch of every round grows its slot's ray
           buffer outside the launch mutex.  A launch that finds all 8 slots growing waits for one (it used to be
           refused).
  mixed    one thread per call family on one tree, beside a thread that turns scheduling knobs and reads the tree's
           tallies, a thread that rewrites the values of a CLONE of a second tree between frames, and a thread that
           renders that second tree itself (the clone's updates must stay in the clone).  The same scripts run
           serially first: threaded == serial word for word, and serial == the yardsticks.
  uploads  a plain, a quantised, a device-resident and a staged (shared pinned-slot cache) upload at the same moment,
           beside two threads that render.
  devices  cold with 8 threads, the odd ones with another current device; skipped with fewer than two devices.

The scenes are the smallest that reach every lookup kind (tests/update_util.py "mixed"): depth 5 SH9 under
top_levels = 2, brick_levels = 1; frames of 44 x 20 pixels (ragged 8 x 8 blocks); ray lists of 3000 rays."""
import dataclasses
import os

import numpy as np
import pytest

from tests import aov_util, build_util, common, fit_util, order_util, weights_util
from tests import grad_util as gu
from tests import query_util as qu
from tests import rays_util as ru
from tests import update_util as uu
from tests.common import ob

pytestmark = pytest.mark.gpu

W, H = 44, 20
F = W * 1111.111 / 800.0
RW, RH = 60, 50                      # the ray list: the 3000 pixel rays of one camera, which the frame yardsticks judge
RF = RW * 1111.111 / 800.0
N_RAYS = RW * RH
N_POINTS = 2000
COLD_THREADS, DEVICE_THREADS, COLD_ROUNDS = 12, 8, 5
ROUNDS = 4                           # of every family of `mixed`
CLONE_ROUNDS = 6
RENDER_ROUNDS = 8                    # of the two rendering threads of `uploads`
UPLOAD_SIZE = 32
UPLOAD_F = UPLOAD_SIZE * 1111.111 / 800.0
GRAD_SCALE = 2.0 / (3 * N_RAYS)
FORMATS = {"RGBA": 0, "SH": 1, "SG": 2, "ASG": 3}


def pose(i, radius=4.0):
    """Pose i of an orbit of 64: no two threads or frames of a mode share one."""
    return np.asarray(common.camera_for(pose_idx=i % 64, n_poses=64, radius=radius)[0], np.float32)


def write_tree(d, name, tree, quant=None):
    bits = lambda a: [int(x) for x in np.asarray(a, np.float32).view(np.uint32)]
    nq, nr = (0, 0) if quant is None else (quant["quant_map"].shape[0], 0 if quant["data_retained"] is None else quant["data_retained"].shape[0])
    meta = [tree.N, tree.capacity, tree.data_dim, FORMATS[tree.format_name], tree.basis_dim, *bits(tree.offset),
            *bits(tree.invradius3), nq, nr]
    (d / f"{name}.meta").write_text(" ".join(map(str, meta)) + "\n")
    np.ascontiguousarray(tree.child, np.int32).tofile(d / f"{name}.child")
    if quant is None:
        np.ascontiguousarray(tree.data, np.float16).tofile(d / f"{name}.data")
        return
    for key, ext in (("quant_colors", "qc"), ("quant_map", "qm"), ("sigma", "sigma"), ("data_retained", "ret")):
        if quant[key] is not None:
            np.ascontiguousarray(quant[key]).tofile(d / f"{name}.{ext}")


def other_values(tree, seed):
    """Another value array for the tree (float16, the file's shape): every coefficient and the occupancy redrawn;
    internal slots get a sigma the library must ignore."""
    rng = np.random.default_rng(seed)
    shape = tree.data.shape
    data = (rng.standard_normal(shape) * 0.6).astype(np.float32)
    sigma = np.where(rng.random(shape[:-1]) < 0.5, np.exp(rng.uniform(np.log(2.0), np.log(60.0), shape[:-1])), 0.0)
    data[..., -1] = np.where(np.asarray(tree.child) == 0, sigma, 7.0)
    return data.astype(np.float16)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The inputs of every mode, written once; -> dict of what the checks need."""
    d = tmp_path_factory.mktemp("threads")
    main = common.small_scene(depth=5, basis_dim=9)
    aux = common.small_scene(depth=4, basis_dim=16)
    write_tree(d, "main", main)
    write_tree(d, "aux", aux)
    a, b = other_values(aux, 1), other_values(aux, 2)
    a.tofile(d / "aux_A.data")
    b.tofile(d / "aux_B.data")
    cold = np.stack([pose(COLD_ROUNDS * t + i) for t in range(COLD_THREADS) for i in range(COLD_ROUNDS)])
    cold.tofile(d / "cold_poses.raw")
    frame_poses = np.stack([pose(3), pose(41)])
    frame_poses.tofile(d / "frame_poses.raw")
    aux_pose = pose(17)
    aux_pose.tofile(d / "aux_pose.raw")
    ray_pose = pose(9)
    o, dirs = ru.rays_of_camera(ray_pose, RW, RH, RF)
    o.tofile(d / "rays_o.raw")
    dirs.tofile(d / "rays_d.raw")
    g = gu.upstream("normal", 1, RH, RW)[0].reshape(-1, 4)
    np.ascontiguousarray(g).tofile(d / "rays_g.raw")
    target = fit_util.targets(N_RAYS, 5)
    target.tofile(d / "rays_target.raw")
    pts = qu.point_set(main, N_POINTS, 104)
    pdirs = qu.direction_set(N_POINTS, 105)
    pts.tofile(d / "points.raw")
    pdirs.tofile(d / "point_dirs.raw")
    upload_pose = pose(24)
    upload_pose.tofile(d / "upload_pose.raw")
    params = dict(w=W, h=H, f=repr(F), n_rays=N_RAYS, n_points=N_POINTS, bg=fit_util.BG, grad_scale=repr(float(np.float32(GRAD_SCALE))),
                  upload_size=UPLOAD_SIZE, upload_f=repr(UPLOAD_F))
    (d / "params.txt").write_text("".join(f"{k} {v}\n" for k, v in params.items()))
    exe = build_util.cpp_program("threads_check", tmp_path_factory.mktemp("bin"), gpu=True)
    return dict(dir=d, exe=exe, main=main, aux=aux, a=a, b=b, cold=cold, frame_poses=frame_poses, aux_pose=aux_pose,
                ray_pose=ray_pose, o=o, d=dirs, g=g, target=target, pts=pts, pdirs=pdirs, upload_pose=upload_pose)


def raw(scene, name, dtype, shape):
    return np.fromfile(os.path.join(scene["dir"], name + ".raw"), dtype).reshape(shape)


def assert_frames(scene, prefix, tree, poses, what, w=W, h=H, f=F):
    """Outputs <prefix>rgba / accum hold len(poses) frames: each equals the oracle's frame of its pose."""
    rgba = raw(scene, prefix + "rgba", np.uint8, (len(poses), h, w, 4))
    accum = raw(scene, prefix + "accum", np.float32, (len(poses), h, w, 4))
    for i, tr in enumerate(poses):
        rgba_o, acc_o, cnt = common.oracle_frame(tree, tr, w, h, f)
        assert cnt["hit_samples"] > 0, f"{what}: pose {i} sees nothing"
        bad = int((rgba[i] != rgba_o).any(-1).sum())
        assert bad == 0, f"{what}, frame {i}: {bad} RGBA8 pixels differ from the oracle"
        bad = int((accum[i].view(np.uint32) != acc_o.view(np.uint32)).any(-1).sum())
        assert bad == 0, f"{what}, frame {i}: {bad} accumulator pixels differ from the oracle"


def check_cold(scene, mode, n_threads):
    got = build_util.run_key_values(scene["exe"], mode, scene["dir"])
    if got.get("skipped") == "1":
        pytest.skip("fewer than two devices")
    assert (got["main_top_levels"], got["main_brick_levels"], got["status"]) == ("2", "1", "0"), got
    if mode == "devices":
        assert got["devices_kept"] == "1", "a thread's current device changed under the library's calls"
    for t in range(n_threads):
        assert_frames(scene, f"{mode}_t{t}_", scene["main"], scene["cold"][COLD_ROUNDS * t:COLD_ROUNDS * (t + 1)],
                      f"{mode}, thread {t}")


def test_cold_launches_of_twelve_threads_wait_for_a_slot(scene):
    """Exit status 0 (no call refused), status word 0, and each of the 12 x 5 frames of the last round is the
    oracle's frame of that thread's pose."""
    check_cold(scene, "cold", COLD_THREADS)


def test_devices_threads_with_another_current_device(scene):
    check_cold(scene, "devices", DEVICE_THREADS)


# ---- mixed -----------------------------------------------------------------------------------------------------------
# worker number -> its outputs: (name, dtype, words per item), the items being given by `counts`
BATCH, AOV, RAYS, WEIGHTS, WEIGHTS_RAYS, QUERY, ORDER, BACKWARD, FIT, TUNING, CLONE, ORIG = range(12)


def mixed_outputs(scene):
    main = scene["main"]
    slots, px = main.capacity * main.N ** 3, W * H
    frames = lambda n: [("rgba", np.uint8, n * px * 4), ("accum", np.float32, n * px * 4)]
    words = (slots + 31) // 32
    return {BATCH: frames(2), AOV: frames(2) + [("depth", np.float32, 2 * px), ("trans", np.float32, 2 * px)],
            RAYS: [("rgba", np.uint8, N_RAYS * 4), ("accum", np.float32, N_RAYS * 4)],
            WEIGHTS: [("max_weight", np.float32, slots), ("hits", np.uint32, slots)],
            WEIGHTS_RAYS: [("max_weight", np.float32, slots), ("hits", np.uint32, slots)],
            QUERY: [("sigma", np.float32, N_POINTS), ("depth", np.int32, N_POINTS), ("coeffs", np.float32, N_POINTS * (main.data_dim - 1)),
                    ("rgb", np.float32, N_POINTS * 3)],
            ORDER: [("order", np.uint32, N_RAYS), ("keys", np.uint32, N_RAYS), ("origins", np.float32, N_RAYS * 3), ("dirs", np.float32, N_RAYS * 3)],
            BACKWARD: [("grad", np.float32, slots * main.data_dim), ("touched", np.uint32, words)],
            FIT: [("grad", np.float32, slots * main.data_dim), ("touched", np.uint32, words), ("sq_err", np.float32, N_RAYS),
                  ("accum", np.float32, N_RAYS * 4)],
            TUNING: [], CLONE: frames(CLONE_ROUNDS), ORIG: frames(CLONE_ROUNDS)}


@pytest.fixture(scope="module")
def mixed(scene):
    """One run of the program -> {(pass, worker, name): array}."""
    got = build_util.run_key_values(scene["exe"], "mixed", scene["dir"])
    assert (got["serial_status"], got["threaded_status"]) == ("0", "0"), got
    out = {}
    for p in ("serial", "threaded"):
        for worker, outs in mixed_outputs(scene).items():
            for name, dtype, count in outs:
                out[p, worker, name] = raw(scene, f"{p}_{worker}_{name}", dtype, (count,))
    return out


@pytest.fixture(scope="module")
def ray_trace(scene):
    """The constants of the ray list's differentiation: the list is the frame of one camera."""
    main = scene["main"]
    trace = gu.Trace(main, scene["ray_pose"], RW, RH, RF, 0)
    return dict(tree=main, traces=[trace], w=RW, h=RH, d64=gu.data64_of(main))


def grad_reference(ray_trace, g):
    """grad_util.reference's dict for ROUNDS calls that each add the list's gradient for the upstream g [n, 4]."""
    grad, mag, under = (np.zeros(ray_trace["d64"].shape, np.float64) for _ in range(3))
    for _ in range(ROUNDS):
        ray_trace["traces"][0].backward64(ray_trace["d64"], np.asarray(g, np.float64).reshape(RH, RW, 4), grad, mag, under)
    return dict(ray_trace, grad=grad, mag=mag, under=under)


def test_mixed_threaded_equals_serial(scene, mixed):
    """Every output word for word, except the two gradient arrays (their sums have no defined order)."""
    for (p, worker, name), serial in mixed.items():
        if p != "serial" or (worker in (BACKWARD, FIT) and name == "grad"):
            continue
        threaded = mixed["threaded", worker, name]
        bad = serial.view(np.uint8) != threaded.view(np.uint8)
        assert not bad.any(), f"worker {worker}, {name}: {int(bad.sum())} bytes differ between the serial and the threaded run"


def test_mixed_serial_frames_equal_the_oracle(scene, mixed):
    assert_frames(scene, f"serial_{BATCH}_", scene["main"], scene["frame_poses"], "vr_render_batch")
    assert_frames(scene, f"serial_{AOV}_", scene["main"], scene["frame_poses"], "vr_render_aov")
    assert_frames(scene, f"serial_{RAYS}_", scene["main"], [scene["ray_pose"]], "vr_render_rays", RW, RH, RF)


def test_mixed_serial_aov_planes_equal_the_restatement(scene, mixed):
    for i, tr in enumerate(scene["frame_poses"]):
        D, T, _, _ = aov_util.restate(scene["main"], tr, W, H, F)
        assert (T < 1).any()
        aov_util.assert_same_bits(mixed["serial", AOV, "depth"].reshape(2, H, W)[i], D, f"depth, frame {i}")
        aov_util.assert_same_bits(mixed["serial", AOV, "trans"].reshape(2, H, W)[i], T, f"transmittance, frame {i}")


def test_mixed_serial_weights_equal_the_restatement(scene, mixed):
    main = scene["main"]
    shape = weights_util.slots_shape(main)
    mw, hits, _ = weights_util.restate(main, list(scene["frame_poses"]) * ROUNDS, W, H, F)
    assert hits.any()
    weights_util.assert_same_slots(mixed["serial", WEIGHTS, "max_weight"].reshape(shape), mixed["serial", WEIGHTS, "hits"].reshape(shape),
                                   mw, hits, "vr_accumulate_weights")
    mw, hits, _ = weights_util.restate(main, [scene["ray_pose"]] * ROUNDS, RW, RH, RF)
    assert hits.any()
    weights_util.assert_same_slots(mixed["serial", WEIGHTS_RAYS, "max_weight"].reshape(shape),
                                   mixed["serial", WEIGHTS_RAYS, "hits"].reshape(shape), mw, hits, "vr_accumulate_weights_rays")


def test_mixed_serial_queries_and_order_equal_the_restatements(scene, mixed):
    main = scene["main"]
    th = ob.TreeHandle(main)
    ans = qu.oracle_answers(main, th, scene["pts"], "tree")
    qu.check_point_set(main, ans, "mixed")
    ans["rgb"] = qu.recompose_rgb(main, th, ans["coeffs"], scene["pdirs"])
    for k in ("sigma", "depth", "coeffs", "rgb"):
        qu.same_words(mixed["serial", QUERY, k].reshape(ans[k].shape), ans[k], f"vr_query_points {k}")
    keys = order_util.keys_of(main, scene["o"], scene["d"], 0)
    order, sorted_keys = order_util.result_of(keys)
    assert np.unique(keys).size > 16
    assert np.array_equal(mixed["serial", ORDER, "order"], order)
    assert np.array_equal(mixed["serial", ORDER, "keys"], sorted_keys)
    assert np.array_equal(mixed["serial", ORDER, "origins"].view(np.uint32).reshape(-1, 3), scene["o"][order].view(np.uint32))
    assert np.array_equal(mixed["serial", ORDER, "dirs"].view(np.uint32).reshape(-1, 3), scene["d"][order].view(np.uint32))


@pytest.mark.parametrize("run", ["serial", "threaded"])
def test_mixed_backward_gradients(scene, mixed, ray_trace, run):
    """As tests/test_gpu_rays.py judges a backward call: |gpu - float64| <= 148 units per element, elements nothing
    touches keep their bits, and the touched bitmap is the restatement's hit set bit for bit."""
    ref = grad_reference(ray_trace, scene["g"])
    gu.assert_parity(mixed[run, BACKWARD, "grad"].reshape(ref["grad"].shape), ref, what=f"{run} vr_render_backward_rays_touched")
    want = gu.mark_words(gu.hit_slots(ref))
    assert want.any() and np.array_equal(mixed[run, BACKWARD, "touched"], want)


@pytest.mark.parametrize("run", ["serial", "threaded"])
def test_mixed_fit_gradients(scene, mixed, ray_trace, run):
    """As tests/test_gpu_fit.py judges a fused call: accum is the colour launch's, sq_err the numpy head's, the
    gradient that of the head's g within 148 units, touched the hit set."""
    _, acc_o, _ = common.oracle_frame(scene["main"], scene["ray_pose"], RW, RH, RF)
    accum = mixed[run, FIT, "accum"].reshape(-1, 4)
    assert np.array_equal(accum.view(np.uint32), acc_o.reshape(-1, 4).view(np.uint32))
    head = fit_util.head(accum, scene["target"], fit_util.BG, np.float32(GRAD_SCALE))
    assert np.array_equal(mixed[run, FIT, "sq_err"].view(np.uint32), head["sq_err"].view(np.uint32))
    ref = grad_reference(ray_trace, head["g"])
    gu.assert_parity(mixed[run, FIT, "grad"].reshape(ref["grad"].shape), ref, what=f"{run} vr_fit_rays")
    assert np.array_equal(mixed[run, FIT, "touched"], gu.mark_words(gu.hit_slots(ref)))


def test_mixed_clone_updates_stay_in_the_clone(scene, mixed):
    """Frame j of the clone thread is the oracle's frame of value array A (j even) or B (j odd); every frame of
    the thread that renders the original is the original's."""
    aux = scene["aux"]
    for run in ("serial", "threaded"):
        for j in range(CLONE_ROUNDS):
            tree = uu.with_data(aux, scene["b"] if j % 2 else scene["a"])
            rgba_o, acc_o, _ = common.oracle_frame(tree, scene["aux_pose"], W, H, F)
            got = mixed[run, CLONE, "rgba"].reshape(CLONE_ROUNDS, H, W, 4)[j], mixed[run, CLONE, "accum"].reshape(CLONE_ROUNDS, H, W, 4)[j]
            assert np.array_equal(got[0], rgba_o) and np.array_equal(got[1].view(np.uint32), acc_o.view(np.uint32)), \
                f"{run}: frame {j} of the clone is not that of value array {'AB'[j % 2]}"
        assert_frames(scene, f"{run}_{ORIG}_", aux, [scene["aux_pose"]] * CLONE_ROUNDS, f"{run}: the original beside its clone's updates")
    a_frame = common.oracle_frame(uu.with_data(aux, scene["a"]), scene["aux_pose"], W, H, F)[0]
    b_frame = common.oracle_frame(uu.with_data(aux, scene["b"]), scene["aux_pose"], W, H, F)[0]
    o_frame = common.oracle_frame(aux, scene["aux_pose"], W, H, F)[0]
    assert (a_frame != b_frame).any() and (a_frame != o_frame).any() and (b_frame != o_frame).any()


# ---- uploads ---------------------------------------------------------------------------------------------------------
def test_uploads_at_the_same_moment(scene, tmp_path):
    """Each new tree's frame is its oracle frame, its read_data what the device must hold of its file; the two
    threads that render meanwhile get the oracle's frame every time."""
    from volrend_amd import _tree
    d = scene["dir"]
    quant = common.small_scene(depth=4, basis_dim=4, seed=5)
    npz = str(tmp_path / "q.npz")
    common.write_quantised_npz(quant, npz, n_retain=1, compressed=False)
    write_tree(d, "quant", quant, _tree._quant_arrays(np.load(npz), quant.child))
    staged = common.small_scene(depth=7, basis_dim=25, seed=431)      # tests/test_gpu_upload.py: the smallest staged upload
    assert staged.capacity == 37481 and staged.child.nbytes + staged.data.nbytes >= 32 << 20
    write_tree(d, "staged", staged)
    got = build_util.run_key_values(scene["exe"], "uploads", d)
    assert got["status"] == "0", got
    for worker, tree in enumerate((scene["aux"], quant, scene["main"], staged)):
        what = ("plain", "quantised", "device-resident", "staged")[worker]
        assert_frames(scene, f"uploads_{worker}_", tree, [scene["upload_pose"]], f"{what} upload", UPLOAD_SIZE, UPLOAD_SIZE, UPLOAD_F)
        read = raw(scene, f"uploads_{worker}_data", np.uint16, tree.data.shape)
        want = uu.stored(tree, tree.data).view(np.uint16)
        bad = read != want
        assert not bad.any(), f"{what} upload: {int(bad.sum())} of {bad.size} halfs of vr_tree_read_data differ from the file"
    for worker, tr in ((4, scene["frame_poses"][0]), (5, scene["frame_poses"][1])):
        assert_frames(scene, f"uploads_{worker}_", scene["main"], [tr] * RENDER_ROUNDS, f"rendering thread {worker - 4}")
    os.remove(d / "staged.data")
    os.remove(d / "uploads_3_data.raw")
