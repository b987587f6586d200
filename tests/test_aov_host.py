"""vr_render_aov, the part that needs no GPU: the C ABI (symbol, prototype, struct layout,
constants) and every refusal -- through C, C++ and Python.  All checks of vr_render_aov come before
the tree handle is dereferenced and before any device call, so the calls below pass a tree handle
that is never followed (and device pointers that are never written)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from volrend_amd import _abi, build

INVALID, UNSUPPORTED = 1, 5
TREE, IMG, PLANE = 0x1000, 0x2000, 0x3000   # never dereferenced


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbol_prototype_and_constants(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "vr_render_aov" in exported
    res, args = _abi.PROTOTYPES["vr_render_aov"]
    assert res is C.c_int and len(args) == 8
    assert L.vr_render_aov.argtypes == args
    assert (_abi.DEPTH_TREE, _abi.DEPTH_WORLD) == (0, 1)
    assert L.vr_abi_version() == 3   # additions only


def test_vraov_layout_matches_the_c_compiler():
    st = _abi.VrAov
    got = build_util.c_struct_layout("VrAov", st, [("tree", "VR_DEPTH_TREE"), ("world", "VR_DEPTH_WORLD"),
                                                   ("abi", "VR_ABI_VERSION")])
    assert [f for f, _ in st._fields_] == ["depth", "transmittance", "pitch"]
    assert got["size"] == C.sizeof(st) == 24
    for fname, _ in st._fields_:
        assert got[fname] == getattr(st, fname).offset, fname
    assert (got["tree"], got["world"], got["abi"]) == (0, 1, 3)


def _args(n=1, w=64, h=48):
    cams = (_abi.VrCamera * n)()
    frames = (_abi.VrFrame * n)()
    aovs = (_abi.VrAov * n)()
    opt = _abi.VrRenderOptions()
    _abi.lib().vr_default_options(C.byref(opt))
    for i in range(n):
        cams[i].width, cams[i].height, cams[i].fx, cams[i].fy = w, h, 50.0, 50.0
        _abi.lib().vr_default_frame(C.byref(frames[i]))
        frames[i].rgba = IMG
        frames[i].offscreen = 1
        aovs[i].depth = PLANE
        aovs[i].transmittance = PLANE
    return cams, opt, frames, aovs


def _call(L, n, cams, opt, frames, aovs, units=0, tree=TREE):
    rc = L.vr_render_aov(tree, n, cams, C.byref(opt), frames, aovs, units, None)
    return rc, (L.vr_last_error() or b"").decode()


def test_invalid_arguments_through_c(L):
    cams, opt, frames, aovs = _args(2)
    rc, msg = _call(L, 2, cams, opt, frames, None)
    assert rc == INVALID and "aovs is NULL" in msg
    rc, msg = _call(L, 2, cams, opt, frames, aovs, units=2)
    assert rc == INVALID and "depth_units" in msg
    rc, msg = _call(L, 2, cams, opt, frames, aovs, units=-1)
    assert rc == INVALID and "depth_units" in msg
    aovs[1].depth = aovs[1].transmittance = None
    rc, msg = _call(L, 2, cams, opt, frames, aovs)
    assert rc == INVALID and "frame 1" in msg and "NULL" in msg
    cams, opt, frames, aovs = _args(1)
    for pitch in (64 * 4 - 4, 64 * 4 + 2, 4, -256):
        aovs[0].pitch = pitch
        rc, msg = _call(L, 1, cams, opt, frames, aovs, units=1)
        assert rc == INVALID and "pitch" in msg, pitch
    # everything vr_render_batch refuses
    cams, opt, frames, aovs = _args(1)
    assert _call(L, 1, cams, opt, frames, aovs, tree=None)[0] == INVALID
    assert _call(L, 0, cams, opt, frames, aovs)[0] == INVALID
    assert _call(L, _abi.MAX_BATCH + 1, cams, opt, frames, aovs)[0] == INVALID
    frames[0].rgba = None
    assert _call(L, 1, cams, opt, frames, aovs)[0] == INVALID
    cams, opt, frames, aovs = _args(1)
    opt.step_size = 0.0
    assert _call(L, 1, cams, opt, frames, aovs)[0] == INVALID
    cams, opt, frames, aovs = _args(1)
    frames[0].fp_mode = 9
    assert _call(L, 1, cams, opt, frames, aovs)[0] == INVALID
    cams, opt, frames, aovs = _args(2)
    cams[1].width = 32
    assert _call(L, 2, cams, opt, frames, aovs)[0] == INVALID


def test_unsupported_through_c(L):
    cams, opt, frames, aovs = _args(2)
    opt.render_depth = 1
    rc, msg = _call(L, 2, cams, opt, frames, aovs)
    assert rc == UNSUPPORTED and "render_depth" in msg
    opt.render_depth, opt.enable_probe = 0, 1
    rc, msg = _call(L, 2, cams, opt, frames, aovs)
    assert rc == UNSUPPORTED and "probe" in msg
    opt.enable_probe = 0
    frames[1].counters = 0x4000
    rc, msg = _call(L, 2, cams, opt, frames, aovs)
    assert rc == UNSUPPORTED and "counters" in msg and "frame 1" in msg


def test_refusals_through_python(L):
    from volrend_amd import api
    cam = api.Camera(64, 48, 50.0, 50.0)
    t = common.FakeTree(handle=TREE, capacity=None, N=None, data_dim=None, data_format=None)

    def code(**kw):
        opts = kw.pop("opts", api.RenderOptions())
        with pytest.raises(_abi.VolrendError) as e:
            api.launch_renderer(t, cam, opts, IMG, None, None, True, **kw)
        return e.value.code

    assert code(aov=api.AovPlanes()) == INVALID
    assert code(aov=api.AovPlanes(PLANE, None, 64 * 4 + 2)) == INVALID
    assert code(aov=(PLANE, PLANE), depth_units=5) == INVALID
    assert code(aov=(PLANE, PLANE), opts=api.RenderOptions(render_depth=True)) == UNSUPPORTED
    assert code(aov=(PLANE, PLANE), opts=api.RenderOptions(enable_probe=True)) == UNSUPPORTED
    assert code(aov=(PLANE, PLANE), counters=0x4000) == UNSUPPORTED
    with pytest.raises(ValueError, match="depth_units"):
        api.launch_renderer(t, cam, api.RenderOptions(), IMG, None, None, True, aov=(PLANE, PLANE),
                            depth_units="metres")
    tr = np.zeros(12, np.float32)
    with pytest.raises(ValueError, match="one AovPlanes per pose"):
        api.PreparedBatch(t, cam, [tr, tr], api.RenderOptions(), [IMG, IMG], aov=[api.AovPlanes(PLANE)])
    pb = api.PreparedBatch(t, cam, [tr, tr], api.RenderOptions(), [IMG, IMG],
                           aov=[api.AovPlanes(PLANE), api.AovPlanes()], depth_units="world")
    with pytest.raises(_abi.VolrendError) as e:
        pb.launch()
    assert e.value.code == INVALID
    with pytest.raises(_abi.VolrendError) as e:
        api.launch_renderer_batch(t, cam, [tr], api.RenderOptions(render_depth=True), [IMG],
                                  aov=[api.AovPlanes(None, PLANE)])
    assert e.value.code == UNSUPPORTED


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("aov_check", tmp_path), refusals=True)
    for case, word in [("both_null", "NULL"), ("units", "depth_units"), ("pitch_small", "pitch"),
                       ("pitch_odd", "pitch"), ("render_depth", "render_depth"), ("probe", "probe"),
                       ("null_image", "rgba"), ("batch_second_null", "frame 1")]:
        assert got[case].startswith("runtime_error: vr_render_aov:") and word in got[case], (case, got[case])
    assert got["batch_sizes"].startswith("invalid_argument:")
