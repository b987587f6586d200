"""The view checks every launch shares (a focal length, one set of intrinsics per batch): the same code and
message from vr_render_batch and from vr_accumulate_weights, and their place among the other refusals of
vr_render_batch.  No GPU: every check comes before the tree handle is followed."""
import ctypes as C
import os

import pytest

from volrend_amd import _abi, build

INVALID = 1
TREE, BUF = 0x1000, 0x2000   # never dereferenced


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def _args(n):
    cams, frames = (_abi.VrCamera * n)(), (_abi.VrFrame * n)()
    opt, out = _abi.VrRenderOptions(), _abi.VrLeafWeights()
    _abi.lib().vr_default_options(C.byref(opt))
    for i in range(n):
        cams[i].width, cams[i].height, cams[i].fx, cams[i].fy = 64, 48, 50.0, 50.0
        _abi.lib().vr_default_frame(C.byref(frames[i]))
        frames[i].rgba = BUF
    out.max_weight = BUF
    return cams, frames, opt, out


def _both(L, n, cams, frames, opt, out):
    """(code, message) of the colour launch and of the leaf-weight launch over the same views."""
    rc_c = L.vr_render_batch(TREE, n, cams, C.byref(opt), frames, None)
    msg_c = (L.vr_last_error() or b"").decode()
    rc_w = L.vr_accumulate_weights(TREE, n, cams, C.byref(opt), 0, C.byref(out), None)
    return (rc_c, msg_c), (rc_w, (L.vr_last_error() or b"").decode())


def test_focal_length_and_intrinsics_are_one_refusal_for_both_launches(L):
    for field in ("fx", "fy"):
        cams, frames, opt, out = _args(2)
        for c in cams:
            setattr(c, field, 0.0)
        colour, weights = _both(L, 2, cams, frames, opt, out)
        assert colour == weights == (INVALID, "focal length must be non-zero"), field
    for field, value in (("width", 32), ("height", 40), ("fx", 51.0), ("fy", 49.0)):
        cams, frames, opt, out = _args(3)
        setattr(cams[2], field, value)
        colour, weights = _both(L, 3, cams, frames, opt, out)
        assert colour == weights == (INVALID, "frame 2: intrinsics differ within the batch"), field


def test_order_of_the_view_checks_in_a_colour_launch(L):
    # the focal length is looked at before any frame, the intrinsics of frame i behind its rgba and before
    # its layout, all of them before step_size
    cams, frames, opt, out = _args(3)
    cams[0].fx = 0.0
    frames[0].rgba = None
    assert "focal length" in _both(L, 3, cams, frames, opt, out)[0][1]
    cams, frames, opt, out = _args(3)
    cams[2].width, frames[1].rgba = 32, None
    assert "frame 1: rgba is NULL" in _both(L, 3, cams, frames, opt, out)[0][1]
    cams, frames, opt, out = _args(3)
    cams[1].width, frames[1].pitch, opt.step_size = 32, 512, 0.0
    colour, weights = _both(L, 3, cams, frames, opt, out)
    assert "frame 1: intrinsics differ" in colour[1]
    assert "step_size" in weights[1]   # (the leaf-weight launch looks at step_size first)
