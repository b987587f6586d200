"""vr_order_rays, the part that needs no GPU: the C ABI (symbols, prototypes, the layout of VrRayOrder), the workspace
rule, and every refusal that comes before the tree handle is followed -- through C and C++.  The calls below pass a
tree handle that is never followed and device pointers that are never read or written."""
import ctypes as C
import os
import subprocess

import pytest

from tests import build_util
from volrend_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
TREE, O, D, P, PO, ORD, KEYS, OO, DO, WS = (0x1000, 0x3000, 0x5000, 0x7000, 0x9000, 0xB000, 0xD000, 0xF000, 0x11000,
                                            0x100000)   # never dereferenced
NAME = "vr_order_rays"


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def test_symbols_prototypes_and_abi_version(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "volrend_hip.h")).read()
    assert NAME in exported and NAME + "_workspace" in exported
    res, args = _abi.PROTOTYPES[NAME]
    assert res is C.c_int and len(args) == 9 and args[1] is C.c_int64 and args[7] is C.c_size_t
    assert args[2] is C.POINTER(_abi.VrRays) and args[5] is C.POINTER(_abi.VrRayOrder)
    assert getattr(L, NAME).argtypes == args
    assert _abi.PROTOTYPES[NAME + "_workspace"] == (C.c_int64, [C.c_int64])
    assert f"int {NAME}(vr_tree_t tree, int64_t n, const VrRays* rays, const VrRenderOptions* opt, int fp_mode,\n" in header
    assert f"int64_t {NAME}_workspace(int64_t n);" in header
    assert L.vr_abi_version() == 3 and "#define VR_ABI_VERSION 3" in header   # additions only
    assert "typedef struct VrRayOrder" in header


def test_vrrayorder_layout_is_the_c_compilers():
    got = build_util.c_struct_layout("VrRayOrder", _abi.VrRayOrder)
    assert got.pop("size") == C.sizeof(_abi.VrRayOrder) == 64
    assert got == {f: getattr(_abi.VrRayOrder, f).offset for f, _ in _abi.VrRayOrder._fields_}
    assert [f for f, _ in _abi.VrRayOrder._fields_] == ["bits", "order", "keys", "origins_out", "dirs_out", "payload",
                                                        "payload_out", "payload_dim"]


def test_workspace_rule(L):
    """0 at 0, non-decreasing over a ladder up to 2^30 - 1, room for the four [n] word arrays of the pairs -- and no
    device call: this process has not initialised HIP, and the function answers where no device is visible."""
    ws = L.vr_order_rays_workspace
    assert ws(0) == 0 and ws(-5) == 0
    ladder = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 65535, 65536, 65537, 10 ** 6, 2 ** 24 + 1, 2 ** 29,
              2 ** 30 - 2, 2 ** 30 - 1]
    sizes = [ws(n) for n in ladder]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s >= 16 * n and s % 256 == 0 for s, n in zip(sizes, ladder))
    assert sizes[-1] < 2 ** 35                     # (about 20 bytes per ray: no overflow, no absurd request)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    code = ("import ctypes as C; L = C.CDLL(%r); L.vr_order_rays_workspace.restype = C.c_int64; "
            "L.vr_order_rays_workspace.argtypes = [C.c_int64]; print(L.vr_order_rays_workspace(65536))" % _abi.LIB_PATH)
    import sys
    assert int(subprocess.check_output([sys.executable, "-c", code], env=env, text=True).split()[-1]) == ws(65536)


def _opt():
    opt = _abi.VrRenderOptions()
    _abi.lib().vr_default_options(C.byref(opt))
    return opt


def _call(L, n=100, rays=(O, D), opt="default", out="default", fp_mode=0, tree=TREE, workspace=WS, nbytes=None,
          **fields):
    """One call; rays / opt / out = None pass a NULL pointer; ``fields`` overwrite those of VrRayOrder -> (rc, message)."""
    r = None
    if rays is not None:
        r = _abi.VrRays()
        r.origins, r.dirs = rays
    o = _opt() if isinstance(opt, str) else opt
    ro = None
    if out is not None:
        ro = _abi.VrRayOrder()
        ro.bits, ro.order, ro.keys, ro.origins_out, ro.dirs_out = 0, ORD, KEYS, OO, DO
        ro.payload, ro.payload_out, ro.payload_dim = P, PO, 3
        for k, v in fields.items():
            setattr(ro, k, v)
    ptr = lambda x: None if x is None else C.byref(x)   # noqa: E731
    if nbytes is None:
        nbytes = L.vr_order_rays_workspace(max(min(n, 2 ** 30 - 1), 0))
    rc = L.vr_order_rays(tree, n, ptr(r), ptr(o), fp_mode, ptr(ro), workspace, nbytes, None)
    return rc, (L.vr_last_error() or b"").decode()


def test_invalid_arguments_through_c(L):
    for kw in (dict(tree=None), dict(rays=None), dict(rays=(None, D)), dict(rays=(O, None)), dict(opt=None),
               dict(out=None), dict(order=None)):
        rc, msg = _call(L, **kw)
        assert rc == INVALID and "NULL" in msg and NAME in msg, kw
    for fp in (2, -1, 9):
        rc, msg = _call(L, fp_mode=fp)
        assert rc == INVALID and "fp_mode" in msg and NAME in msg
    for n in (-1, 1 << 30, 1 << 40):
        rc, msg = _call(L, n=n)
        assert rc == INVALID and "n=" in msg and NAME in msg
    for bits in (-1, 6, 32):
        rc, msg = _call(L, bits=bits)
        assert rc == INVALID and "bits" in msg and NAME in msg
    for kw in (dict(payload=None), dict(payload_out=None)):
        rc, msg = _call(L, **kw)
        assert rc == INVALID and "payload" in msg and NAME in msg, kw
    for kw in (dict(payload_dim=0), dict(payload_dim=9), dict(payload_dim=-1),
               dict(payload=None, payload_out=None, payload_dim=3)):
        rc, msg = _call(L, **kw)
        assert rc == INVALID and "payload_dim" in msg and NAME in msg, kw
    need = L.vr_order_rays_workspace(100)
    for kw in (dict(workspace=None), dict(nbytes=need - 1), dict(nbytes=0), dict(workspace=WS + 64)):
        rc, msg = _call(L, **kw)
        assert rc == INVALID and "workspace" in msg and NAME in msg, kw
    for kw in (dict(origins_out=O), dict(dirs_out=D), dict(payload_out=P)):
        rc, msg = _call(L, **kw)
        assert rc == INVALID and "input" in msg and NAME in msg, kw
    # n == 0 still checks its arguments -- and then needs no workspace
    assert _call(L, n=0, rays=(None, D))[0] == INVALID
    assert _call(L, n=0, opt=None)[0] == INVALID
    assert _call(L, n=0, order=None)[0] == INVALID
    assert _call(L, n=0, bits=7)[0] == INVALID
    assert _call(L, n=0, workspace=None, nbytes=0)[0] == 0


def test_optional_outputs_are_not_what_is_refused(L):
    """keys / origins_out / dirs_out / payload = NULL pass the argument checks: what is refused next is the workspace."""
    for kw in (dict(keys=None), dict(origins_out=None), dict(dirs_out=None),
               dict(payload=None, payload_out=None, payload_dim=0),
               dict(keys=None, origins_out=None, dirs_out=None, payload=None, payload_out=None, payload_dim=0)):
        rc, msg = _call(L, workspace=None, **kw)
        assert rc == INVALID and "workspace" in msg, kw


def test_refusals_through_cpp(L, tmp_path):
    got = build_util.run_key_values(build_util.cpp_program("order_refusals", tmp_path), refusals=True)
    words = {"null_origins": "NULL", "null_dirs": "NULL", "null_order": "NULL", "fp_mode": "fp_mode",
             "n_negative": "n=", "n_large": "n=", "bits_negative": "bits", "bits_large": "bits",
             "payload_without_out": "payload", "out_without_payload": "payload", "payload_dim_large": "payload_dim",
             "payload_dim_zero": "payload_dim", "payload_dim_without_payload": "payload_dim",
             "null_workspace": "workspace", "small_workspace": "workspace", "misaligned_workspace": "workspace",
             "origins_in_place": "input", "dirs_in_place": "input", "payload_in_place": "input", "null_tree": "NULL"}
    assert got.pop("n_zero") == "OK"
    assert sorted(got) == sorted(words)
    for case, text in got.items():
        assert text.startswith(f"runtime_error: {NAME}:") and words[case] in text, (case, text)


def test_optimizers_take_reorder():
    pytest.importorskip("torch")
    import inspect

    from volrend_amd import api, optim
    assert api.N3Tree.order_rays is api.order_rays
    for cls in (optim.SparseTreeOptimizer, optim.TreeRays):
        p = inspect.signature(cls.__init__).parameters["reorder"]
        assert p.default is optim.REORDER_DEFAULT and isinstance(p.default, bool)
