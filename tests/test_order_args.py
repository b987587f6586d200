"""The argument checks of ``order_rays``, with no GPU and no library, in the manner of tests/test_api_args.py: every
buffer argument is given every defect in turn and must be refused with a ValueError that names it -- before any C
call (the library is a stub that fails on any access), and before the tree is asked anything unless the defect is the
device index; then the arguments that are not buffers."""
import numpy as np
import pytest

from tests import common
from tests.test_api_args import _Cai, _StubLib, stub_lib  # noqa: F401  (the autouse fixture: the library is a stub)
from volrend_amd import api

N_RAYS, K = 100, 3
_O = api.RenderOptions()
# argument -> (dtype, shape, how the call receives it)
ARGS = {
    "origins": ("float32", (N_RAYS, 3)), "dirs": ("float32", (N_RAYS, 3)), "payload": ("float32", (N_RAYS, K)),
    "order": ("int32", (N_RAYS,)), "keys": ("int32", (N_RAYS,)), "origins_out": ("float32", (N_RAYS, 3)),
    "dirs_out": ("float32", (N_RAYS, 3)), "payload_out": ("float32", (N_RAYS, K)), "workspace": ("uint8", (1 << 20,)),
}
OUT_KEY = {"order": "order", "keys": "keys", "origins_out": "origins", "dirs_out": "dirs", "payload_out": "payload"}
WRONG_DTYPE = {"float32": "float64", "int32": "int64", "uint8": "int8"}


def _call(tree, a, **kw):
    out = {OUT_KEY[k]: a[k] for k in OUT_KEY if a.get(k) is not None}
    return api.order_rays(tree, a["origins"], a["dirs"], _O, payload=a.get("payload"), out=out,
                          workspace=a.get("workspace"), **dict(dict(n=N_RAYS, payload_dim=K), **kw))


def _valid(others):
    if others == "pointers":
        return {name: 0x5000 + 0x1000 * i for i, name in enumerate(ARGS)}
    return {name: common.FakeCudaTensor(shape, dt, ptr=0x5000 + 0x1000 * i) for i, (name, (dt, shape)) in enumerate(ARGS.items())}


def _defects(arg):
    dtype, shape = ARGS[arg]
    exact = arg != "workspace"
    bad_shape = shape[:-1] + (shape[-1] + 1,)
    good = dict(shape=shape, dtype=dtype)
    yield "kind: list", [0.0, 1.0, 2.0], 0
    yield "kind: numpy", np.zeros(shape, dtype), 0
    yield "kind: bool", True, 0
    yield "dtype", common.FakeCudaTensor(shape, WRONG_DTYPE[dtype]), 0
    if exact:
        yield "shape", common.FakeCudaTensor(bad_shape, dtype), 0
        if len(shape) > 1:
            yield "shape: flat", common.FakeCudaTensor((int(np.prod(shape)),), dtype), 0
    yield "not contiguous", common.FakeCudaTensor(contiguous=False, **good), 0
    yield "host (fake)", common.FakeCudaTensor(is_cuda=False, **good), 0
    yield "other device", common.FakeCudaTensor(index=1, **good), 1
    cai = dict(shape=shape, typestr={"float32": "<f4", "int32": "<i4", "uint8": "|u1"}[dtype], data=(0x9000, False),
               version=3)
    yield "interface: dtype", _Cai(dict(cai, typestr="<f8", strides=None)), 0
    if exact:
        yield "interface: shape", _Cai(dict(cai, shape=bad_shape, strides=None)), 0
    yield "interface: strides", _Cai(dict(cai, strides=tuple(8 for _ in shape))), 0


@pytest.mark.parametrize("others", ["tensors", "pointers"])
@pytest.mark.parametrize("arg", list(ARGS))
def test_every_defect_of_every_buffer_is_refused_by_name(arg, others):
    for label, bad, info_calls in _defects(arg):
        tree = common.FakeTree(info=0)
        a = dict(_valid(others), **{arg: bad})
        with pytest.raises(ValueError, match=arg) as e:
            _call(tree, a)
        assert str(e.value).startswith(arg + " "), (label, str(e.value))    # (origins_out is not origins)
        assert tree.info_calls <= info_calls, (label, tree.info_calls)


def test_arguments_that_are_not_buffers():
    t = common.FakeTree()
    a = _valid("pointers")

    def refused(match, args=a, **kw):
        with pytest.raises(ValueError, match=match):
            _call(t, args, **kw)
    for bits in (-1, 6, 2.0, True, None):
        refused("bits", bits=bits)
    refused("want", want=("order", "rgba"))
    refused("want", want=("keys", "keys"))
    refused("payload", args=dict(a, payload=None))                              # payload_out without a payload
    refused("payload", args=dict(a, payload=None, payload_out=None))            # payload_dim without a payload
    refused("payload", args=dict(a, payload=None, payload_out=None), payload_dim=None, want=("payload",))
    refused("payload_dim", payload_dim=None)                                    # a raw pointer has no width
    for k in (0, 9, -3):
        refused("columns", payload_dim=k)
    refused("columns", args=dict(a, payload=common.FakeCudaTensor((N_RAYS, 9))), payload_dim=None)
    refused("pass n", n=None)
    refused("own input", args=dict(a, origins_out=a["origins"]))
    refused("own input", args=dict(a, dirs_out=a["dirs"]))
    refused("own input", args=dict(a, payload_out=a["payload"]))
    with pytest.raises(ValueError, match="out names"):
        api.order_rays(t, a["origins"], a["dirs"], _O, out={"rgba": 0x9000}, n=N_RAYS)
    assert t.info_calls == 0


def test_a_tree_that_is_not_on_the_device_is_refused_first():
    class NoHandle:
        @property
        def handle(self):
            raise RuntimeError("tree is not on the device")
    with pytest.raises(RuntimeError, match="not on the device"):
        api.order_rays(NoHandle(), None, None, _O)
