"""The argument checks of the Python API, with no GPU and no library: every buffer argument of every operation is
given every defect in turn, and must be refused with a ValueError that names it -- before any C call (the library is
a stub that fails on any access), and before the tree is asked anything unless the defect is the device index."""
import subprocess
import sys

import numpy as np
import pytest

from tests import common
from volrend_amd import _abi, api

try:
    import torch
except ImportError:     # (the fake-tensor cases need none)
    torch = None

N_RAYS, W, H, POSES = 100, 64, 48, 2
TR = np.zeros(12, np.float32)


class _StubLib:
    touched = 0

    def __getattr__(self, name):
        _StubLib.touched += 1
        raise AssertionError(f"the library must not be called (vr lib attribute {name!r})")


@pytest.fixture(autouse=True)
def stub_lib(monkeypatch):
    _StubLib.touched = 0
    monkeypatch.setattr(_abi, "lib", lambda: _StubLib())
    yield
    assert _StubLib.touched == 0, "the library was touched"


def _shape(tree, what):
    """(shape, exact) of a buffer kind; exact False: any shape with that many elements."""
    leaf = (tree.capacity, tree.N, tree.N, tree.N)
    return {"rays3": ((N_RAYS, 3), True), "rays4": ((N_RAYS, 4), True), "leaf": (leaf, True),
            "frames": ((POSES, H, W, 4), True), "grad": (leaf + (tree.data_dim,), True),
            "data": (leaf + (tree.data_dim,), False), "words": ((api.touched_words(tree),), False)}[what]


def _cam():
    return api.Camera(W, H, 50.0, 50.0)


_O = api.RenderOptions()
# operation -> (call(tree, args), {argument: (dtype, buffer kind)}); the argument names are those of the messages
OPS = {
    "query": (lambda t, a: api.query_points(t, a["points"], a["dirs"], want=("sigma", "rgb"), n=N_RAYS),
              {"points": ("float32", "rays3"), "dirs": ("float32", "rays3")}),
    "accumulate_weights": (lambda t, a: api.accumulate_weights(t, _cam(), [TR] * POSES, _O, **a),
                           {"max_weight": ("float32", "leaf"), "hits": ("int32", "leaf")}),
    "render_backward": (lambda t, a: api.render_backward(t, _cam(), [TR] * POSES, _O, a["grad_accum"],
                                                         grad_data=a["grad_data"], touched=a["touched"]),
                        {"grad_accum": ("float32", "frames"), "grad_data": ("float32", "grad"),
                         "touched": ("int32", "words")}),
    "render_rays": (lambda t, a: api.render_rays(t, a["origins"], a["dirs"], _O, rgba=a["rgba"], accum=a["accum"],
                                                 n=N_RAYS),
                    {"origins": ("float32", "rays3"), "dirs": ("float32", "rays3"), "rgba": ("uint8", "rays4"),
                     "accum": ("float32", "rays4")}),
    "accumulate_weights_rays": (lambda t, a: api.accumulate_weights_rays(
        t, a["origins"], a["dirs"], _O, max_weight=a["max_weight"], hits=a["hits"], n=N_RAYS),
        {"origins": ("float32", "rays3"), "dirs": ("float32", "rays3"), "max_weight": ("float32", "leaf"),
         "hits": ("int32", "leaf")}),
    "render_backward_rays": (lambda t, a: api.render_backward_rays(
        t, a["origins"], a["dirs"], _O, a["grad_accum"], grad_data=a["grad_data"], touched=a["touched"], n=N_RAYS),
        {"origins": ("float32", "rays3"), "dirs": ("float32", "rays3"), "grad_accum": ("float32", "rays4"),
         "grad_data": ("float32", "grad"), "touched": ("int32", "words")}),
    "update_data": (lambda t, a: api.update_data(t, a["data"]), {"data": ("float16", "data")}),
    "read_data": (lambda t, a: api.read_data(t, out=a["out"]), {"out": ("float32", "data")}),
    "tree_step": (lambda t, a: api.tree_step(t, a["master"], a["grad"], a["touched"], kind="adam", lr=0.1, m=a["m"],
                                             v=a["v"]),
                  {"master": ("float32", "data"), "grad": ("float32", "data"), "m": ("float32", "data"),
                   "v": ("float32", "data"), "touched": ("int32", "words")}),
}
CASES = [(op, arg) for op, (_, args) in OPS.items() for arg in args]
WRONG_DTYPE = {"float32": "float64", "float16": "float64", "int32": "int64", "uint8": "int8"}


def _defects(tree, dtype, what):
    """(label, defective value, info() calls allowed) for one argument."""
    shape, exact = _shape(tree, what)
    bad_shape = shape[:-1] + (shape[-1] + 1,)
    good = dict(shape=shape, dtype=dtype)
    yield "kind: list", [0.0, 1.0, 2.0], 0
    yield "kind: numpy", np.zeros(shape, dtype), 0
    yield "kind: bool", True, 0
    yield "dtype", common.FakeCudaTensor(shape, WRONG_DTYPE[dtype]), 0
    yield "shape" if exact else "count", common.FakeCudaTensor(bad_shape, dtype), 0
    if exact:
        yield "shape: flat", common.FakeCudaTensor((int(np.prod(shape)),), dtype), 0
    yield "not contiguous", common.FakeCudaTensor(contiguous=False, **good), 0
    yield "host (fake)", common.FakeCudaTensor(is_cuda=False, **good), 0
    if torch is not None:
        yield "host (torch)", torch.zeros(shape, dtype=getattr(torch, dtype)), 0
    yield "other device", common.FakeCudaTensor(index=1, **good), 1
    cai = dict(shape=shape, typestr={"float32": "<f4", "float16": "<f2", "int32": "<i4", "uint8": "|u1"}[dtype],
               data=(0x9000, False), version=3)
    yield "interface: dtype", _Cai(dict(cai, typestr="<f8", strides=None)), 0
    yield "interface: shape", _Cai(dict(cai, shape=bad_shape, strides=None)), 0
    yield "interface: strides", _Cai(dict(cai, strides=tuple(8 for _ in shape))), 0


class _Cai:
    def __init__(self, d):
        self.__cuda_array_interface__ = d


def _valid(tree, args, others):
    if others == "pointers":
        return {name: 0x5000 + 0x100 * i for i, name in enumerate(args)}
    return {name: common.FakeCudaTensor(_shape(tree, what)[0], dt) for name, (dt, what) in args.items()}


@pytest.mark.parametrize("others", ["tensors", "pointers"])
@pytest.mark.parametrize("op,arg", CASES, ids=[f"{op}-{arg}" for op, arg in CASES])
def test_every_defect_of_every_buffer_argument_is_refused(op, arg, others):
    call, args = OPS[op]
    tree = common.FakeTree(info=0)
    for label, bad, info_calls in _defects(tree, *args[arg]):
        tree.info_calls = 0
        with pytest.raises(ValueError) as e:
            call(tree, dict(_valid(tree, args, others), **{arg: bad}))
        assert str(e.value).startswith(arg + " "), (label, str(e.value))   # names the argument
        assert tree.info_calls == info_calls, (label, tree.info_calls, str(e.value))


@pytest.mark.parametrize("op,arg", CASES, ids=[f"{op}-{arg}" for op, arg in CASES])
def test_a_host_tensor_is_refused_before_the_tree_is_asked_even_next_to_one_on_another_device(op, arg):
    """Steps 1-5 run for all arguments before the device index of any is compared."""
    call, args = OPS[op]
    tree = common.FakeTree(info="raises")
    shape, dt = _shape(tree, args[arg][1])[0], args[arg][0]
    elsewhere = {name: common.FakeCudaTensor(_shape(tree, what)[0], d, index=1) for name, (d, what) in args.items()}
    with pytest.raises(ValueError, match=arg):
        call(tree, dict(elsewhere, **{arg: common.FakeCudaTensor(shape, dt, is_cuda=False)}))
    assert tree.info_calls == 0


def test_raw_pointers_and_interfaces_pass_the_checks_and_the_tree_is_asked_at_most_once():
    """Valid arguments get as far as the library (here: the stub's AssertionError).  Tensors cost one info() call
    however many there are; raw pointers and __cuda_array_interface__ objects none when nothing is allocated."""
    typestr = {"float32": "<f4", "float16": "<f2", "int32": "<i4", "uint8": "|u1"}
    for op, (call, args) in OPS.items():
        if op == "query":   # (allocates its outputs: needs a device)
            continue
        tree = common.FakeTree(info=0)
        cais = {name: _Cai(dict(shape=_shape(tree, what)[0], typestr=typestr[dt], data=(0x9000, False), strides=None,
                                version=3)) for name, (dt, what) in args.items()}
        for passed, asked in ((_valid(tree, args, "tensors"), 1), (_valid(tree, args, "pointers"), 0), (cais, 0)):
            tree.info_calls = 0
            with pytest.raises(AssertionError, match="library must not be called"):
                call(tree, passed)
            assert tree.info_calls == asked, (op, tree.info_calls)
    _StubLib.touched = 0    # (this test went as far as the stub on purpose)


def test_tensor_rays_give_n_to_raw_pointer_outputs_and_gradients():
    """A ray list of tensors carries its n: raw-pointer outputs / gradients next to it need no ``n`` and get as far
    as the library."""
    tree = common.FakeTree(info=0)
    o, d = common.FakeCudaTensor((N_RAYS, 3)), common.FakeCudaTensor((N_RAYS, 3))
    for call in (lambda: api.render_rays(tree, o, d, _O, accum=0x5000),
                 lambda: api.render_rays(tree, o, d, _O, want=(), rgba=0x5000),
                 lambda: api.render_rays(tree, o, d, _O, rgba=0x5000, accum=0x6000),
                 lambda: api.render_backward_rays(tree, o, d, _O, 0x5000, grad_data=0x6000),
                 lambda: api.accumulate_weights_rays(tree, o, d, _O, max_weight=0x5000, hits=0x6000)):
        with pytest.raises(AssertionError, match="library must not be called"):
            call()
    for call in (lambda: api.render_rays(tree, 0x4000, d, _O, accum=0x5000),     # a pointer in the list itself
                 lambda: api.render_backward_rays(tree, o, 0x4000, _O, 0x5000, grad_data=0x6000)):
        with pytest.raises(ValueError, match="pass n"):
            call()
    with pytest.raises(ValueError, match="n is negative"):
        api.render_rays(tree, 0x4000, 0x4100, _O, accum=0x5000, n=-1)
    _StubLib.touched = 0    # (this test went as far as the stub on purpose)


def test_bool_is_no_raw_pointer_and_ray_lists_of_pointers_need_n():
    tree = common.FakeTree(info="raises")
    with pytest.raises(ValueError, match="points"):
        api.query_points(tree, True, n=4)
    for call in (lambda: api.query_points(tree, 0x5000),
                 lambda: api.render_rays(tree, 0x5000, 0x6000, _O),
                 lambda: api.accumulate_weights_rays(tree, 0x5000, 0x6000, _O),
                 lambda: api.render_backward_rays(tree, 0x5000, 0x6000, _O, 0x7000, grad_data=0x8000)):
        with pytest.raises(ValueError, match="pass n"):
            call()
    with pytest.raises(ValueError, match="want"):
        api.query_points(tree, 0x5000, n=4, want=())
    with pytest.raises(ValueError, match="want"):
        api.render_rays(tree, 0x5000, 0x6000, _O, n=4, want=("accum", "accum"))
    with pytest.raises(ValueError, match="want"):
        api.accumulate_weights_rays(tree, 0x5000, 0x6000, _O, n=4, want="weights")


METHODS = {"query": "query_points", "query_grid": "query_grid", "accumulate_weights": "accumulate_weights",
           "render_backward": "render_backward", "render_rays": "render_rays",
           "accumulate_weights_rays": "accumulate_weights_rays", "render_backward_rays": "render_backward_rays",
           "touched_words": "touched_words", "step": "tree_step", "update_data": "update_data",
           "read_data": "read_data"}


def test_the_methods_are_the_module_functions():
    assert len(METHODS) == 11
    for method, function in METHODS.items():
        assert getattr(api.N3Tree, method) is getattr(api, function), method
    for text in (open(m.__file__).read() for m in (api, sys.modules["volrend_amd._ops"], sys.modules["volrend_amd._tree"])):
        assert "documented there" not in text


def test_both_spellings_reach_the_same_refusal():
    class Loaded(api.N3Tree):       # a real N3Tree whose handle is never followed
        handle = common.FakeTree.HANDLE

        def info(self):
            return {"device": 0}

    t = Loaded.from_synth(common.small_scene(depth=2, basis_dim=4, seed=1), upload=False)
    bad = common.FakeCudaTensor((N_RAYS, 3), "float64")
    good = common.FakeCudaTensor((N_RAYS, 3))
    pairs = [(lambda: t.query(bad), lambda: api.query_points(t, bad)),
             (lambda: t.render_rays(good, bad, _O), lambda: api.render_rays(t, good, bad, _O)),
             (lambda: t.accumulate_weights_rays(bad, good, _O), lambda: api.accumulate_weights_rays(t, bad, good, _O)),
             (lambda: t.render_backward_rays(good, good, _O, bad), lambda: api.render_backward_rays(t, good, good, _O, bad)),
             (lambda: t.accumulate_weights(_cam(), [TR], _O, hits=bad),
              lambda: api.accumulate_weights(t, _cam(), [TR], _O, hits=bad)),
             (lambda: t.render_backward(_cam(), [TR], _O, bad), lambda: api.render_backward(t, _cam(), [TR], _O, bad)),
             (lambda: t.update_data(bad), lambda: api.update_data(t, bad)),
             (lambda: t.read_data(out=bad), lambda: api.read_data(t, out=bad)),
             (lambda: t.step(bad, good, good, lr=0.1), lambda: api.tree_step(t, bad, good, good, lr=0.1)),
             (lambda: t.query_grid((0, 0, 0), (1, 1, 1), (2.5, 2, 2)),
              lambda: api.query_grid(t, (0, 0, 0), (1, 1, 1), (2.5, 2, 2)))]
    for method, function in pairs:
        with pytest.raises(ValueError) as a:
            method()
        with pytest.raises(ValueError) as b:
            function()
        assert str(a.value) == str(b.value)
    assert t.touched_words() == api.touched_words(t) == (t.capacity * t.N ** 3 + 31) // 32


def test_a_tree_that_is_not_on_the_device_is_refused_first_by_every_operation():
    t = api.N3Tree.from_synth(common.small_scene(depth=2, basis_dim=4, seed=1), upload=False)
    bad = [1.0, 2.0]    # no buffer at all: would be a ValueError
    calls = [lambda: t.query(bad), lambda: t.query_grid(bad, bad, bad),
             lambda: t.accumulate_weights(_cam(), [TR], _O, max_weight=bad, want=("nothing",)),
             lambda: t.render_backward(_cam(), [TR], _O, bad, grad_data=bad, touched=bad),
             lambda: t.render_rays(bad, bad, _O, want=("nothing",)),
             lambda: t.accumulate_weights_rays(bad, bad, _O, hits=bad),
             lambda: t.render_backward_rays(bad, bad, _O, bad, touched=bad),
             lambda: t.touched_words(), lambda: t.step(bad, bad, bad, kind="rmsprop", lr=0.1),
             lambda: t.update_data(bad), lambda: t.read_data(dtype="int8", out=bad),
             lambda: api.tree_step(t, bad, bad, bad, lr=0.1), lambda: api.render_rays(t, bad, bad, _O)]
    assert len(calls) == 11 + 2
    for call in calls:
        with pytest.raises(RuntimeError, match="not on the device"):
            call()


def test_importing_the_api_does_not_import_torch():
    code = "import sys, volrend_amd.api; assert 'torch' not in sys.modules, 'torch was imported'"
    subprocess.check_call([sys.executable, "-c", code], cwd=common.GOLDEN + "/../..")
