"""The yardstick of the vr_order_rays tests (tests/order_util.py over tests/cpp/order_restatement.c), tied down
without a GPU: the bit layout of the key on hand-made rays through known cells of the unit box, the quantisation
rule on values, the tie to the oracle's ray/box test, and the result rule."""
import numpy as np
import pytest

from tests import order_util as ou
from tests import rays_util as ru

F32 = np.float32
# axis-parallel rays through the unit box (tree coordinates = world coordinates: ou.unit_tree), directions of any
# length: (origin, direction, entry cell and exit cell in eighths / halves / 32nds come from these points)
#   the box test moves a face by 1e-6 inwards: an entry at x = 0 is 1e-6, an exit at x = 1 is 1 - 1e-6
RAYS = {
    "plus_x": ((-1.0, 0.3, 0.6), (2.0, 0.0, 0.0), (0.0, 0.3, 0.6), (1.0, 0.3, 0.6)),
    "minus_y": ((0.7, 5.0, 0.2), (0.0, -0.01, 0.0), (0.7, 1.0, 0.2), (0.7, 0.0, 0.2)),
    "inside_minus_z": ((0.5, 0.25, 0.75), (0.0, 0.0, -3.0), (0.5, 0.25, 0.75), (0.5, 0.25, 0.0)),  # entry = origin
}
MISSES = {"beside": ((-1.0, 2.0, 0.5), (1.0, 0.0, 0.0)), "behind": ((2.0, 0.5, 0.5), (1.0, 0.0, 0.0))}


def _cell(v, bits):
    """The cell of a face point: the faces sit 1e-6 inside the box."""
    return int(min(max(np.floor(min(max(v, 1e-6), 1 - 1e-6) * 2 ** bits), 0), 2 ** bits - 1))


@pytest.mark.parametrize("fp_mode", [0, 1])
@pytest.mark.parametrize("bits", [1, 3, 5])
def test_bit_layout_on_hand_made_rays(bits, fp_mode):
    tree = ou.unit_tree()
    o = np.array([r[0] for r in RAYS.values()], F32)
    d = np.array([r[1] for r in RAYS.values()], F32)
    keys, seg = ou.keys_of(tree, o, d, bits, fp_mode, segments=True)
    for i, (name, (_, _, entry, exit_)) in enumerate(RAYS.items()):
        q = [_cell(v, bits) for v in entry + exit_]
        assert int(keys[i]) == ou.morton(q, bits), (name, q, hex(int(keys[i])))
        assert int(keys[i]) < 1 << (6 * bits)                      # the higher bits are zero
        np.testing.assert_allclose(seg[i], entry + exit_, atol=2e-6, err_msg=name)
    assert np.array_equal(seg[2, :3], o[2]), "a ray that starts inside enters at its origin (tmin = 0)"
    # the layout, spelt out once: coordinate c owns bits c, 6 + c, 12 + c, ...
    q = [_cell(v, bits) for v in RAYS["plus_x"][2] + RAYS["plus_x"][3]]
    for c in range(6):
        got = sum(((int(keys[0]) >> (6 * b + c)) & 1) << b for b in range(bits))
        assert got == q[c], (c, got, q)


@pytest.mark.parametrize("fp_mode", [0, 1])
def test_misses_and_a_tree_without_cells(fp_mode):
    tree = ou.unit_tree()
    o = np.array([r[0] for r in MISSES.values()], F32)
    d = np.array([r[1] for r in MISSES.values()], F32)
    assert (ou.keys_of(tree, o, d, 3, fp_mode) == ou.MISS).all()
    o = np.array([r[0] for r in RAYS.values()], F32)
    d = np.array([r[1] for r in RAYS.values()], F32)
    for N in (0, -2):                                              # enable_draw = tree.N > 0: no ray enters
        assert (ou.keys_of(tree, o, d, 3, fp_mode, N=N) == ou.MISS).all()


@pytest.mark.parametrize("fp_mode", [0, 1])
def test_a_narrowed_render_bbox_moves_entry_and_exit(fp_mode):
    tree = ou.unit_tree()
    o = np.array([RAYS["plus_x"][0], (-1.0, 0.3, 0.75)], F32)
    d = np.array([RAYS["plus_x"][1]] * 2, F32)
    keys, seg = ou.keys_of(tree, o, d, 5, fp_mode, segments=True, render_bbox=ou.NARROW_BBOX)
    np.testing.assert_allclose(seg[0], (0.1, 0.3, 0.6, 0.8, 0.3, 0.6), atol=2e-6)
    # 0.1 * 32 = 3.2, 0.8 * 32 = 25.6 less a hair, 0.3 * 32 = 9.6, 0.6 * 32 = 19.2
    assert int(keys[0]) == ou.morton([3, 9, 19, 25, 9, 19], 5)
    assert keys[1] == ou.MISS                                      # z = 0.75 is outside the narrowed box (z < 0.7)
    assert ou.keys_of(tree, o, d, 5, fp_mode)[1] != ou.MISS        # ... and inside the whole one


def test_quantisation_rule_on_values():
    q = ou.lib().order_quantise
    for bits in (1, 3, 5):
        top = 2 ** bits - 1
        for v, want in ((0.0, 0), (-0.0, 0), (-3.0, 0), (float("-inf"), 0), (float("nan"), 0), (1.0, top), (7.5, top),
                        (float("inf"), top), (np.nextafter(F32(1), F32(0)), top), (0.5, 2 ** (bits - 1)),
                        (np.nextafter(F32(0.5), F32(0)), 2 ** (bits - 1) - 1), (1e-30, 0)):
            assert q(float(v), bits) == want, (bits, v)


@pytest.mark.parametrize("name", ["plain", "bbox", "ndc"])
@pytest.mark.parametrize("fp_mode", [0, 1])
def test_keys_of_seeded_rays(name, fp_mode):
    """On the scenes the GPU tests use: a ray has the miss key exactly when the oracle's ray misses the box; the key
    is the Morton code of the quantised segment; entry and exit lie on faces of the box (an entry may be the
    origin of a ray that starts inside)."""
    tree, ndc, kw = ou.scene(name)
    n = 160
    o, d = ou.rays(name, n)
    bits = 5
    keys, seg = ou.keys_of(tree, o, d, bits, fp_mode, ndc=ndc, segments=True, **kw)
    entered = keys != ou.MISS
    assert 0 < entered.sum() and (name == "ndc" or entered.sum() < n)
    for i in range(0, n, 4):                                       # the oracle, ray by ray (a 2 x 2 camera each)
        hit = ru.oracle_rays(tree, o[i:i + 1], d[i:i + 1], fp_mode, ndc=ndc, **kw)[2]
        assert bool(hit) == bool(entered[i]), i
    box = np.asarray(kw.get("render_bbox", (0, 0, 0, 1, 1, 1)), np.float64)
    for i in np.flatnonzero(entered):
        q = [ou.lib().order_quantise(float(v), bits) for v in seg[i]]
        assert int(keys[i]) == ou.morton(q, bits)
        on_face = lambda p: (np.abs(p - box[:3]).min() < 1e-4) or (np.abs(p - box[3:]).min() < 1e-4)   # noqa: E731
        assert on_face(seg[i, 3:].astype(np.float64)), (i, seg[i])
        inside = ((seg[i, :3] > box[:3] + 1e-4) & (seg[i, :3] < box[3:] - 1e-4)).all()
        assert on_face(seg[i, :3].astype(np.float64)) or inside, (i, seg[i])
    # fewer bits: the key of b bits is the low 6 b bits' worth of cells, i.e. each coordinate shifted down
    k3 = ou.keys_of(tree, o, d, 3, fp_mode, ndc=ndc, **kw)
    for i in np.flatnonzero(entered)[:40]:
        q5 = [ou.lib().order_quantise(float(v), 5) for v in seg[i]]
        assert int(k3[i]) == ou.morton([c >> 2 for c in q5], 3)
    assert ou.DEFAULT_BITS == 2, "what include/volrend_hip.h states for bits == 0"
    assert np.array_equal(ou.keys_of(tree, o, d, 0, fp_mode, ndc=ndc, **kw),
                          ou.keys_of(tree, o, d, ou.DEFAULT_BITS, fp_mode, ndc=ndc, **kw))


def test_result_rule():
    """order = the stable argsort of the keys: a permutation, keys non-decreasing, ties in increasing index, the
    rays that miss at the end in their own order."""
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 7, 500).astype(np.uint32)
    keys[rng.random(500) < 0.2] = ou.MISS
    order, sorted_keys = ou.result_of(keys)
    assert order.dtype == np.uint32 and np.array_equal(np.sort(order), np.arange(500))
    assert (np.diff(sorted_keys.astype(np.int64)) >= 0).all()
    same = sorted_keys[1:] == sorted_keys[:-1]
    assert (np.diff(order.astype(np.int64))[same] > 0).all()
    n_miss = int((keys == ou.MISS).sum())
    assert np.array_equal(order[500 - n_miss:], np.flatnonzero(keys == ou.MISS))
    assert np.array_equal(ou.result_of(np.full(9, ou.MISS))[0], np.arange(9))
