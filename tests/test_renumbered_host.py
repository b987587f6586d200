"""common.renumbered is what it claims (no GPU): the renumbered tree is the same scene to the oracle and to the
leaf-weight restatement, its orphans are out of every ray's reach, and the host statement of svox's parent_depth
follows the rule of vr_tree_geometry on every kind of it."""
import numpy as np
import pytest

from tests import common, geometry_util as gg, renumber_util as rn, weights_util as wu
from volrend_amd import _tree


def test_the_kinds_do_what_they_say():
    tree = rn.base("sh9")
    cap, rows = tree.capacity, common.rows_of(tree)
    level = common.node_levels(rows)
    assert (level >= 0).all() and not (rows < 0).any()               # breadth-first, forward, nothing unreachable
    rev, new_of = common.renumbered(tree, ["reversed"])
    r = common.rows_of(rev)
    assert np.array_equal(new_of[1:], cap - np.arange(1, cap)) and new_of[0] == 0
    assert (r[1:][r[1:] != 0] < 0).all() and (r != 0).sum() == (rows != 0).sum()      # every link below the root: backward
    assert np.array_equal(rev.data[new_of], tree.data)
    rnd, new_of = common.renumbered(tree, ["random"], seed=7)
    assert np.array_equal(common.rows_of(rnd), common.scrambled(rows, 7)[0]) and (common.rows_of(rnd) < 0).any()
    pr, new_of = common.renumbered(tree, ["pruned"])
    p = common.rows_of(pr)
    cut = np.argwhere(p != rows)
    assert cut.shape == (1, 2) and p[tuple(cut[0])] == 0 and level[cut[0, 0]] == 1   # one slot of depth 2
    lost = common.orphan_nodes(pr)
    assert lost.sum() >= 8 and np.array_equal(pr.data, tree.data) and np.array_equal(new_of, np.arange(cap))
    top = cut[0, 0] + rows[tuple(cut[0])]
    assert lost.sum() == common.subtree_sizes(rows)[top] and (p[lost] != 0).sum() == lost.sum() - 1   # linked among itself
    assert np.flatnonzero(lost).min() < cap - lost.sum()             # not a tail: in the middle of the array
    z, _ = common.renumbered(tree, ["slack_zero"])
    assert z.capacity == cap + 7 and not z.child[cap:].any() and not z.data[cap:].any()
    assert np.array_equal(z.child[:cap], tree.child)
    sl, _ = common.renumbered(tree, ["slack_linked"])
    s = common.rows_of(sl)
    assert sl.capacity == cap + 5 and np.array_equal(s, np.concatenate([common.with_unreachable(rows)[:-1], s[-1:]]))
    tgt = (np.arange(cap + 5)[:, None] + s)[s != 0]
    assert (tgt == 1).sum() == 2 and ((tgt < 1) | (tgt >= cap + 5)).sum() == 1        # node 1 twice; one link leaves
    assert (sl.data[cap:, ..., :-1] == 3.0).all() and (sl.data[cap:, ..., -1] == 200.0).all()
    for t in (rev, rnd, pr, z, sl):
        assert t.extra is tree.extra and t.offset is tree.offset and t.invradius3 is tree.invradius3
        assert t.data_format == tree.data_format and t.data.dtype == np.float16 and t.child.dtype == np.int32


@pytest.mark.parametrize("scene", sorted(rn.SCENES))
def test_combined_tree_is_the_same_scene(scene):
    """random + pruned + slack_linked: the oracle's frame and the restated leaf weights of the renumbered tree are
    those of the pruned original, bit for bit, through new_of; no ray reaches an orphan."""
    c = rn.case(scene, rn.COMBINED)
    tree, orig, new_of = c["tree"], c["orig"], c["new_of"]
    assert c["orphan"].sum() >= 8 + 5 and (tree.child < 0).any()
    trs, w, h, f = rn.views()
    for tr in trs:
        a, b = common.oracle_frame(tree, tr, w, h, f), common.oracle_frame(orig, tr, w, h, f)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
        assert a[0][..., :3].any()
    mw2, hc2, _ = wu.restate(tree, trs, w, h, f)
    mw, hc, _ = wu.restate(orig, trs, w, h, f)
    assert wu.bits(mw2).tobytes() == wu.bits(rn.carry(mw, new_of, tree.capacity)).tobytes()
    assert np.array_equal(hc2, rn.carry(hc, new_of, tree.capacity))
    assert not mw2[c["orphan"]].any() and not hc2[c["orphan"]].any()
    assert (hc2 > 0).sum() >= 100, "the frames hit too few slots to show anything"


KINDS = [("random",), ("reversed",), ("pruned",), ("slack_zero",), ("pruned", "reversed"), rn.RAW]


@pytest.mark.parametrize("kinds", KINDS, ids="+".join)
@pytest.mark.parametrize("scene", ["sh9", "n3"])
def test_parent_depth_host_follows_the_header(scene, kinds):
    """_parent_depth_host (what save() writes for a tree that is not on the device) is vr_tree_geometry's parent_slot
    and node_depth, with the root's row (0, 0): an orphan that another orphan links to names that slot, depth -1."""
    tree = rn.case(scene, kinds)["tree"]
    rows = common.rows_of(tree)
    parent, depth, _ = gg.restate(rows)
    want = np.stack([parent, depth], axis=1)
    want[0] = 0
    got = _tree._parent_depth_host(tree.child)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if "pruned" in kinds:
        chained = (got[:, 1] < 0) & (got[:, 0] >= 0)
        assert chained.sum() >= 7                                     # the orphan chain: a slot, and depth -1
    down = gg.walk_down(rows)
    assert all(tuple(got[m]) == (down[m][0], down[m][1]) for m in down if m)
