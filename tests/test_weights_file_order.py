"""The device-node -> file-node vector an upload keeps for vr_accumulate_weights
(inverse_permutation, volrend_amd/csrc/vr_tree_walk.cpp): the inverse of what node_permutation returns,
unreachable nodes included.  tests/cpp/walk_inverse_check.cpp is built with plain g++ against that one
source -- no HIP, no library."""
import subprocess

import numpy as np
import pytest

from tests import build_util, common
from tests.common import rows_of, scrambled, with_unreachable


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_util.csrc_program("walk_inverse_check", "vr_tree_walk", tmp_path_factory.mktemp("bin"))


@pytest.mark.parametrize("G0,BL", [(0, 0), (2, 2), (1, 3)])
def test_file_node_vector_is_the_inverse_of_the_renumbering(exe, tmp_path, G0, BL):
    """A small scrambled tree (the renumbering is far from the identity) with five nodes nothing links to."""
    child = with_unreachable(scrambled(rows_of(common.small_scene(depth=4)))[0]).astype(np.int32)
    cap = child.shape[0]
    p = str(tmp_path / "child.bin")
    np.ascontiguousarray(child).tofile(p)
    out = subprocess.check_output([exe, p, str(cap), str(child.shape[1]), str(G0), str(BL)], text=True)
    rows = {l.split()[0]: np.array(l.split()[1:], np.int64) for l in out.splitlines()}
    perm, file_node = rows["perm"], rows["file_node"]
    assert perm.size == file_node.size == cap
    assert np.array_equal(np.sort(perm), np.arange(cap)) and not np.array_equal(perm, np.arange(cap))
    assert np.array_equal(file_node[perm], np.arange(cap))       # device node of file node i maps back to i
    assert np.array_equal(perm[file_node], np.arange(cap))
    # the five unreachable nodes are numbered last on the device, and map back to the file's last five
    assert np.array_equal(file_node[cap - 5:], np.arange(cap - 5, cap))
