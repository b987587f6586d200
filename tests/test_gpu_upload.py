"""-m gpu: the staged host-to-device copy pipeline of an upload (volrend_amd/csrc/vr_h2d.cpp).  It starts
at 32 MB, above every other tree of the suite."""
import re

import numpy as np
import pytest

from tests import common, query_util as qu
from tests.common import ob
from tests.query_util import gpu_query, same_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def test_staged_upload_delivers_every_leaf(torch_cuda, monkeypatch, capfd):
    """The smallest tree that makes the pipeline do everything it can do: 37,481 nodes of 76 halfs per
    slot = child 1.14 MB + data 43.47 MB.  That is 1 + 22 chunks of 2 MB for at most 4 workers x 2 slots
    (every slot is reused and waits on its event), and both segments end in a short chunk (1,199,392 and
    1,536,704 bytes).  The `staged H2D:` line shows that the pipeline ran (no line: the plain copy ran,
    and the test fails); then every one of the 262,368 leaves is queried at its centre and compared with
    the oracle word for word, which ties the staged bytes, the renumbering, the re-layout and the lookup
    structure to the file; and one frame equals the oracle's."""
    from volrend_amd import api
    torch = torch_cuda
    tree = common.small_scene(depth=7, basis_dim=25, seed=431)
    assert (tree.capacity, tree.data_dim) == (37481, 76)
    assert tree.child.nbytes % (2 << 20) == 1199392 and tree.data.nbytes % (2 << 20) == 1536704
    assert tree.child.nbytes + tree.data.nbytes >= 32 << 20

    monkeypatch.setenv("VR_UPLOAD_TIMING", "1")
    capfd.readouterr()
    t = api.N3Tree.from_synth(tree)
    err = capfd.readouterr().err
    monkeypatch.delenv("VR_UPLOAD_TIMING")
    m = re.search(r"staged H2D: ([0-9.]+) MB in (\d+) segments, (\d+) workers", err)
    assert m, f"the plain copy ran, not the staged pipeline:\n{err}"
    assert abs(float(m.group(1)) - (tree.child.nbytes + tree.data.nbytes) / 1e6) < 0.06
    assert int(m.group(2)) == 2 and int(m.group(3)) >= 2, m.group(0)

    corners, sizes, depths, slots = qu.leaf_boxes(tree)
    assert slots.size == 262368 and np.unique(slots).size == slots.size
    centres = (corners + 0.5 * sizes[:, None]).astype(np.float32)
    ans = qu.oracle_answers(tree, ob.TreeHandle(tree), centres, "tree")
    assert np.array_equal(ans["leaf"], slots)                # the oracle finds each leaf at its centre
    got = gpu_query(torch, t, centres, space="tree")
    for k in ("sigma", "depth", "local", "coeffs"):
        same_words(got[k], ans[k], f"staged upload, {k}")

    tr, w, h, f = common.camera_for(pose_idx=3, size=96)
    cam = api.Camera(w, h, f, f)
    cam.transform = np.asarray(tr, dtype=np.float32)
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    api.launch_renderer(t, cam, api.RenderOptions(), img, None, torch.cuda.current_stream(), True, accum=acc)
    torch.cuda.synchronize()
    assert t.status() == 0
    rgba_o, acc_o, _ = common.oracle_frame(tree, tr, w, h, f)
    assert np.array_equal(img.cpu().numpy(), rgba_o)
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), acc_o.view(np.uint32))
    t.free_device()
