"""Cross-check of the oracle against the reference's OTHER backend: shaders/rt.frag (read
from the reference mount at run time) executed on a software GL rasteriser
(oracle/ref_build/rtfrag_baseline.py).  The GLSL path differs from the CUDA path by
documented rounding details (UNORM8 rounds to nearest, exp/pow in the
rasteriser's own precision), so agreement is PSNR-level: > 45 dB, no pixel off by more than 2.
The rt.frag frame is stored in tests/golden/ref_frames_v1.npz (tests/common.py ref_array); where
the reference mount and SwiftShader are present it is rendered again and must equal the stored one."""
import json
import os
import subprocess
import sys

import numpy as np

from tests.common import ob, ref_array
from volrend_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "oracle", "ref_build", "rtfrag_baseline.py")


def available():
    if not os.path.exists("/root/reference/shaders/rt.frag"):
        return False
    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_build"))
    import rtfrag_baseline
    return rtfrag_baseline.find_swiftshader() is not None


def test_rt_frag_agrees_with_oracle(request, tmp_path):
    size, pose = 64, 37

    def rt_frag():
        out = str(tmp_path / "r.json")
        subprocess.check_call([sys.executable, SCRIPT, "--size", str(size), "--pose", str(pose), "--out", out],
                              stdout=subprocess.DEVNULL, timeout=600)
        assert json.load(open(out))["gl_error"] == 0
        from PIL import Image
        return np.asarray(Image.open(str(tmp_path / "r_rtfrag.png")).convert("RGBA"))
    # the CUDA-path semantics on the same inputs (what rtfrag_baseline.py compares with)
    cfg = synth.CONFIGS["C0"]
    tree = synth.make_config_tree("C0")
    tr = synth.c2w_to_transform(synth.make_poses(200)[pose])
    cam = ob.make_camera(tr, size, size, cfg["focal"] * size / cfg["width"])
    want, _, cnt = ob.render(ob.TreeHandle(tree), cam, ob.default_options(), want_accum=False)
    img = ref_array(request.node.name + "/rgba", rt_frag, available=available())
    d = np.abs(img[..., :3].astype(int) - want[..., :3].astype(int))
    mse = float(np.mean(d.astype(np.float64) ** 2))
    assert mse == 0.0 or 10 * np.log10(255.0 ** 2 / mse) > 45.0
    assert d.max() <= 2 and int((d > 2).any(-1).sum()) == 0
    assert cnt["samples"] > 10000
