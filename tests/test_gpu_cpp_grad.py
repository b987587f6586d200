"""-m gpu: the C++ wrapper volrend::render_backward (include/volrend/grad.hpp) on one tree: tests/cpp/grad_check.cpp
adds four poses in two calls into one buffer and writes it out; it is compared element by element with the
float64 restatement (tests/grad_util.py), within the K of tests/test_gpu_grad.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import grad_util as gu
from volrend_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    subprocess.check_call(["make", "-C", ROOT, "host"], stdout=subprocess.DEVNULL)
    out = str(tmp_path_factory.mktemp("bin") / "grad_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "grad_check.cpp"),
                           os.path.join(ROOT, "volrend_amd", "libvolrend_host.a"),
                           "-L", os.path.join(ROOT, "volrend_amd"), "-lvolrend_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-pthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "volrend_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


@pytest.mark.parametrize("fp_mode", [0, 1], ids=["strict", "fma"])
def test_cpp_render_backward_matches_the_restatement(exe, tmp_path, fp_mode):
    ref = gu.reference("sh16", "default", fp_mode, 4, 48)
    tree, trs, w, h, f = ref["tree"], ref["trs"], ref["w"], ref["h"], ref["f"]
    npz, poses, g_raw, out_raw = (str(tmp_path / n) for n in ("t.npz", "poses.raw", "g.raw", "grad.raw"))
    synth.save_npz(tree, npz, compressed=False)
    np.stack(trs).astype(np.float32).tofile(poses)
    np.ascontiguousarray(ref["g"], np.float32).tofile(g_raw)
    r = subprocess.run([exe, npz, poses, str(len(trs)), str(w), str(h), repr(float(f)), str(fp_mode), g_raw, out_raw],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split() for line in r.stdout.splitlines() if len(line.split()) == 2)   # (the loader prints too)
    assert got["throws"] == "1" and int(got["elements"]) == ref["grad"].size
    grad = np.fromfile(out_raw, np.float32).reshape(ref["grad"].shape)
    ratio, zeros_same = gu.worst_ratio(grad, ref)
    print(f"C++ wrapper fp{fp_mode}: worst |gpu - f64| / unit = {ratio:.3f} of {gu.K}")
    assert (ref["mag"] > 0).sum() > 1000
    assert ratio <= gu.K and zeros_same
