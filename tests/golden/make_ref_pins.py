#!/usr/bin/env python3
"""Generates tests/golden/ref_pins_v1.json and ref_frames_v1.npz -- what the reference's own code
outputs for the cases of the tests that compare against it (tests/common.py assert_ref_equal /
ref_array): its device code compiled for the host (oracle/_ref, made by build() where the reference
is mounted) and its GLSL backend on a software rasteriser.  Outputs that must be equal bit for bit
are stored as SHA-256 digests; the two frames that tests compute with are stored as they are.

Run where both are available:   python tests/golden/make_ref_pins.py

The script runs those tests with VOLREND_RECORD_REF_PINS set, so every output a test asks of the
reference is recorded, then packs the records.  A test that fails while recording (the oracle no
longer equals the reference) leaves the files unwritten.
"""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
TESTS = ["tests/test_oracle_vs_ref.py", "tests/test_rtfrag_crosscheck.py"]


def main():
    from oracle import binding as ob
    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_build"))
    import rtfrag_baseline
    if ob.ref_lib() is None or rtfrag_baseline.find_swiftshader() is None:
        raise SystemExit("needs the reference's host build (oracle/_ref) and a software GL")
    with tempfile.TemporaryDirectory() as rec:
        env = dict(os.environ, VOLREND_RECORD_REF_PINS=rec)
        subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", *TESTS],
                              cwd=ROOT, env=env)
        key = lambda f, ext: os.path.basename(f)[:-len(ext)].replace("__", "/")  # noqa: E731
        digests = {key(f, ".sha256"): open(f).read() for f in sorted(glob.glob(os.path.join(rec, "*.sha256")))}
        frames = {key(f, ".npy"): np.load(f) for f in sorted(glob.glob(os.path.join(rec, "*.npy")))}
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "ref_pins_v1.json"), "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(here, "ref_frames_v1.npz"), **frames)
    for name in ("ref_pins_v1.json", "ref_frames_v1.npz"):
        print("wrote", name, os.path.getsize(os.path.join(here, name)) // 1024, "KiB")


if __name__ == "__main__":
    main()
