"""How the tests build and run their helper programs: the C restatements (the oracle's flags), the C++ check
programs of tests/cpp (the host archive's link line), the HIP check programs that include the kernels' headers
(the product's flags), the struct-layout probe, and the parse of a check program's `key value` output.  Each
command stands here once."""
from __future__ import annotations

import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@functools.lru_cache(maxsize=None)
def c_library(src, defines=(), oracle=False):
    """tests/cpp/<src> as a shared library, built with the oracle's flags (its FP model: no contraction, FMA
    only where fmaf is written) into a directory removed at exit; once per argument list.
    oracle: the file calls liboracle.so's or_* functions."""
    td = tempfile.mkdtemp(prefix="vr_" + os.path.splitext(src)[0] + "_")
    atexit.register(shutil.rmtree, td, ignore_errors=True)
    so = os.path.join(td, "lib" + os.path.splitext(src)[0] + ".so")
    link = []
    if oracle:
        from oracle import binding as ob
        where = os.path.dirname(ob.build_oracle())
        link = ["-L", where, "-loracle", "-Wl,-rpath," + where]
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-mfma", "-fPIC", "-shared",
                           "-Wno-unused-function", *defines, "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(CPP, src), "-o", so, *link, "-lm"])
    return C.CDLL(so)


def cpp_program(name, out_dir, gpu=False):
    """tests/cpp/<name>.cpp linked against the C++ host layer and libvolrend_hip -> the program's path.
    gpu: the program calls HIP itself; skips the calling test when no device is visible."""
    if gpu:
        import torch
        if not torch.cuda.is_available():
            pytest.skip("no GPU visible")
    subprocess.check_call(["make", "-C", ROOT, "host"], stdout=subprocess.DEVNULL)
    out = os.path.join(str(out_dir), name)
    lib_dir = os.path.join(ROOT, "volrend_amd")
    hip = (["-D__HIP_PLATFORM_AMD__"], ["-I", "/opt/rocm/include"], ["-L/opt/rocm/lib", "-lamdhip64"], ["-pthread"])
    define, include, hip_lib, threads = hip if gpu else ([], [], [], [])
    subprocess.check_call(["g++", "-O1", "-std=c++17", *define, "-I", os.path.join(ROOT, "include"), *include,
                           os.path.join(CPP, name + ".cpp"), os.path.join(lib_dir, "libvolrend_host.a"),
                           "-L", lib_dir, "-lvolrend_hip", *hip_lib, "-lz", *threads,
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def hip_program(name, out_dir, c_sources=()):
    """tests/cpp/<name>.hip, which includes the kernels' headers, compiled with the product's own flags
    (volrend_amd/build.py FLAGS without -shared / -fPIC: -ffp-contract=off and -fno-gpu-flush-denormals-to-zero are
    the contract under test) and linked with liboracle.so and the c_library of every file of c_sources -> the
    program's path.  Skips the calling test when no device is visible."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from oracle import binding as ob
    from volrend_amd import build as vb
    ob.build_oracle()
    flags = [f for f in vb.FLAGS if f not in ("-shared", "-fPIC")]
    assert "-ffp-contract=off" in flags and "-fno-gpu-flush-denormals-to-zero" in flags
    libs = [("oracle", os.path.dirname(ob.ORACLE_SO))]
    libs += [(os.path.splitext(src)[0], os.path.dirname(c_library(src, oracle=True)._name)) for src in c_sources]
    out = os.path.join(str(out_dir), name)
    subprocess.check_call([vb.HIPCC, *flags, "-I", vb.CSRC, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "oracle"), os.path.join(CPP, name + ".hip"),
                           *[a for lib, where in libs for a in ("-L", where, "-l" + lib, "-Wl,-rpath," + where)],
                           "-pthread", "-o", out])
    return out


def csrc_program(name, unit, out_dir):
    """tests/cpp/<name>.cpp with the host unit volrend_amd/csrc/<unit>.cpp, stand-alone (no library, no device)."""
    csrc = os.path.join(ROOT, "volrend_amd", "csrc")
    out = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", csrc, os.path.join(CPP, name + ".cpp"),
                           os.path.join(csrc, unit + ".cpp"), "-o", out])
    return out


def run_key_values(exe, *args, timeout=300, refusals=False):
    """Runs a check program, which must exit with 0 -> its `key value` lines as a dict of strings.
    The default takes the stdout lines of exactly two fields (the loader prints too).  refusals: every stdout
    line but the loader's INFO: lines must be `key value`, the value being the rest of the line."""
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    if refusals:
        return dict(l.split(" ", 1) for l in r.stdout.splitlines() if not l.startswith("INFO:"))
    return dict(line.split() for line in r.stdout.splitlines() if len(line.split()) == 2)


def c_struct_layout(struct_name, ctypes_struct, extra=()):
    """include/volrend_hip.h as the C compiler sees it -> dict of ints: "size" = sizeof(struct_name), every
    field of ctypes_struct -> its offsetof, and every (key, C expression) of `extra` -> the expression's value."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "volrend_hip.h"', 'int main(void){',
             f'printf("size %zu\\n", sizeof({struct_name}));']
    lines += [f'printf("{f} %zu\\n", offsetof({struct_name}, {f}));' for f, _ in ctypes_struct._fields_]
    lines += [f'printf("{key} %lld\\n", (long long)({expr}));' for key, expr in extra]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "layout.c"), os.path.join(td, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        return {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe], text=True).splitlines())}


def word_digest(a) -> str:
    """sum_i (w_i + 1) * ((2 i + 1) * K) mod 2^64 over the 32-bit words: mirrors digest() of
    tests/cpp/query_check.cpp (and of the check programs that print the same digests)."""
    w = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        d = ((w + np.uint64(1)) * ((np.uint64(2) * i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))).sum(dtype=np.uint64)
    return f"{int(d):016x}"
