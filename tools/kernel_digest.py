#!/usr/bin/env python3
"""One line per gfx950 kernel of the product build: mangled name, code size, SHA-256 of its code bytes,
SHA-256 of its kernel descriptor.  Two trees whose lines are equal run the same machine code with the same
register / LDS / scratch allocation, whatever file a kernel sits in.  No GPU needed.

    python tools/kernel_digest.py [file.hip ...]        (default: every .hip of volrend_amd/build.py SOURCES)

The descriptor (<name>.kd, 64 bytes) is hashed with kernel_code_entry_byte_offset (bytes 16-23) zeroed:
that field is the distance between descriptor and code and moves with the layout of the object.
"""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volrend_amd import build as vb  # noqa: E402

BUNDLER = os.path.join(os.path.dirname(os.path.realpath(vb.HIPCC)), "..", "llvm", "bin", "clang-offload-bundler")


def device_elf(src: str, tmp: str) -> bytes:
    obj, elf = os.path.join(tmp, "dev.o"), os.path.join(tmp, "dev.elf")
    subprocess.check_call([vb.HIPCC, *[f for f in vb.FLAGS if f != "-shared"], "--cuda-device-only", "-c",
                           "-I", os.path.join(vb.ROOT, "include"), "-I", os.path.dirname(src), src, "-o", obj])
    subprocess.check_call([BUNDLER, "--unbundle", "--type=o", f"--input={obj}", f"--output={elf}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
    return open(elf, "rb").read()


def kernels(elf: bytes):
    """(name, size, code sha256, masked descriptor sha256) of every FUNC symbol that has a descriptor."""
    shoff, shentsize, shnum = struct.unpack_from("<Q", elf, 0x28)[0], *struct.unpack_from("<HH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    symtab = next(s for s in sec if s[1] == 2)  # SHT_SYMTAB
    strtab = sec[symtab[6]]
    syms = {}
    for off in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, off)
        end = elf.index(b"\0", strtab[4] + name)
        syms[elf[strtab[4] + name:end].decode()] = (info & 15, shndx, value, size)

    def data(shndx, value, size):  # bytes [value, value + size) of a symbol of section shndx
        start = sec[shndx][4] + value - sec[shndx][3]
        return elf[start:start + size]

    for name, (typ, shndx, value, size) in sorted(syms.items()):
        if typ != 2 or name + ".kd" not in syms:  # STT_FUNC with a kernel descriptor
            continue
        _, kshndx, kvalue, ksize = syms[name + ".kd"]
        kd = bytearray(data(kshndx, kvalue, ksize))
        assert len(kd) == 64, (name, len(kd))
        kd[16:24] = bytes(8)
        yield name, size, hashlib.sha256(data(shndx, value, size)).hexdigest(), hashlib.sha256(kd).hexdigest()


if __name__ == "__main__":
    files = sys.argv[1:] or [os.path.join(vb.CSRC, s) for s in vb.SOURCES if s.endswith(".hip")]
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for f in files:
            lines += ["%s %d %s %s" % k for k in kernels(device_elf(os.path.abspath(f), tmp))]
    print("\n".join(sorted(lines)))
