#!/usr/bin/env python
"""Digest of the gfx950 device code of csrc/taco_lib.hip: the proof that a refactor of the kernel headers changed no instruction.

Builds the device side only, with the production flags of csrc/build.sh plus whatever is given after `--`, unbundles the gfx950
ELF and prints its sha256, then one sha256 per kernel (every FUNC symbol of .text that has a `.kd` descriptor), in the order the
kernels have in the code object.  Two trees whose first lines agree run the same device code; where they differ, the per-kernel
lines say which kernel moved.  A kernel's bytes hold pc-relative offsets to what it calls or reads, so a change of size in one kernel
can show in another that refers across it: read the first differing line first.  The script hashes bytes and reads no instruction.

    python tools/device_code_digest.py [--src DIR] [--keep FILE] [-- -DDX_DLY_RT ...]

DIR is a csrc directory (of this checkout by default; of another checkout -- `git worktree add`, `git archive` -- to compare against).
The compiler runs inside DIR on the relative name taco_lib.hip with a fixed compilation-unit id (CUID below), so that no path reaches
the object; everything it writes goes to a temporary directory.  Without the fixed id two builds of the same source into two output
paths differ in the name of one symbol (and in the symbol hash tables with it), in no byte of .text.
The record of the refactor that introduced this script is profiles/r22_code_identity.txt."""
import argparse
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-speaker-tacotron-tensorflow_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c"]
# hipcc names one symbol of the code object (__hip_cuid_...) after a hash of its command line, the output path included: fixed here, so that the
# temporary directory an object is written to does not show in its bytes
CUID = "-cuid=taco_lib"
TARGET = "hip-amdgcn-amd-amdhsa--gfx950"
STT_FUNC = 2


def tool(name):
    for d in (os.path.join(ROCM, "bin"), os.path.join(ROCM, "lib", "llvm", "bin"), os.path.join(ROCM, "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return name


def build_elf(src, extra, tmp):
    """the unbundled gfx950 ELF of src/taco_lib.hip, as bytes"""
    obj = os.path.join(tmp, "taco_lib.o")
    elf = os.path.join(tmp, "taco_lib.gfx950.elf")
    hipcc = os.environ.get("HIPCC", tool("hipcc"))
    subprocess.run([hipcc] + FLAGS + [CUID] + list(extra) + ["-o", obj, "taco_lib.hip"], cwd=src, check=True)
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                    "--input=" + obj, "--output=" + elf], check=True)
    with open(elf, "rb") as f:
        return f.read()


def kernels(elf):
    """[(name, bytes)] of every kernel in .text, by address"""
    if elf[:6] != b"\x7fELF\x02\x01":
        sys.exit("not a little-endian ELF64")
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]    # name type flags addr off size link info align entsize

    def cstr(tab, at):
        base = sec[tab][4] + at
        return elf[base:elf.index(b"\0", base)].decode()

    text = next(i for i, s in enumerate(sec) if cstr(shstrndx, s[0]) == ".text")
    symtab = next(s for s in sec if cstr(shstrndx, s[0]) == ".symtab")
    syms = []
    for at in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, at)
        syms.append((cstr(symtab[6], name), info & 15, shndx, value, size))
    descriptors = {n[:-3] for n, _t, _s, _v, _z in syms if n.endswith(".kd")}
    out = []
    for n, t, shndx, value, size in sorted(syms, key=lambda s: s[3]):
        if t == STT_FUNC and shndx == text and n in descriptors:
            at = sec[text][4] + value - sec[text][3]
            out.append((n, elf[at:at + size]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--src", default=CSRC, help="csrc directory to build (default: this checkout's)")
    ap.add_argument("--keep", help="also write the unbundled ELF to this file")
    ap.add_argument("flags", nargs="*", help="extra compiler flags, after --")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        elf = build_elf(os.path.abspath(a.src), a.flags, tmp)
    if a.keep:
        with open(a.keep, "wb") as f:
            f.write(elf)
    print("%s  ELF gfx950 %s (%d bytes)" % (hashlib.sha256(elf).hexdigest(), " ".join(a.flags) or "(production flags)", len(elf)))
    for n, code in kernels(elf):
        print("%s  %6d  %s" % (hashlib.sha256(code).hexdigest()[:16], len(code), n))


if __name__ == "__main__":
    main()
