#!/usr/bin/env python3
"""Compare the gfx950 device code of two csrc trees, kernel by kernel.

    python tools/kernel_code_diff.py BASE_CSRC NEW_CSRC [file.hip ...]

Each .hip file is compiled device-only with the Makefile's FLAGS in both trees, the gfx950 code object is unbundled and
disassembled, and per function symbol the sequence of instruction encoding words is compared.  Kernels move inside the
object when the order of template instantiation changes, so the comparison is per symbol, not per file.  Prints, per
file, the number of functions on each side, the names only one side has and the names whose bodies differ; exit status 1
on any difference.  A host-only refactor must print `differing 0` everywhere.
"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")
INSN = re.compile(r"//\s*[0-9A-Fa-f]+:\s*((?:[0-9A-Fa-f]{8}\s*)+)$")


def flags(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read()
    line = re.search(r"^FLAGS\s*=\s*(.*)$", mk, re.M).group(1)
    return line.replace("$(ARCH)", "gfx950").split()


def functions(csrc, name, tmp):
    """{symbol: tuple of encoding words} of one .hip file's gfx950 code object."""
    stem = os.path.join(tmp, name)
    run = lambda *a: subprocess.run(a, check=True, cwd=csrc, stdout=subprocess.PIPE, text=True).stdout
    run(os.path.join(ROCM, "bin", "hipcc"), *flags(csrc), "--cuda-device-only", "-c", name, "-o", stem + ".bundle")
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
        "--input=" + stem + ".bundle", "--output=" + stem + ".co")
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", stem + ".co").splitlines():
        m = SYM.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = INSN.search(line)
        if m and cur is not None:
            cur.extend(m.group(1).split())
    return {k: tuple(v) for k, v in out.items()}


def main():
    base, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    files = sys.argv[3:] or sorted(f for f in os.listdir(new) if f.endswith(".hip"))
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, ThreadPoolExecutor(8) as pool:
        jobs = [(f, pool.submit(functions, base, f, ta), pool.submit(functions, new, f, tb)) for f in files]
        for f, ja, jb in jobs:
            a, b = ja.result(), jb.result()
            lost, extra = sorted(set(a) - set(b)), sorted(set(b) - set(a))
            diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
            print(f"{f}: functions {len(a)} -> {len(b)}, only in base {len(lost)}, only in new {len(extra)}, differing {len(diff)}")
            for tag, names in (("only in base", lost), ("only in new", extra), ("differs", diff)):
                for k in names:
                    print(f"    {tag}: {k}")
            bad += len(lost) + len(extra) + len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
