#!/usr/bin/env python3
"""Fingerprint of every gfx950 kernel in a shared library (CPU only).

    python scripts/kernel_fingerprint.py speculative-decoding_amd/specdec_amd/libspecdec.so > new.txt

One line per kernel, sorted by name: symbol, code size, SHA-256 of the kernel's bytes in .text, then
the code-object notes' register, LDS, scratch, kernarg and spill figures.  Two builds whose outputs
are equal run the same machine code, however the kernels were spread over translation units; diff
the outputs of the library before and after a change that must not touch device code.

Extraction follows tests/test_lib_cpu.py::kernel_notes: objcopy the .hip_fatbin section, split it at
the bundle magic (one bundle per HIP translation unit), unbundle the gfx950 code object with
clang-offload-bundler, read it with llvm-readelf.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size", ".kernarg_segment_size", ".sgpr_spill_count", ".vgpr_spill_count")


def code_objects(lib_path, llvm, arch, tmp):
    fb = os.path.join(tmp, "fb.bin")
    subprocess.check_call(["objcopy", "--dump-section", f".hip_fatbin={fb}", lib_path, os.path.join(tmp, "x.so")])
    data = open(fb, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    for i, st in enumerate(starts):
        part, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"co{i}.o")
        with open(part, "wb") as f:
            f.write(data[st:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", f"--input={part}",
                               f"--output={co}", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}"])
        yield co


def kernel_notes(co, llvm):
    """{kernel symbol: {field: value}} from the code object's metadata note."""
    notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co]).decode()
    # amdhsa.kernels is a YAML list at the top level: one item per kernel, opened by "  - " at an
    # indent of two; a kernel's arguments are list items too, but nested deeper (.args)
    m = re.search(r"^amdhsa\.kernels:\n((?:[ ].*\n)*)", notes, re.M)
    if not m:
        raise SystemExit(f"{co}: no amdhsa.kernels in the metadata note")
    out = {}
    for item in re.split(r"^  - ", m.group(1), flags=re.M)[1:]:
        top = {}   # the item's own keys: the first line, and the lines indented by exactly four
        for line in item.splitlines():
            kv = re.match(r"(?:    )?(\.\w+):\s*(.*?)\s*$", line)
            if kv:
                top.setdefault(kv.group(1), kv.group(2))
        missing = [f for f in (".symbol",) + FIELDS if f not in top]
        if missing:
            raise SystemExit(f"{co}: kernel {top.get('.symbol', top.get('.name', '?'))} lacks {missing}")
        out[top[".symbol"].strip("'")[:-len(".kd")]] = {f: top[f] for f in FIELDS}
    return out


def text_symbols(co, llvm):
    """(.text bytes, its address, {function symbol: (address, size)})"""
    secs = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "-S", "--wide", co]).decode()
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", secs)
    addr, off, size = (int(x, 16) for x in m.groups())
    with open(co, "rb") as f:
        f.seek(off)
        text = f.read(size)
    syms = {}
    table = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--symbols", "--wide", co]).decode()
    for line in table.splitlines():
        p = line.split()
        if len(p) == 8 and p[3] == "FUNC" and p[6] != "UND":
            syms[p[7]] = (int(p[1], 16), int(p[2], 0))
    return text, addr, syms


def fingerprint(lib_path, llvm, arch):
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib_path, llvm, arch, tmp):
            notes = kernel_notes(co, llvm)
            text, addr, syms = text_symbols(co, llvm)
            for name, vals in notes.items():
                if name not in syms:
                    raise SystemExit(f"{co}: kernel {name} has no function symbol")
                a, n = syms[name]
                code = text[a - addr:a - addr + n]
                assert len(code) == n, name
                lines.append(" ".join([name, f"size={n}", "sha256=" + hashlib.sha256(code).hexdigest()] +
                                      [f"{f[1:]}={vals[f]}" for f in FIELDS]))
    return sorted(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("library")
    ap.add_argument("--llvm", default="/opt/rocm/lib/llvm/bin", help="directory of clang-offload-bundler and llvm-readelf")
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    lines = fingerprint(a.library, a.llvm, a.arch)
    print("\n".join(lines))
    print(f"{len(lines)} kernels", file=sys.stderr)


if __name__ == "__main__":
    main()
