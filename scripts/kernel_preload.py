"""Per kernel of a gfx950 assembly file (hipcc -S --cuda-device-only): .sgpr_count, .vgpr_count and
.amdhsa_user_sgpr_kernarg_preload_length (SGPRs the hardware fills with leading kernel arguments
before the wave starts; 0 for a kernel whose first parameter is a struct passed by value).
Sorted by name, one line each: python scripts/kernel_preload.py file.s [filter]  (`make resources`)"""
import re
import shutil
import subprocess
import sys

text = open(sys.argv[1]).read()
flt = sys.argv[2] if len(sys.argv) > 2 else ""
preload = {m.group(1): int(m.group(2)) for m in re.finditer(
    r"\.amdhsa_kernel\s+(\S+)(?:(?!\.end_amdhsa_kernel).)*?\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", text, re.S)}
rows = []
for blk in re.split(r"\n\s*- \.agpr_count", text)[1:]:
    name = re.search(r"\.name:\s*(\S+)", blk).group(1)
    g = lambda k: int(re.search(rf"\.{k}:\s*(\d+)", blk).group(1))
    rows.append((name, g("sgpr_count"), g("vgpr_count"), preload.get(name, 0)))
filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
try:
    pretty = subprocess.run([filt], input="\n".join(r[0] for r in rows), capture_output=True, text=True, check=True).stdout.split("\n")
except (OSError, subprocess.CalledProcessError):
    pretty = [r[0] for r in rows]
for (name, s, v, p), pn in sorted(zip(rows, pretty), key=lambda t: t[1]):
    if flt in pn:
        print(f"{s:>4} sgpr {v:>4} vgpr {p:>3} preload  {pn}")
