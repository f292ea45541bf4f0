#!/usr/bin/env python3
"""Kernel resource usage of one source file as a table, and the comparison of two such tables.

  hipcc --offload-arch=gfx950 <the build's flags> -c audio_rag_amd/csrc/dense.hip -o /dev/null \\
      -Rpass-analysis=kernel-resource-usage 2> remarks.txt
  python tools/kernel_resource_summary.py summary remarks.txt > profiles/<name>.txt
  python tools/kernel_resource_summary.py compare parent.txt new.txt [--only dense_scan_i8_kernel]

`summary` prints one line per kernel (demangled by c++filt when it is installed): SGPRs, VGPRs,
AGPRs, scratch bytes per lane, occupancy in waves per SIMD, static LDS bytes and the spill counts.
`compare` exits 1 when a kernel present in both tables differs in any column (with --only: among
the kernels whose name contains that text), and lists the kernels only one table has."""

import re
import shutil
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy"),
          ("LDS Size [bytes/block]", "lds"), ("SGPRs Spill", "sgpr_spill"),
          ("VGPRs Spill", "vgpr_spill")]


def parse(path: str) -> dict:
    kernels, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for label, short in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\S+)", line)
            if m and cur is not None:
                cur[short] = m.group(1)
    return kernels


def demangle(names: list) -> list:
    if not shutil.which("c++filt") or not names:
        return names
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    got = out.stdout.splitlines()
    got = [re.sub(r"\(anonymous namespace\)::", "", g).split("(")[0].removeprefix("void ") for g in got]
    return got if len(got) == len(names) else names


def summary(path: str) -> None:
    kernels = parse(path)
    names = sorted(kernels)
    print("# kernel " + " ".join(short for _, short in FIELDS))
    for name, shown in sorted(zip(names, demangle(names)), key=lambda p: p[1]):
        print(shown.replace(" ", ""), " ".join(kernels[name].get(short, "?") for _, short in FIELDS))


def table(path: str) -> dict:
    rows = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        name, *vals = line.split()
        rows[name] = vals
    return rows


def compare(a: str, b: str, only: str | None) -> int:
    ta, tb = table(a), table(b)
    keep = lambda n: only is None or only in n
    bad = 0
    for name in sorted(n for n in ta if n in tb and keep(n)):
        same = ta[name] == tb[name]
        bad += not same
        print(("same      " if same else "DIFFERENT ") + name + " " + " ".join(ta[name])
              + ("" if same else "  ->  " + " ".join(tb[name])))
    for name in sorted(n for n in tb if n not in ta and keep(n)):
        print("new       " + name + " " + " ".join(tb[name]))
    for name in sorted(n for n in ta if n not in tb and keep(n)):
        print("gone      " + name)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
        sys.exit(compare(sys.argv[2], sys.argv[3], only))
    else:
        sys.exit(__doc__)
