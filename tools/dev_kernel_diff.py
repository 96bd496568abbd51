#!/usr/bin/env python3
"""dev: compare the gfx950 kernels of two builds of libqverse.so instruction by instruction (no GPU needed).

    python tools/dev_kernel_diff.py OLD/libqverse.so NEW/libqverse.so [--match REGEX] [--metadata]

Both libraries are unbundled (llvm-objdump --offloading) and disassembled; every kernel symbol present in OLD is looked up
in NEW by name and its instruction stream (addresses stripped) compared.  Prints one line per kernel that differs or is
missing and a summary; exit status 1 if any compared kernel differs.  --metadata also compares the register / LDS / scratch
figures of the AMDGPU notes.  Used to show that a change which adds kernels (e.g. a second instantiation set) left the
existing ones as they were -- stronger than a timing."""
import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def kernels_of(lib: Path, tmp: Path):
    tmp.mkdir(parents=True, exist_ok=True)
    shutil.copy(lib, tmp / "lib.so")
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
    code, meta = {}, {}
    for o in sorted(tmp.glob("lib.so.*gfx950")):
        dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", str(o)], capture_output=True, text=True, check=True).stdout
        name = None
        for ln in dis.splitlines():
            m = re.match(r"[0-9a-f]+ <(\S+)>:", ln)
            if m:
                name = m.group(1)
                code.setdefault(name, [])
            elif name and ln.strip() and ln.strip() != "...":   # "...": zero padding up to the next symbol, not code
                code[name].append(re.sub(r"^\s*[0-9a-f]+:\s*", "", re.sub(r"\s*//.*$", "", ln)).strip())
        for ins in code.values():                       # s_nop after the last s_endpgm: padding up to the next symbol / the section's end
            while ins and ins[-1] == "s_nop 0":
                ins.pop()
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(o)], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            kn = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kn] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                        for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                  "group_segment_fixed_size")}
    return code, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default=".")
    ap.add_argument("--metadata", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        oc, om = kernels_of(Path(a.old), Path(td) / "a")
        nc, nm = kernels_of(Path(a.new), Path(td) / "b")
    rx = re.compile(a.match)
    same = diff = missing = 0
    for k in sorted(om):                     # kernels (the symbols the notes describe), not helper symbols
        if not rx.search(k):
            continue
        if k not in nc:
            print("MISSING in new:", k)
            missing += 1
        elif oc.get(k) != nc[k] or (a.metadata and om[k] != nm.get(k)):
            print(f"DIFFERS: {k} ({len(oc.get(k, []))} vs {len(nc[k])} instructions; {om[k]} vs {nm.get(k)})")
            diff += 1
        else:
            same += 1
    added = sorted(k for k in nm if k not in om and rx.search(k))
    print(f"{same} kernels identical, {diff} differ, {missing} missing, {len(added)} only in new")
    if a.metadata:
        for k in added:
            print("  new:", k, nm[k])
    return 1 if diff or missing else 0


if __name__ == "__main__":
    sys.exit(main())
