#!/usr/bin/env python3
"""Kernel resource usage from hipcc's -Rpass-analysis=kernel-resource-usage
remarks, one row per kernel; with two logs, side by side with the rows that
differ marked.  No GPU needed:

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> \\
          -Rpass-analysis=kernel-resource-usage -c conv3x3.hip -o /dev/null 2> new.txt
    python tools/resource_table.py parent.txt new.txt [--filter conv12p,convnet_convs]
"""
import argparse
import re
import subprocess

FIELDS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "LDS"))


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return [re.sub(r"\(.*", "", s).replace("void ", "") for s in out.stdout.splitlines()]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def parse(path):
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            cur = rows.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    names = list(rows)
    return dict(zip(demangle(names), (rows[n] for n in names)))


def fmt(r):
    return "  ".join(f"{short} {r.get(key, '-'):>4}" for key, short in FIELDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logs", nargs="+")
    ap.add_argument("--filter", default="", help="comma-separated substrings of kernel names to keep")
    a = ap.parse_args()
    keep = [f for f in a.filter.split(",") if f]
    tabs = [parse(p) for p in a.logs[:2]]
    names = sorted(set().union(*tabs))
    ndiff = 0
    for n in names:
        if keep and not any(k in n for k in keep):
            continue
        rs = [t.get(n) for t in tabs]
        print(n)
        for p, r in zip(a.logs, rs):
            print(f"    {fmt(r) if r else '(absent)':<80} {p}")
        if len(rs) == 2 and rs[0] is not None and rs[1] is not None and rs[0] != rs[1]:
            ndiff += 1
            print("    ^^^ DIFFERS")
    if len(tabs) == 2:
        print(f"{ndiff} kernel(s) present in both logs differ")


if __name__ == "__main__":
    main()
