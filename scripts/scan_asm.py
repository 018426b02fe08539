#!/usr/bin/env python3
"""Per-kernel metadata and instruction counts of klf_kernels.hip's device assembly.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S klf_kernels.hip -o new.s
  scripts/scan_asm.py new.s            # one line per kernel
  scripts/scan_asm.py old.s new.s      # kernels whose metadata or instruction text differ

It reads the .amdhsa_* metadata, the "; Occupancy:" / spill comments and the instruction
text (labels normalised), and counts lines; nothing else.
"""
import hashlib
import re
import subprocess
import sys

META = {"vgpr": "next_free_vgpr", "sgpr": "next_free_sgpr", "lds": "group_segment_fixed_size",
        "priv": "private_segment_fixed_size"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"klf::\(anonymous namespace\)::|void |\(klf::RunArgs.*", "", d) for n, d in zip(names, out)}


def kernels(path):
    """{symbol: {vgpr, sgpr, lds, priv, occ, spill, lines, sha}} of every kernel in the file."""
    ks, cur, body, name, lane = {}, None, [], None, 0
    for line in open(path):
        s = line.strip()
        m = re.match(r"(\w+):\s*; @\1", s)
        if m:
            name, body, lane = m.group(1), [], 0
            continue
        if name and s.startswith(".Lfunc_end"):
            text = re.sub(r"\.LBB\d+_\d+", "L", "\n".join(body))
            ks.setdefault(name, {}).update(lines=len(body), lane=lane, sha=hashlib.sha1(text.encode()).hexdigest()[:10])
            cur = name
            name = None
            continue
        if name and s and not s.startswith((";", ".")) and not s.endswith(":"):
            body.append(s.split(";")[0].strip())
        if name and "SGPR spill to VGPR lane" in s:
            lane += 1
        m = re.match(r"\.amdhsa_kernel (\w+)", s)
        if m:
            cur = m.group(1)
        for k, key in META.items():
            m = re.match(r"\.amdhsa_%s (\d+)" % key, s)
            if m and cur:
                ks.setdefault(cur, {})[k] = int(m.group(1))
        m = re.match(r"; (Occupancy|ScratchSize|sgpr_spill_count|vgpr_spill_count): (\d+)", s)
        if m and cur:
            key = "occ" if m.group(1) == "Occupancy" else "spill"
            ks[cur][key] = ks[cur].get(key, 0) + int(m.group(2)) if key == "spill" else int(m.group(2))
    return {k: v for k, v in ks.items() if "lines" in v and "vgpr" in v}


def row(v):
    return "vgpr %3d sgpr %3d lds %6d priv %d occ %d spill %d+%d lines %5d %s" % (
        v["vgpr"], v["sgpr"], v["lds"], v["priv"], v.get("occ", 0), v.get("spill", 0), v["lane"], v["lines"], v["sha"])


def main(argv):
    new = kernels(argv[-1])
    old = kernels(argv[1]) if len(argv) > 2 else None
    names = demangle(sorted(set(new) | set(old or {})))
    same = 0
    for k in sorted(names, key=names.get):
        if old is None:
            print("%-44s %s" % (names[k], row(new[k])))
        elif k not in new or k not in old:
            print("%-44s only in %s" % (names[k], "old" if k in old else "new"))
        elif old[k] != new[k]:
            print("%-44s old %s\n%-44s new %s" % (names[k], row(old[k]), "", row(new[k])))
        else:
            same += 1
    if old is not None:
        print("%d kernels identical (metadata and instruction text)" % same)


if __name__ == "__main__":
    main(sys.argv)
