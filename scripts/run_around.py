#!/usr/bin/env python3
"""Times klf_around (SPEC.md S4g, DESIGN.md "Time context across streams") on one BASELINE
config's device-resident batch.

    python scripts/run_around.py c3 [--steps K] [--warmup W] [--around SECONDS]

The batch is loaded once.  Three engines run over it, each `warmup + steps` times, and the best
(lowest) time of the timed steps is reported beside all of them:

  "needle"   --grep NEEDLE at the config's needle rate (1 % of the lines; the TEXT streams of C1 /
             C3 carry no needle, there the literal "user=r" stands for it: 0.9 % of the lines):
             klf_around with before = after = SECONDS
  "single"   --grep of a marker written over one line's content in the middle of stream 0 (the
             only change to the batch): one anchor
  "tight"    the "needle" engine again with before = after = 0: every distinct anchor instant is
             an interval of its own (K ~ n), so k_ar_build searches a table as long as an
             unmerged one would be; the same anchors, keys and sort
  "window"   no patterns, klf_window with closed bounds around the whole span: k_tw_build walking
             every parsed line, the same 32 bytes per line without a search (the yardstick)

Per case: the device time of building the selection (klf_result_around_info; for the window the
whole klf_result_timing[4], which is k_tw_build plus the tail stage), klf_result_timing[4], the
anchors n, the intervals K and the selected lines.  Prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

MARKER = b"XQ_AROUND_ANCHOR_QX"
TEXT_NEEDLE = b"user=r"  # in 0.9 % of synth.TEXT's lines


def plant_marker(dev, seg_base, lens, sizes, kind, permille) -> int:
    """Writes MARKER over the content of one line in the middle of stream 0; returns its offset."""
    import numpy as np
    import torch
    from klogs_amd import synth

    h = np.empty(lens[0] + 1, dtype=np.uint8)
    synth.generate_into(h, kind, 42, 0, sizes[0], permille=permille)
    body = h[:lens[0]].tobytes()
    pos = body.index(b"\n", lens[0] // 2) + 1  # a line start
    while True:
        end = body.index(b"\n", pos)
        space = body.index(b" ", pos)
        if end - space > len(MARKER) + 2:
            break
        pos = end + 1
    at = space + 1
    assert body[:lens[0]].count(MARKER) == 0
    dev[seg_base[0] + at: seg_base[0] + at + len(MARKER)] = torch.frombuffer(bytearray(MARKER), dtype=torch.uint8).to(dev.device)
    torch.cuda.synchronize()
    return at


def main():
    import torch
    from klogs_amd import engine as E
    from klogs_amd import synth

    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--around", type=float, default=1.0, metavar="SECONDS")
    a = ap.parse_args()
    sizes, kind, pats, permille, mode, desc = bench.config_table(a.config)
    dev, seg_base, lens = bench.load_batch(sizes, kind, permille, list(range(len(sizes))), 0)
    plant_marker(dev, seg_base, lens, sizes, kind, permille)
    ptr = dev.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    d = int(round(a.around * 1e9))
    needle = TEXT_NEEDLE if kind == synth.TEXT else synth.NEEDLE
    span = ((synth.T0 - 1, 0), (synth.T0 + synth.SPAN + 1, 0))
    out = {"workload": desc, "streams": len(lens), "bytes": int(sum(lens)), "around_s": a.around, "steps": a.steps, "needle": needle.decode(),
           "device": torch.cuda.get_device_name(0)}

    def case(name, grep, go, build_of):
        eng = E.Engine(0, hip_stream=stream, grep=grep)
        build, total, info, counts = [], [], None, None
        for i in range(a.warmup + a.steps):
            r = eng.run_device(ptr, seg_base, lens, since=None, tail=0)  # (leaves M and the line meta; no output)
            w = go(r)
            r.free()
            if i >= a.warmup:
                build.append(build_of(w))
                total.append(w.timing()[4])
            info, counts = w.around_counts(), w.totals()
            w.free()
        eng.close()
        out["case_" + name] = {"build_ms_best": round(min(build), 4), "timing4_ms_best": round(min(total), 4),
                     "build_ms_all": [round(x, 4) for x in build], "anchors": info[0], "intervals": info[1],
                     "lines": counts["lines"], "parsed": counts["parsed"], "selected_from": counts["matched"]}

    case("needle", [needle], lambda r: r.around(d, d, tail=0), lambda w: w.around_build_ms())
    case("tight", [needle], lambda r: r.around(0, 0, tail=0), lambda w: w.around_build_ms())
    case("single", [MARKER], lambda r: r.around(d, d, tail=0), lambda w: w.around_build_ms())
    case("window", [], lambda r: r.window(span[0], span[1], tail=0), lambda w: w.timing()[4])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
