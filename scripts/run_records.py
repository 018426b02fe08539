#!/usr/bin/env python3
"""Times klf_records (SPEC.md S4h, DESIGN.md "Multi-line records") on one BASELINE config's
device-resident batch.

    python scripts/run_records.py c3 [--steps K] [--warmup W]

The batch is loaded once.  Engines run over it, each `warmup + steps` times, and the best (lowest)
time of the timed steps is reported beside all of them:

  "indent"   --grep NEEDLE at the config's needle rate (the TEXT streams of C1 / C3 carry no
             needle, there the literal "user=r" stands for it), klf_records with INDENT alone: no
             line of the synthetic streams is indented, every line is a head, G' = M; one 16-byte
             load per parsed line
  "cont8"    eight two-byte continuation prefixes that about half of the lines start with: the
             most compares a line can cost, still one load per line
  "long"     one continuation prefix of 21 bytes: the classifier's second 16-byte load on every
             line longer than 16 bytes
  "regroup"  the same engine, klf_regroup with 2 lines of context each way (the yardstick among
             the bitmap transforms: the same three-kernel carry without a walk over the lines)
  "window"   no patterns, klf_window with closed bounds around the whole span: k_tw_build walking
             every parsed line, 32 bytes per line (the yardstick among the walks)

Per case: the device time of building the selection (klf_result_records_info; for the yardsticks
the whole klf_result_timing[4], which is their build plus the tail stage), klf_result_timing[4],
heads, continuations and the selected lines.  Prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

TEXT_NEEDLE = b"user=r"  # in 0.9 % of synth.TEXT's lines
CONT8 = [b"re", b"se", b"qu", b"ha", b"ba", b"st", b"mi", b"sy"]
LONG = [b"retry retry took took"]


def main():
    import torch
    from klogs_amd import engine as E
    from klogs_amd import synth

    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    sizes, kind, pats, permille, mode, desc = bench.config_table(a.config)
    dev, seg_base, lens = bench.load_batch(sizes, kind, permille, list(range(len(sizes))), 0)
    ptr = dev.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    needle = TEXT_NEEDLE if kind == synth.TEXT else synth.NEEDLE
    span = ((synth.T0 - 1, 0), (synth.T0 + synth.SPAN + 1, 0))
    out = {"workload": desc, "streams": len(lens), "bytes": int(sum(lens)), "steps": a.steps, "needle": needle.decode(),
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
            info, counts = w.records_info(), w.totals()
            w.free()
        eng.close()
        out["case_" + name] = {"build_ms_best": round(min(build), 4), "timing4_ms_best": round(min(total), 4),
                               "build_ms_all": [round(x, 4) for x in build], "heads": info[0], "conts": info[1],
                               "lines": counts["lines"], "parsed": counts["parsed"], "selected_from": counts["matched"]}

    case("indent", [needle], lambda r: r.records(indent=True, tail=0), lambda w: w.records_info()[2])
    case("cont8", [needle], lambda r: r.records(cont=CONT8, tail=0), lambda w: w.records_info()[2])
    case("long", [needle], lambda r: r.records(cont=LONG, tail=0), lambda w: w.records_info()[2])
    case("regroup", [needle], lambda r: r.regroup(2, 2, tail=0), lambda w: w.timing()[4])
    case("window", [], lambda r: r.window(span[0], span[1], tail=0), lambda w: w.timing()[4])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
