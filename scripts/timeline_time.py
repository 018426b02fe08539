#!/usr/bin/env python3
"""Times klf_result_timeline (SPEC.md S4d, DESIGN.md "Merged timeline") on a BASELINE config.

    python scripts/timeline_time.py c3|c5 [--steps K] [--warmup W]

Per timed step: one device-resident run of the config (no --since; --tail as the config has it),
one histogram of the result over the streams' whole time span as a yardstick (k_hist walks a
bitmap the same way), then one timeline with tags and without timestamps.  Reports the medians
of the timeline's device time (klf_timeline_ms), of the histogram's, and of the timeline call's
wall time, the entries and merged bytes, and how many of the twelve radix passes ran (the key
bytes that differ somewhere, from the entries).  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def passes_run(entries) -> int:
    """Key bytes (nsec 0..3, sec 0..7) that are not the same in every entry."""
    import numpy as np

    if len(entries) == 0:
        return 0
    n = 0
    for col, width in ((entries["nsec"].astype(np.uint32), 4), (entries["sec"].astype(np.int64).view(np.uint64), 8)):
        lo, hi = np.bitwise_and.reduce(col), np.bitwise_or.reduce(col)
        n += sum(1 for k in range(width) if (int(lo) >> (8 * k)) & 255 != (int(hi) >> (8 * k)) & 255)
    return n


def probe(name: str, steps: int, warmup: int) -> dict:
    import numpy as np
    import torch
    from klogs_amd import engine as E
    from klogs_amd import synth

    sizes, kind, pats, permille, mode, desc = bench.config_table(name)
    dev, seg_base, lens = bench.load_batch(sizes, kind, permille, list(range(len(sizes))), 0)
    tail = -1 if mode == "-l" else bench.TAIL
    tags = [b"pod-%d/container " % i for i in range(len(lens))]
    nb = (synth.SPAN + 60) // 60
    eng = E.Engine(0, hip_stream=torch.cuda.current_stream().cuda_stream, **pats)
    ptr = dev.data_ptr()
    tl_ms, hist_ms, wall_ms = [], [], []
    n = size = passes = 0
    for i in range(warmup + steps):
        r = eng.run_device(ptr, seg_base, lens, since=None, tail=tail)
        r.histogram((synth.T0, 0), 60 * 10**9, nb)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tl = r.timeline(tags=tags)  # (synchronous: the merged length came back)
        t_wall = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            tl_ms.append(tl.ms)
            hist_ms.append(r.hist_ms)
            wall_ms.append(t_wall)
        if i == warmup + steps - 1:
            n, size = len(tl), tl.size
            passes = passes_run(tl.entries)
            assert n == r.totals()["selected"]
        tl.free()
        r.free()
    eng.close()
    med = lambda v: round(float(np.median(v)), 4)
    return {"workload": desc, "streams": len(lens), "bytes": int(sum(lens)), "tail": tail, "steps": steps,
            "entries": n, "merged_bytes": size, "radix_passes": passes, "timeline_ms": med(tl_ms),
            "hist_ms": med(hist_ms), "timeline_call_wall_ms": med(wall_ms),
            "timeline_ms_all": [round(x, 4) for x in tl_ms], "hist_ms_all": [round(x, 4) for x in hist_ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    print(json.dumps(probe(a.config, a.steps, a.warmup)))


if __name__ == "__main__":
    main()
