#!/usr/bin/env python3
"""Runs one BASELINE config's device-resident filter a few times (profiling driver).

    python scripts/run_config.py c1|c2|c3|c4|c5 [--steps K] [--warmup W] [--window FRAC] [--hist SECONDS]

bench.run_config without the checks, the CPU baseline, the write and capture paths.
Prints the result dict as one JSON line.

--window FRAC measures klf_window instead (SPEC.md S4b, DESIGN.md "Time window"): per timed
step one run of the config (its patterns and --tail, no --since), then a window over the middle
FRAC of the streams' time span with the same --tail, then a fresh run over the same resident
batch with since = the window's lower bound (the nearest thing the engine could do before
klf_window).  Reports the medians of
klf_result_timing[4] of the three, and the wall time of the klf_window call (it includes the
line index a run without patterns and without --tail left out, built on first use).

--hist SECONDS measures klf_result_histogram (SPEC.md S4c, DESIGN.md "Histogram"): per timed
step one run of the config (no --since), one klf_window over the streams' whole time span as a
yardstick (k_tw_build walks the same lines the same way), then one histogram of that result over
the whole span in buckets of SECONDS.  Reports the medians of the histogram's device time, of the
window's klf_result_timing[4], and of the histogram call's wall time."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def window_probe(name: str, frac: float, steps: int, warmup: int, now: int) -> dict:
    import time

    import numpy as np
    import torch
    from klogs_amd import engine as E
    from klogs_amd import synth

    sizes, kind, pats, permille, mode, desc = bench.config_table(name)
    dev, seg_base, lens = bench.load_batch(sizes, kind, permille, list(range(len(sizes))), 0)
    tail = -1 if mode == "-l" else bench.TAIL
    since = None  # (the window stands in for the config's --since 5m, which would drop all it selects)
    lo = synth.T0 + int(synth.SPAN * (0.5 - frac / 2))
    frm, until = (lo, 0), (lo + int(synth.SPAN * frac), 0)
    eng = E.Engine(0, hip_stream=torch.cuda.current_stream().cuda_stream, **pats)
    ptr = dev.data_ptr()
    run_ms, win_ms, rerun_ms, wall_ms = [], [], [], []
    counts = {}
    for i in range(warmup + steps):
        r = eng.run_device(ptr, seg_base, lens, since=since, tail=tail)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w = r.window(frm, until, tail=tail)  # (returns after its counts came back: synchronous)
        t_wall = (time.perf_counter() - t0) * 1e3
        t_run, t_win = r.timing()[4], w.timing()[4]
        counts = {"window": w.totals()}
        r.free()
        w.free()
        r2 = eng.run_device(ptr, seg_base, lens, since=frm, tail=tail)
        t_rerun = r2.timing()[4]
        counts["rerun"] = r2.totals()
        r2.free()
        if i >= warmup:
            run_ms.append(t_run)
            win_ms.append(t_win)
            rerun_ms.append(t_rerun)
            wall_ms.append(t_wall)
    med = lambda v: round(float(np.median(v)), 4)
    return {"workload": desc, "streams": len(lens), "bytes": int(sum(lens)), "window_frac": frac, "steps": steps,
            "from": frm[0], "until": until[0], "tail": tail,
            "run_device_ms": med(run_ms), "window_ms": med(win_ms), "window_call_wall_ms": med(wall_ms), "rerun_since_from_ms": med(rerun_ms),
            "window_ms_all": [round(x, 4) for x in win_ms], "rerun_ms_all": [round(x, 4) for x in rerun_ms],
            "counts": counts}


def hist_probe(name: str, seconds: float, steps: int, warmup: int) -> dict:
    import time

    import numpy as np
    import torch
    from klogs_amd import engine as E
    from klogs_amd import synth

    sizes, kind, pats, permille, mode, desc = bench.config_table(name)
    dev, seg_base, lens = bench.load_batch(sizes, kind, permille, list(range(len(sizes))), 0)
    tail = -1 if mode == "-l" else bench.TAIL
    frm, until = (synth.T0, 0), (synth.T0 + synth.SPAN + 1, 0)
    width_ns = int(round(seconds * 1e9))  # (a whole number of seconds takes the 32-bit division)
    nb = ((until[0] - frm[0]) * 10**9 + width_ns - 1) // width_ns
    eng = E.Engine(0, hip_stream=torch.cuda.current_stream().cuda_stream, **pats)
    ptr = dev.data_ptr()
    hist_ms, win_ms, wall_ms = [], [], []
    counted = below_above = None
    for i in range(warmup + steps):
        r = eng.run_device(ptr, seg_base, lens, since=None, tail=tail)
        w = r.window(frm, until, tail=tail)
        r.free()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts, outside = w.histogram(frm, width_ns, nb)  # (synchronous: the table came back)
        t_wall = (time.perf_counter() - t0) * 1e3
        counted, below_above = int(counts.sum()), [int(x) for x in outside.sum(axis=0)]
        assert counted + sum(below_above) == w.totals()["matched"]
        if i >= warmup:
            hist_ms.append(w.hist_ms)
            win_ms.append(w.timing()[4])
            wall_ms.append(t_wall)
        w.free()
    med = lambda v: round(float(np.median(v)), 4)
    return {"workload": desc, "streams": len(lens), "bytes": int(sum(lens)), "bucket_s": seconds, "buckets": nb,
            "steps": steps, "tail": tail, "hist_ms": med(hist_ms), "window_ms": med(win_ms),
            "hist_call_wall_ms": med(wall_ms), "hist_ms_all": [round(x, 4) for x in hist_ms],
            "window_ms_all": [round(x, 4) for x in win_ms], "lines_in_buckets": counted, "below_above": below_above}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--probe", action="store_true", help="add bench.box_probe (the box's copy / read rates)")
    ap.add_argument("--window", type=float, default=None, metavar="FRAC",
                    help="time klf_window over the middle FRAC of the time span against a rerun with since = from")
    ap.add_argument("--hist", type=float, default=None, metavar="SECONDS",
                    help="time klf_result_histogram in buckets of SECONDS beside a klf_window over the whole span")
    a = ap.parse_args()
    ns = argparse.Namespace(steps=a.steps, warmup=a.warmup, no_verify=True, no_write=True, no_capture=True,
                            no_cpu_baseline=True, capture_piece=4 << 20, full=True, dump_outputs=None)
    now = bench.synth.T0 + bench.synth.SPAN + 1
    probe = bench.box_probe(0) if a.probe else None
    if a.window is not None:
        out = window_probe(a.config, a.window, a.steps, a.warmup, now)
    elif a.hist is not None:
        out = hist_probe(a.config, a.hist, a.steps, a.warmup)
    else:
        out = bench.run_config(a.config, ns, 0, now)
    if probe:
        out["box_probe"] = probe
    print(json.dumps(out))


if __name__ == "__main__":
    main()
