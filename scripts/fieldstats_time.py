#!/usr/bin/env python3
"""Times klf_result_field_stats (SPEC.md S4f, DESIGN.md "Numeric field statistics").

    python scripts/fieldstats_time.py c5|text|all

The batches are those of scripts/groups_time.py.  c5: the bench's C5 batch and run (64 regexes,
--since 5m --tail 100: a sparse H of long lines).  text: 16 and 64 TEXT streams of 64 MiB on an
engine without patterns (every line in H).  Per case: the run, then the call's own `ms` output over
repeated calls with p50 / p90 / p99: with the key "latency" (in the synthetic text a word followed
by ' ' or '=' and sometimes a digit: hits, bad lines and misses), as durations with the key
"took", and with a key that occurs nowhere (every content searched to its end).  On the same
result, as yardsticks: klf_result_groups (top = 100, digits masked) and klf_result_histogram.  The
bytes the call reads are reported as h_content_bytes (the contents of H without their '\\n') and
side_bytes (index entries, meta, bitmap); eff_GBps is their sum over the best time.  Prints one
JSON line per measurement."""
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from klogs_amd import engine as E  # noqa: E402
from klogs_amd import synth  # noqa: E402

QUANTILES = (5000, 9000, 9900)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def stats_ms(r, reps, key, **kw):
    ms, rows = [], None
    for _ in range(reps):
        rows, _ = r.field_stats(key, quantiles=QUANTILES, **kw)
        ms.append(round(r.field_ms, 4))
    return ms, rows[-1]


def case(name, sizes, kind, pats, permille, since, tail, reps, max_groups):
    t = time.time()
    dev, seg_base, lens = bench.load_batch(sizes, kind, permille, list(range(len(sizes))), 0)
    emit(case=name, loaded_bytes=sum(lens), load_s=round(time.time() - t, 1))
    eng = E.Engine(0, hip_stream=torch.cuda.current_stream().cuda_stream, **pats)
    r = eng.run_device(dev.data_ptr(), seg_base, lens, since=since, tail=tail)
    tot = r.totals()
    emit(case=name, totals=tot, run_ms=r.timing()[4])
    # the content bytes of H: exact from the unmasked groups when they all fit into `top`
    hbytes = None
    try:
        with r.groups(65536, False, 0, max_groups) as g:
            ent = g.entries
            if g.n_groups <= 65536:
                hbytes = int((ent["count"] * ent["key_len"]).sum())
    except E.KlfError as ex:
        emit(case=name, unmasked_error=str(ex)[:200])
    if hbytes is None and not pats:  # every line out: out_bytes = the contents with their '\n'
        hbytes = tot["out_bytes"] - tot["lines"]
    nh = tot["matched"] if pats else tot["parsed"]
    side = 16 * nh + 2 * nh + ((tot["lines"] + 7) // 8 if pats else 2 * tot["lines"])  # index entries, meta, bitmap / meta
    for key, kw in ((b"latency", {}), (b"latency", dict(decimals=3)), (b"took", dict(duration=True)),
                    (b"no-such-key=", {})):
        ms, all_row = stats_ms(r, reps, key, **kw)
        best = min(ms)
        emit(case=name, key=key.decode(), opts=kw, ms=ms, lines=int(all_row["lines"]), hits=int(all_row["hits"]),
             bad=int(all_row["bad"]), h_content_bytes=hbytes, side_bytes=side,
             eff_GBps=None if hbytes is None or not best else round((hbytes + side) / best / 1e6, 1))
    gms = []
    for _ in range(3):
        with r.groups(100, True, 0, max_groups) as g:
            gms.append(round(g.ms, 4))
    hms = []
    for _ in range(3):
        r.histogram((synth.T0, 0), 60 * 10**9, 64)
        hms.append(round(r.hist_ms, 4))
    emit(case=name, groups_ms=gms, histogram_ms=hms)
    r.free()
    eng.close()
    del dev
    torch.cuda.empty_cache()


which = sys.argv[1]
now = synth.T0 + synth.SPAN + 1
if which in ("text", "all"):
    for nstreams in (16, 64):
        case(f"text {nstreams} x 64 MiB, no patterns", [64 << 20] * nstreams, synth.TEXT, {}, 10, None, -1, 3, 1 << 26)
if which in ("c5", "all"):
    sizes, kind, pats, permille, mode, desc = bench.config_table("c5")
    case("c5", sizes, kind, pats, permille, (now - bench.SINCE_S, 0), bench.TAIL, 5, 0)
