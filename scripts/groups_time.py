#!/usr/bin/env python3
"""Times klf_result_groups (SPEC.md S4e, DESIGN.md "Grouped counts").

    python scripts/groups_time.py c5|text

c5: the bench's C5 batch and run (64 regexes, --since 5m --tail 100: a sparse H of long lines).
text: 16 and 64 TEXT streams of 64 MiB on an engine without patterns (every line in H).
Per case: the run, then klf_groups_ms of repeated calls with top = 100 and the digits masked and
not masked, with max_key = 64, and klf_timeline_ms on the same result as the yardstick (the
existing accessor that also reads every line's bytes; on c5 it covers the emitted lines only).
The bytes the call reads are reported as h_content_bytes (the contents of H without their '\n')
and side_bytes (index entries, meta, bitmap); eff_GBps is their sum over the best time.  Prints
one JSON line per measurement."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from klogs_amd import engine as E  # noqa: E402
from klogs_amd import synth  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def groups_ms(r, reps, **kw):
    ms, info = [], None
    for _ in range(reps):
        with r.groups(**kw) as g:
            ms.append(round(g.ms, 4))
            info = (g.n_groups, g.n_lines)
    return ms, info


def case(name, sizes, kind, pats, permille, since, tail, reps, timeline, max_groups):
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
            emit(case=name, unmasked_groups=g.n_groups, n_lines=g.n_lines, first_call_ms=round(g.ms, 4))
    except E.KlfError as ex:
        emit(case=name, unmasked_error=str(ex)[:200])
    if hbytes is None and not pats:  # every line out: out_bytes = the contents with their '\n'
        hbytes = tot["out_bytes"] - tot["lines"]
    nh = tot["matched"] if pats else tot["parsed"]
    side = 16 * nh + 2 * nh + ((tot["lines"] + 7) // 8 if pats else 2 * tot["lines"])  # index entries, meta, bitmap / meta
    for mask in (True, False):
        try:
            ms, info = groups_ms(r, reps, top=100, mask_digits=mask, max_key=0, max_groups=max_groups)
            best = min(ms)
            emit(case=name, mask=mask, ms=ms, n_groups=info[0], n_lines=info[1], h_content_bytes=hbytes,
                 side_bytes=side, eff_GBps=None if hbytes is None else round((hbytes + side) / best / 1e6, 1))
        except E.KlfError as ex:
            emit(case=name, mask=mask, error=str(ex)[:200])
    ms, info = groups_ms(r, 3, top=100, mask_digits=True, max_key=64, max_groups=max_groups)
    emit(case=name, mask=True, max_key=64, ms=ms, n_groups=info[0])
    with r.groups(5, True, 0, max_groups) as g:
        emit(case=name, top5=[(int(e["count"]), k[:80].decode("latin1")) for e, k in zip(g.entries, g.keys())])
    if timeline:
        tms = []
        for _ in range(3):
            tl = r.timeline()
            tms.append(round(tl.ms, 4))
            n, size = len(tl), tl.size
            tl.free()
        emit(case=name, timeline_ms=tms, timeline_entries=n, timeline_bytes=size)
    r.free()
    eng.close()
    del dev
    torch.cuda.empty_cache()


which = sys.argv[1]
now = synth.T0 + synth.SPAN + 1
if which == "text":
    for nstreams in (16, 64):
        case(f"text {nstreams} x 64 MiB, no patterns", [64 << 20] * nstreams, synth.TEXT, {}, 10, None, -1, 3, True, 1 << 26)
if which == "c5":
    sizes, kind, pats, permille, mode, desc = bench.config_table("c5")
    case("c5", sizes, kind, pats, permille, (now - bench.SINCE_S, 0), bench.TAIL, 5, True, 0)
