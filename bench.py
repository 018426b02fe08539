#!/usr/bin/env python3
"""klogs filter-path benchmark.  Headline: BASELINE.json's north-star workload, config 5 ("C5"):

    32 GiB of 1-32 KiB JSON log lines per GPU in 28 pod/container streams (8 pods, each with
    1-2 init containers and 2 containers, the -i stream table of getPodLogs), 64 --match
    RE2-subset regexes, --since 5m --tail 100

A step = one full klf_run_device pass over the device-resident batch (memsets, scan with the
fused q-gram prefilter, tile index, factor verification, Glushkov NFA windows, counts, tail,
compaction), plus, at N > 1, the all-gather of the per-stream count records (+ the 64
per-pattern counts) over RCCL.  Weak scaling: every rank owns 32 GiB (8 pods x N, the stream
table LPT-sharded, shard.assign); value = all ranks' input bytes / max-over-ranks wall time.

The same line carries the other BASELINE configs under "extra.configs" (N = 1: C2, C1, C3,
C4; N > 1: C2 and C3 sharded), each measured the same way, and per config the honest step
bytes: the u64 line index counts only when the run wrote it (klf_result_index_mode "full");
runs that index only their tail windows (literal sets) or nothing (-l only) report a second
timing with KLF_FILTER_FULL_INDEX beside it.

A plain run does only what the headline needs: it loads the batch, warms up, times the
steps, writes the last timed step's outputs under --dump-outputs DIR, and prints the line.
Everything else lives behind --full: the other configs, the full-index second timing, the
one-shot (cold) cost, the checks against the C oracle, the stage split, the CPU baseline,
the card's state and the box probe, the committed rocprof evidence.

Launch: python bench.py [--gpus 1 --steps K --warmup W] [--full] [--dump-outputs DIR]; for
N > 1 the driver runs
`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

from klogs_amd import engine as E  # noqa: E402  (binds to torch's HIP runtime)
from klogs_amd import shard, synth  # noqa: E402

METRIC = "filtered log GB/s (whole node) at 1/2/4/8 MI355X; % of HBM peak"
HBM_PEAK_GBS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md
HEADLINE = "c5"
SINCE_S = 300  # --since 5m
TAIL = 100
PER_GPU = 32 << 30  # C4 / C5 bytes per GPU


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def oracle():
    """The C oracle (test infrastructure): only ever the checker / the CPU baseline leg,
    imported after the timed regions."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import c_oracle as co
    return co


def host_threads() -> int:
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))


# ---------------------------------------------------------------- configs -----------
def c5_pods(n_pods: int):
    return [(f"synthetic-{p}", [f"init-{k}" for k in range(1 + p % 2)], ["app", "sidecar"]) for p in range(n_pods)]


SHORT = {  # <= 110 characters: the driver's record cuts longer strings
    "c1": "C1: 1 x 64 MiB text stream, --since 5m --tail 100",
    "c2": "C2: 4 GiB JSON stream per GPU, --since 5m --tail 100, 1 --grep literal",
    "c3": "C3: 128 x 64 MiB text streams per GPU (1,024 over 8 GPUs), -l only (every line out)",
    "c4": "C4: 32 GiB/GPU mixed-length lines, 1,024 --grep literals, --since 5m --tail 100",
    "c5": "C5: 28 streams (-i), 32 GiB/GPU 1-32 KiB JSON lines, 64 --match regexes, --since 5m --tail 100",
}


def config_table(name: str, world: int = 1):
    """(stream sizes, generator kind, patterns, permille, mode, description) of BASELINE
    config `name`; at N ranks the per-GPU share times N (weak scaling)."""
    if name == "c1":  # the reference's own CPU-runnable case (BASELINE configs[0])
        return [64 << 20], synth.TEXT, {}, 10, "since+tail", \
            "C1: one 64 MiB stream (lognormal line lengths, median 96 B), --since 5m --tail 100"
    if name == "c2":
        return [4 << 30] * world, synth.JSON, dict(grep=[synth.NEEDLE]), 10, "since+tail", \
            (f"C2: one 4 GiB JSON log stream per GPU (x {world}), --since 5m --tail 100 --grep "
             + synth.NEEDLE.decode())
    if name == "c3":  # one GPU's share of C3 at 8 GPUs: 256 pods x 4 containers / 8
        return [64 << 20] * (128 * world), synth.TEXT, {}, 10, "-l", \
            (f"C3: 128 x 64 MiB streams per GPU (x {world}; 256 pods x 4 containers over 8 GPUs), -l selection "
             "only: no --since, no --tail, no grep (every line out, prefix stripped)")
    if name == "c4":
        n = 8 * world
        return [PER_GPU // 8] * n, synth.MIXED, dict(grep=synth.c4_literals(1024)), 5, "since+tail", \
            (f"C4: 8 streams per GPU (x {world}) of mixed-length lines (16 B-8 KiB, lognormal), 1,024 --grep "
             "literals (6-24 B, 0.5% of lines hold one), --since 5m --tail 100")
    if name == "c5":
        from klogs_amd import host as H
        table = H.stream_table(c5_pods(8 * world), init=True)  # getPodLogs order with -i (cmd/root.go:240-262)
        w = [1 if is_init else 4 for _, _, is_init in table]
        sizes = [PER_GPU * world * x // sum(w) for x in w]
        return sizes, synth.LONGJSON, dict(match=synth.c5_regexes()), 5, "since+tail", \
            (f"C5: {len(table)} streams (8 pods per GPU x {world}, 1-2 init containers + 2 containers each, -i), "
             "32 GiB per GPU of 1-32 KiB JSON lines, 64 --match RE2-subset regexes (0.5% of lines match one, "
             "1% hold a factor but no match), --since 5m --tail 100")
    raise ValueError(name)


def scan_kernel_name(name: str, pats: dict) -> str:
    if name == "c2":
        return "k_scan<literal>"
    if not pats:
        return "k_scan<plain>"
    return "k_scan<general: fused q-gram prefilter>"


def load_batch(sizes, kind, permille, ids, local):
    """Streams `ids` of the config generated on the host and copied into one device batch."""
    lens = [synth.size(kind, 42, i, sizes[i], permille=permille) for i in ids]
    seg_base, total = E.layout(lens)
    dev = torch.empty(total, dtype=torch.uint8, device=f"cuda:{local}")
    h = np.empty(max(lens) + 1, dtype=np.uint8)
    for j, i in enumerate(ids):
        synth.generate_into(h, kind, 42, i, sizes[i], permille=permille)
        dev[int(seg_base[j]):int(seg_base[j]) + lens[j]].copy_(torch.from_numpy(h[:lens[j]]))
    torch.cuda.synchronize()
    return dev, seg_base, lens


# ---------------------------------------------------------------- GPU state ---------
def gpu_state(local: int) -> dict:
    """This rank's card as numbers only (rocm-smi): sclk / mclk MHz, package power W,
    junction / memory temperature C, so a box-to-box spread can be attributed; {"error": ...}
    when rocm-smi cannot say.  (Round 5 kept rocm-smi's whole text fields: ~1.2 KB per config,
    which pushed the headline's verdict out of the driver's 8 KB stdout tail.)"""
    import re
    try:
        bus = None
        try:
            p = torch.cuda.get_device_properties(local)
            bus = getattr(p, "pci_bus_id", None)
        except Exception:
            pass
        out = subprocess.run(["rocm-smi", "--showbus", "-c", "-P", "-t", "--json"], capture_output=True,
                             text=True, timeout=30)
        d = json.loads(out.stdout[out.stdout.find("{"):])
        cards = {k: v for k, v in d.items() if k.startswith("card")}
        mine = [v for v in cards.values()
                if bus is not None and any(str(x).lower().endswith(f"{bus:02x}:00.0") for x in v.values())]
        v = (mine or list(cards.values()) or [{}])[0]

        def num(*keys):
            for f, x in v.items():
                fl = f.lower()
                if all(k in fl for k in keys):
                    m = re.search(r"-?\d+(?:\.\d+)?", str(x))
                    if m:
                        return float(m.group())
            return None
        return {"sclk_mhz": num("sclk", "speed"), "mclk_mhz": num("mclk", "speed"), "power_w": num("power"),
                "t_junction_c": num("temperature", "junction"), "t_mem_c": num("temperature", "memory"),
                "card_matched": bool(mine)}
    except Exception as ex:  # noqa: BLE001 (diagnostic only)
        return {"error": f"{type(ex).__name__}: {ex}"[:120]}


def box_probe(local: int) -> dict:
    """This box's own HBM rates, so that a box-to-box spread of the scan can be attributed:
    the runtime's device-to-device copy (2 GiB read + 2 GiB written) and a read-only
    reduction (torch sum over 4 GiB), best of 5 each, timed with events on cuda:local."""
    try:
        n = 2 << 30
        src = torch.empty(n, dtype=torch.uint8, device=f"cuda:{local}").fill_(1)
        dst = torch.empty_like(src)
        rd = torch.empty(2 * n // 8, dtype=torch.int64, device=f"cuda:{local}").fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def best(f):
            f()
            ts = []
            for _ in range(5):
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            return min(ts)
        tc = best(lambda: dst.copy_(src))
        tr = best(lambda: rd.sum())
        out = {"d2d_copy_GBps": round(2 * n / tc / 1e6, 1), "read_sum_GBps": round(2 * n / tr / 1e6, 1),
               "how": "torch copy_ (2 GiB in + 2 GiB out) and int64 sum over 4 GiB, best of 5"}
        try:  # the clock a VALU loop holds (s_memtime / s_memrealtime over every CU)
            out["valu_loop_clock"] = E.debug_clock(local)
        except Exception as ex:  # noqa: BLE001 (diagnostic only)
            out["valu_loop_clock"] = {"error": f"{type(ex).__name__}: {ex}"[:120]}
        del src, dst, rd
        torch.cuda.empty_cache()
        return out
    except Exception as ex:  # noqa: BLE001 (diagnostic only)
        return {"error": f"{type(ex).__name__}: {ex}"[:200]}


# ---------------------------------------------------------------- bytes -------------
def step_bytes(n_in: int, tot: dict, n_streams: int, has_patterns: bool, index_full: bool) -> int:
    """SURVEY.md §8d B_alg = B_in + B_out + 8 (L + S) + ceil(L / 8), with the u64 line index
    counted only when the run wrote it, and the match bitmap only when the run has patterns."""
    b = n_in + tot["out_bytes"]
    if has_patterns:
        b += (tot["lines"] + 7) // 8
    if index_full:
        b += 8 * (tot["lines"] + n_streams)
    return b


# ---------------------------------------------------------------- outputs -----------
DUMP_CAPS = {"out_bytes": 6 << 20, "line_offsets": 2 << 20, "match_bits": 4 << 20}  # entries: 56 MiB in all


def dump_outputs(r, n_streams: int, ddir: str, suffix: str = "") -> None:
    """--dump-outputs: what a caller of the timed path receives from result `r` (the last
    timed step's), as DIR/<name>.npy: `counts` (float64 [streams, 6]: lines, parsed, since_ok,
    matched, selected, out_bytes), `out_bytes` (float32: every stream's selected bytes, in
    stream order), `line_offsets` (float64: every stream's u64 line offsets, exact below
    2^53) and `match_bits` (float32: the match bitmaps' bytes).  An array longer than its
    DUMP_CAPS entry is cut to a fixed sample of its positions (seeded by its length alone, in
    ascending order), so two builds that compute the same arrays write the same files."""
    os.makedirs(ddir, exist_ok=True)
    outs, counts, lines, bits = [], [], [], []
    for i in range(n_streams):
        so = r.stream(i)
        outs.append(so.out)
        counts.append([so.counts[k] for k in ("lines", "parsed", "since_ok", "matched", "selected", "out_bytes")])
        lines.append(r.lines(i))
        bits.append(r.match_bits(i))

    def sample(a, cap):
        if a.size <= cap:
            return a
        return a[np.sort(np.random.default_rng(a.size).choice(a.size, cap, replace=False))]
    arrays = {"counts": np.array(counts, dtype=np.float64).reshape(n_streams, 6),
              "out_bytes": sample(np.frombuffer(b"".join(outs), dtype=np.uint8), DUMP_CAPS["out_bytes"])
              .astype(np.float32),
              "line_offsets": sample(np.concatenate(lines), DUMP_CAPS["line_offsets"]).astype(np.float64),
              "match_bits": sample(np.frombuffer(b"".join(bits), dtype=np.uint8), DUMP_CAPS["match_bits"])
              .astype(np.float32)}
    for k, a in arrays.items():
        np.save(os.path.join(ddir, f"{k}{suffix}.npy"), a)
    log(f"[dump] {sum(a.nbytes for a in arrays.values())} B of outputs under {ddir}")


# ---------------------------------------------------------------- one config (N = 1) -
def run_config(name: str, args, local: int, now: int, headline: bool = False, dump_dir=None) -> dict:
    sizes, kind, pats, permille, mode, desc = config_table(name)
    t = time.time()
    dev, seg_base, lens = load_batch(sizes, kind, permille, list(range(len(sizes))), local)
    log(f"[{name}] generated + uploaded {sum(lens)} B in {time.time() - t:.1f}s")
    since, tail = ((None, -1) if mode == "-l" else ((now - SINCE_S, 0), TAIL))
    stream = torch.cuda.current_stream()
    state0 = gpu_state(local) if args.full else None
    eng = E.Engine(local, hip_stream=stream.cuda_stream, **pats)
    ptr = dev.data_ptr()
    n = sum(lens)

    def timed(steps, warmup, **kw):
        for _ in range(warmup):
            eng.run_device(ptr, seg_base, lens, since=since, tail=tail, **kw).free()
        torch.cuda.synchronize()
        scan, copy, dev_ms = [], [], []
        t0 = time.perf_counter()
        last = None
        for i in range(steps):
            r = eng.run_device(ptr, seg_base, lens, since=since, tail=tail, **kw)
            tm = r.timing()
            scan.append(tm[6])
            copy.append(tm[7])
            dev_ms.append(tm[4])
            if i + 1 < steps:
                r.free()
            else:
                last = r
        torch.cuda.synchronize()
        return (time.perf_counter() - t0), last, float(np.mean(scan)), float(np.mean(copy)), float(np.mean(dev_ms))

    dt, last, scan_ms, copy_ms, dev_ms = timed(args.steps, args.warmup)
    tot = last.totals()
    index_mode = last.index_mode()
    has_pats = bool(pats)
    alg = step_bytes(n, tot, len(lens), has_pats, index_mode == "full")
    ms_step = dt / args.steps * 1e3
    out = {"workload": desc, "workload_short": SHORT[name], "streams": len(lens), "bytes": n, "lines": tot["lines"],
           "value_GBps": round(n * args.steps / dt / 1e9, 1), "ms_per_step": round(ms_step, 4),
           "device_ms_per_step": round(dev_ms, 4), "line_index": index_mode}
    # the dominant kernel: the scan, except C3 (-l only, every line out) where the dense copy
    # k_tcopy takes ~60 % of the step; its algorithmic bytes are the bytes it must move, the
    # selected content read once and written once (2 B_out)
    compaction = last.compaction()
    out["compaction"] = compaction
    if mode == "-l" and compaction == "one_pass":  # the scan compacts in place: it reads and writes
        k_alg, k_ms, k_name = n + tot["out_bytes"], scan_ms, "k_scan<plain, one-pass compaction>"
    elif mode == "-l":
        k_alg, k_ms, k_name = 2 * tot["out_bytes"], copy_ms, "k_tcopy"
    else:
        k_alg, k_ms, k_name = n, scan_ms, scan_kernel_name(name, pats)
    k_ms = max(k_ms, 1e-9)  # (0: a build without the dispatch events, KLF_SCAN_EVENTS=0)
    out["roofline"] = {"bound": "hbm", "kernel": k_name, "achieved": round(k_alg / k_ms / 1e6, 1),
                       "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(k_alg / k_ms / 1e6 / HBM_PEAK_GBS, 4),
                       "alg_bytes_per_launch": k_alg, "avg_launch_ms": round(k_ms, 4),
                       "frac_source": "HIP events carrying the kernel dispatch's own start / end timestamps "
                                      "(hipExtLaunchKernel on the launch stream), this run's timed steps"}
    if mode == "-l" and compaction == "one_pass":
        out["roofline"]["alg_bytes_note"] = "the one-pass scan reads the input once and writes the output once"
    elif mode == "-l":
        out["roofline"]["alg_bytes_note"] = ("k_tcopy moves the selected contents: B_out read + B_out written "
                                             "(the input's 31-B prefixes are skipped in place)")
        out["scan"] = {"kernel": "k_scan<plain>", "avg_launch_ms": round(scan_ms, 4),
                       "frac": round(n / max(scan_ms, 1e-9) / 1e6 / HBM_PEAK_GBS, 4)}
    out["step_alg_bytes"] = alg
    out["step_alg_frac_of_peak"] = round(alg / (ms_step / 1e3) / 1e9 / HBM_PEAK_GBS, 4)
    out["step_alg_frac_of_peak_device"] = round(alg / (dev_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4)
    out["step_bytes_rule"] = ("B_in + B_out" + (" + ceil(L/8) match bitmap" if has_pats else "")
                              + (" + 8 (L + S) u64 line index (written by the run)" if index_mode == "full" else
                                 " (the u64 line index is not written by this run: see full_index)"))
    out["matched_lines"], out["selected_lines"], out["out_bytes"] = tot["matched"], tot["selected"], tot["out_bytes"]
    if dump_dir:
        dump_outputs(last, len(lens), dump_dir)
    if not args.full:  # a plain run: the timed steps (and their outputs) only
        last.free()
        eng.close()
        del dev
        torch.cuda.empty_cache()
        return out
    # the step that writes every line's u64 offset too (KLF_FILTER_FULL_INDEX), beside it
    if index_mode != "full":
        last.free()
        last = None
        fsteps = max(3, args.steps // 2)
        fdt, flast, _, _, fdev = timed(fsteps, 1, full_index=True)
        ftot = flast.totals()
        assert flast.index_mode() == "full" and ftot == tot, (flast.index_mode(), ftot, tot)
        falg = step_bytes(n, ftot, len(lens), has_pats, True)
        out["full_index"] = {"ms_per_step": round(fdt / fsteps * 1e3, 4), "steps": fsteps,
                             "value_GBps": round(n * fsteps / fdt / 1e9, 1), "step_alg_bytes": falg,
                             "step_alg_frac_of_peak": round(falg / (fdt / fsteps) / 1e9 / HBM_PEAK_GBS, 4),
                             "device_ms_per_step": round(fdev, 4)}
        last = flast
    out["cold"] = cold_run(local, pats, ptr, seg_base, lens, since, tail)
    # checks after the timed regions
    co = None
    if not args.no_verify:
        co = oracle()
    if name in ("c1", "c2") and co is not None:  # the whole stream: bytes, counts, every line offset
        h = np.empty(lens[0] + 1, dtype=np.uint8)
        synth.generate_into(h, kind, 42, 0, sizes[0], permille=permille)
        ref_out, ref_lo, _, ref_c = co.filter_stream(h[:lens[0]], since, tail, pats.get("grep", []), want_bits=False)
        so = last.stream(0)
        out["verified_vs_oracle"] = bool(so.out == ref_out and all(so.counts[k] == ref_c[k] for k in ref_c)
                                         and np.array_equal(last.lines(0), ref_lo))
        out["verify"] = {"scope": "the whole stream: output bytes, all counts, every u64 line offset (C oracle)"}
        if name == "c2" and not args.no_capture:
            out["capture_path"] = capture_path(local, pats, h[:lens[0]], since, tail, so.out, args.capture_piece)
        del h
    write = None
    if name == "c3" and not args.no_write:
        write = write_path(last, lens, sizes, kind, permille, co)
        out["write_path"] = write
        if co is not None and "verified_vs_c_oracle" in write:
            out["verified_vs_oracle"] = write["verified_vs_c_oracle"]
            out["verify"] = {"scope": f"every stream ({write['verified_streams']}) as written to its file (C oracle)"}
    if name in ("c4", "c5") and co is not None:
        del dev  # the checks regenerate the streams on the host
        torch.cuda.empty_cache()
        dev = None
        v = verify_large(name, sizes, lens, kind, permille, pats, since, tail, last, co)
        out["verified_vs_oracle"] = v.pop("ok")
        out["verify"] = v
    if dev is not None:
        last.free()
        last = None
        staged = eng.run_device(ptr, seg_base, lens, since=since, tail=tail, stage_times=True)
        stage = staged.timing()
        staged.free()
    else:  # the batch was dropped for the checks: the stage split of the timed runs' last
        stage = last.timing()
    out["stage_ms"] = [round(x, 4) for x in stage]
    out["stage_names"] = ["scan stage", "matchers", "counts+tail", "compaction", "total", "memsets", "k_scan",
                          "k_tcopy"]
    if last is not None:
        last.free()
    eng.close()
    del dev
    torch.cuda.empty_cache()
    out["gpu_state"] = {"before": state0, "after": gpu_state(local)}
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(name, kind, pats, permille, since, tail, headline)
    return out


def capture_path(local, pats, host, since, tail, want, piece) -> dict:
    """§8f-2, C2 at N = 1: the product's host entry points on this run's bytes -- klf_stage in
    pieces (io.Copy's role) into pinned chunks, then klf_run (DMA H2D from the pinned chunks
    + the whole filter) and the output D2H.  Reported beside `value`, never as it."""
    n = len(host)
    ceng = E.Engine(local, **pats)
    runs = []
    for _ in range(2):  # the first pays the pinned-chunk allocation
        ceng.reset()
        ceng.set_streams(1)
        t0 = time.perf_counter()
        for off in range(0, n, piece):
            ceng.stage_array(0, host[off:off + piece])
        t1 = time.perf_counter()
        r = ceng.run(since=since, tail=tail, n_streams=1)
        got = r.stream(0).out
        t2 = time.perf_counter()
        r.free()
        runs.append((t1 - t0, t2 - t1, got == want))
    ceng.close()
    st_s, run_s, same = runs[-1]
    return {"stage_GBps": round(n / st_s / 1e9, 2), "h2d_filter_d2h_GBps": round(n / run_s / 1e9, 2),
            "end_to_end_GBps": round(n / (st_s + run_s) / 1e9, 2), "piece_bytes": piece,
            "staging": "pinned 64 MiB chunks (hipHostMalloc, reused across runs)",
            "output_matches_device_run": bool(same and runs[0][2])}


def write_path(last, lens, sizes, kind, permille, co) -> dict:
    """§8f-3 output write path (C3): every stream into its own file (klf_result_write);
    every file checked against the C oracle (one host thread per stream)."""
    wdir = tempfile.TemporaryDirectory(prefix="klf_c3_")
    paths = [os.path.join(wdir.name, f"pod{i // 4}__c{i % 4}.log") for i in range(len(lens))]
    tw = time.perf_counter()
    try:
        wbytes = last.write_files(paths)
    except E.KlfError as ex:  # e.g. no room for 6.9 GB in the temp dir: reported, not fatal
        wdir.cleanup()
        return {"error": str(ex)}
    wdt = time.perf_counter() - tw
    write = {"GBps": round(wbytes / wdt / 1e9, 2), "bytes": wbytes, "files": len(paths), "s": round(wdt, 3),
             "how": "klf_result_write: 64 MiB pinned D2H chunks, double-buffered, 8 writer threads each owning "
                    "whole files, into page-cache files under " + os.path.dirname(wdir.name)}
    if co is not None:
        def check(i):
            h = np.empty(lens[i] + 1, dtype=np.uint8)
            synth.generate_into(h, kind, 42, i, sizes[i], permille=permille, threads=1)
            want = co.filter_stream(h[:lens[i]], co.GO_ZERO_TIME, -1, [], want_lines=False, want_bits=False)[0]
            with open(paths[i], "rb") as f:  # the written file, i.e. the D2H + write path too
                return f.read() == want
        tv = time.perf_counter()
        with ThreadPoolExecutor(min(host_threads(), len(lens))) as ex:
            ok = list(ex.map(check, range(len(lens))))
        write["verified_vs_c_oracle"] = all(ok)
        write["verified_streams"] = len(ok)
        write["failed_streams"] = [i for i, x in enumerate(ok) if not x]
        write["verify_s"] = round(time.perf_counter() - tv, 1)
    wdir.cleanup()
    return write


def verify_large(name, sizes, lens, kind, permille, pats, since, tail, r, co) -> dict:
    """Checks the last timed run of C4 / C5 against the C oracle, every stream in full, one
    host thread per stream: output bytes, all counts and the match bitmap.  C4: Aho-Corasick
    over the 1,024 literals.  C5: the oracle's own Go-regexp restatement (ko_filter_rx:
    oracle/klf_oracle_rx.c, its own parser, Thompson NFA + lazy DFA behind a required-literal
    pass; tests/test_oracle.py checks it against the Python oracle)."""
    t = time.perf_counter()
    got = [(r.stream(i), r.match_bits(i)) for i in range(len(lens))]
    sn = since if since is not None else co.GO_ZERO_TIME
    rs = co.RegexSet(pats["match"]) if "match" in pats else None

    def check(i):
        h = np.empty(lens[i] + 1, dtype=np.uint8)
        synth.generate_into(h, kind, 42, i, sizes[i], permille=permille, threads=1)
        if rs is not None:
            out, _, bits, c = co.filter_stream_rx(h[:lens[i]], sn, tail, rs, want_lines=False)
        else:
            out, _, bits, c = co.filter_stream(h[:lens[i]], sn, tail, pats["grep"], want_lines=False)
        so, gbits = got[i]
        return so.out == out and gbits == bits and all(so.counts[k] == c[k] for k in c)
    with ThreadPoolExecutor(min(host_threads(), len(lens))) as ex:
        ok = list(ex.map(check, range(len(lens))))
    bad = [i for i, x in enumerate(ok) if not x]
    scope = ("every stream in full: output bytes, all counts, match bitmap ("
             + ("C oracle ko_filter_rx: own Go-regexp restatement" if rs is not None else "C oracle, Aho-Corasick")
             + ")")
    short = (f"all {len(lens)} streams: out bytes, counts, match bitmap vs "
             + ("C oracle ko_filter_rx (own Go-regexp leg)" if rs is not None else "C oracle (Aho-Corasick)"))
    return {"ok": not bad, "streams": len(lens), "failed_streams": bad, "scope": scope, "scope_short": short,
            "s": round(time.perf_counter() - t, 1)}


def cold_run(local: int, pats: dict, ptr: int, seg_base, lens, since, tail: int) -> dict:
    """One-shot cost, as one klogs invocation pays it (klf_run once per
    run): a fresh engine (klf_open: pattern compile + table uploads) and its first run on
    the device-resident batch, host wall clock; beside it the same engine's second run."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = E.Engine(local, hip_stream=torch.cuda.current_stream().cuda_stream, **pats)
    t1 = time.perf_counter()
    r = eng.run_device(ptr, seg_base, lens, since=since, tail=tail)
    t2 = time.perf_counter()
    r.free()
    t3 = time.perf_counter()
    r = eng.run_device(ptr, seg_base, lens, since=since, tail=tail)
    t4 = time.perf_counter()
    r.free()
    # the same warm engine after 3 ms with the GPU idle (about the host work in front of a
    # cold run's kernels): a long VALU-bound scan runs slower after an idle gap (C5 6.67 ms
    # back to back, 7.25 ms after 3 ms, 7.87 ms after 30 ms: gpurun_out/r5o), which the
    # cold run pays too
    time.sleep(0.003)
    t5 = time.perf_counter()
    r = eng.run_device(ptr, seg_base, lens, since=since, tail=tail)
    t6 = time.perf_counter()
    r.free()
    eng.close()
    return {"open_ms": round((t1 - t0) * 1e3, 3), "first_run_ms": round((t2 - t1) * 1e3, 3),
            "cold_ms": round((t2 - t0) * 1e3, 3), "second_run_ms": round((t4 - t3) * 1e3, 3),
            "ratio": round((t2 - t0) / max(t4 - t3, 1e-9), 3),
            "warm_run_after_3ms_idle_ms": round((t6 - t5) * 1e3, 3),
            "ratio_vs_warm_after_idle": round((t2 - t0) / max(t6 - t5, 1e-9), 3)}


# ---------------------------------------------------------------- CPU baseline ------
def cpu_baseline(name, kind, pats, permille, since, tail, headline: bool) -> dict:
    """The C restatement (oracle/klf_oracle_c.c, klf_oracle_rx.c) timed on this box's host
    cores over a bounded sample of the same generator and shape (rank 0, N = 1): one core
    (the baseline object itself), and T threads with one stream each (the reference runs one
    goroutine per stream).  The headline's sample is ~10 s of single-core work.  Literal
    paths: ko_filter (memmem / Aho-Corasick).  C5: ko_filter_rx, the C leg's own Go-regexp
    restatement behind a required-literal pass."""
    co = oracle()
    threads = host_threads()
    sample = {"c1": 64 << 20, "c2": 64 << 20, "c3": 64 << 20, "c4": 4 << 20, "c5": 16 << 20}[name]
    nstreams = 1 if name == "c1" else threads
    streams = [synth.generate(kind, 7, i, sample, permille=permille) for i in range(nstreams)]
    grep = pats.get("grep", [])
    sn = since if since is not None else co.GO_ZERO_TIME
    if "match" in pats:
        rs = co.RegexSet(pats["match"])

        def one(b):
            return co.filter_stream_rx(b, sn, tail, rs, want_lines=False, want_bits=False)
        impl = "oracle/klf_oracle_rx.c ko_filter_rx (own Go-regexp restatement: Thompson NFA + lazy DFA behind " \
               "a required-literal Aho-Corasick pass)"
    else:
        def one(b):
            return co.filter_stream(b, sn, tail, grep, want_lines=False, want_bits=False)
        impl = "oracle/klf_oracle_c.c ko_filter (memchr line split, Go time.Parse restated, memmem / Aho-Corasick, " \
               "kubelet tail + since)"

    def timed(f, budget):
        k, tt = 0, 0.0
        while tt < budget and k < 2048:
            t0 = time.perf_counter()
            f()
            tt += time.perf_counter() - t0
            k += 1
        return k, tt
    k, tt = timed(lambda: one(streams[0]), 10.0 if headline else 3.0)
    res = {"value": round(sample * k / tt / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "port",
           "sample": f"{k} passes, one {sample >> 20} MiB {name.upper()} stream, 1 thread, {tt:.1f} s "
                     f"({'oracle ko_filter_rx' if 'match' in pats else 'oracle ko_filter'})",
           "impl": impl,
           "host_cpus": os.cpu_count(), "host_cpus_affinity": len(os.sched_getaffinity(0))}
    if nstreams > 1:
        with ThreadPoolExecutor(threads) as ex:
            k, tt = timed(lambda: list(ex.map(one, streams)), 4.0 if headline else 3.0)
        res["threads"] = {"value": round(sample * threads * k / tt / 1e9, 4), "unit": "GB/s", "cores": threads,
                          "kind": "port", "sample": f"{k} passes over {threads} streams of {sample >> 20} MiB, one "
                                                    f"host thread per stream, {tt:.1f} s",
                          "note": f"threads = min(16, OMP_NUM_THREADS) of the box's {os.cpu_count()} CPUs "
                                  "(the GPU box's CPU share is 16)"}
    if headline:  # the reference client's own work: io.Copy of each body into its file
        res["copy_bound"] = copy_bound(streams[0])
    return res


def copy_bound(host: bytes) -> dict:
    """klogs itself only io.Copy's each body into its file (cmd/root.go:359-374): a host
    memcpy and a page-cache file write of the sample bound that from above."""
    src = np.frombuffer(host, dtype=np.uint8)
    dst = np.empty_like(src)
    t = time.perf_counter()
    for _ in range(8):
        np.copyto(dst, src)
    t_cp = (time.perf_counter() - t) / 8
    with tempfile.NamedTemporaryFile(prefix="klf_cpy_") as f:
        t = time.perf_counter()
        mv = memoryview(src)
        off = 0
        while off < len(src):
            off += os.write(f.fileno(), mv[off:off + (64 << 20)])
        t_w = time.perf_counter() - t
    return {"memcpy_1t_GBps": round(len(src) / t_cp / 1e9, 2), "file_write_GBps": round(len(src) / t_w / 1e9, 2)}


# ---------------------------------------------------------------- N > 1 -------------
def run_sharded(name: str, args, world: int, rank: int, local: int, coll_dev, now: int) -> dict:
    """BASELINE config `name` across ranks: the stream table LPT-assigned
    (shard.assign), each rank one device batch of its own streams, then the one all-gather
    of per-stream count records (+ per-pattern counts) per step over RCCL.  value = all
    ranks' bytes / max-over-ranks time.  After the timed region every rank checks its own
    rows of the gathered table and verifies its first and last stream in full against the C
    oracle; the flags are all-reduced (MIN)."""
    sizes, kind, pats, permille, mode, desc = config_table(name, world)
    since, tail = ((None, -1) if mode == "-l" else ((now - SINCE_S, 0), TAIL))
    lens_all = [synth.size(kind, 42, i, sz, permille=permille) for i, sz in enumerate(sizes)]
    mine = shard.local_streams(lens_all, world, rank)
    t = time.time()
    dev, seg_base, lens = load_batch(sizes, kind, permille, mine, local)
    log(f"[rank {rank}] {name} share: {len(mine)} streams, {sum(lens)} B in {time.time() - t:.1f}s")
    eng = E.Engine(local, hip_stream=torch.cuda.current_stream().cuda_stream, **pats)
    ptr = dev.data_ptr()
    npat = len(pats.get("match", [])) + len(pats.get("grep", []))
    pending = []

    def records(r):
        recs = {}
        for j, sid in enumerate(mine):
            c = r.stream_counts(j)
            if npat:
                c = dict(c, patterns=r.pattern_counts(j))
            recs[sid] = c
        return recs

    def step():
        r = eng.run_device(ptr, seg_base, lens, since=since, tail=tail, pattern_counts=bool(npat))
        # the records go out while the next step filters; every gather is waited for before
        # the timed region closes
        pending.append(shard.gather_counts_async(records(r), lens_all, world, device=coll_dev, n_patterns=npat))
        if len(pending) > 1:
            pending.pop(0).wait()
        return r

    def finish():
        while pending:
            step.table = pending.pop(0).wait()
    for _ in range(args.warmup):
        step().free()
    finish()
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    scan_ms = []
    for i in range(args.steps):
        r = step()
        scan_ms.append(r.timing()[6])
        if i + 1 < args.steps:
            r.free()
        else:
            last = r
    finish()
    torch.cuda.synchronize()
    dist.barrier()
    dt = time.perf_counter() - t0
    tt = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())
    mine_rec = records(last)
    fields = shard.RECORD_FIELDS[1:]
    rec_ok = all(step.table[sid].tolist() == [mine_rec[sid][k] for k in fields] + list(mine_rec[sid].get("patterns", []))
                 for sid in mine)
    rec_ok = rec_ok and int(step.table[:, 0].sum()) > 0 and int(step.table[:, 5].sum()) > 0
    tot = last.totals()
    index_mode = last.index_mode()
    n_mine = sum(lens)
    scan_avg = max(float(np.mean(scan_ms)), 1e-9)
    if args.dump_outputs and name == HEADLINE:
        dump_outputs(last, len(lens), args.dump_outputs, suffix=f".rank{rank}" if rank else "")
    ver = None
    if args.full and not args.no_verify:
        co = oracle()
        rs = co.RegexSet(pats["match"]) if "match" in pats else None
        sn = since if since is not None else co.GO_ZERO_TIME
        got = {j: (last.stream(j), last.match_bits(j) if npat else None) for j in sorted({0, len(mine) - 1})}
        del dev
        torch.cuda.empty_cache()
        dev = None

        def check(j):
            i = mine[j]
            hh = np.empty(lens[j] + 1, dtype=np.uint8)
            synth.generate_into(hh, kind, 42, i, sizes[i], permille=permille)
            if rs is not None:
                out, _, bits, c = co.filter_stream_rx(hh[:lens[j]], sn, tail, rs, want_lines=False)
            else:
                out, _, bits, c = co.filter_stream(hh[:lens[j]], sn, tail, pats.get("grep", []), want_lines=False,
                                                   want_bits=bool(npat))
            so, gb = got[j]
            return so.out == out and all(so.counts[k] == c[k] for k in c) and (gb is None or gb == bits)
        tv = time.perf_counter()
        with ThreadPoolExecutor(len(got)) as ex:
            ver = all(ex.map(check, list(got)))
        log(f"[rank {rank}] {name} verified={ver} ({time.perf_counter() - tv:.1f}s)")
    # every rank's scan fraction and step bytes, reduced: MIN fraction, SUM bytes
    alg_mine = step_bytes(n_mine, tot, len(lens), bool(npat), index_mode == "full")
    red = torch.tensor([alg_mine, n_mine], dtype=torch.float64, device=coll_dev)
    dist.all_reduce(red, op=dist.ReduceOp.SUM)
    fmin = torch.tensor([n_mine / scan_avg / 1e6 / HBM_PEAK_GBS], dtype=torch.float64, device=coll_dev)
    dist.all_reduce(fmin, op=dist.ReduceOp.MIN)
    flags = torch.tensor([int(rec_ok), -1 if ver is None else int(ver)], dtype=torch.int64, device=coll_dev)
    dist.all_reduce(flags, op=dist.ReduceOp.MIN)
    last.free()
    eng.close()
    del dev
    torch.cuda.empty_cache()
    total_in = int(sum(lens_all))
    out = {"workload": desc, "workload_short": SHORT[name].replace("per GPU", f"per GPU x {world}")
                                                          .replace("/GPU", f"/GPU x {world}"),
           "streams": len(lens_all), "bytes": total_in,
           "value_GBps": round(total_in * args.steps / dt / 1e9, 1), "ms_per_step": round(dt / args.steps * 1e3, 4),
           "line_index": index_mode,
           "rank0": {"streams": len(mine), "bytes": n_mine,
                     "scan": {"kernel": scan_kernel_name(name, pats), "avg_launch_ms": round(scan_avg, 4),
                              "alg_bytes_per_launch": n_mine,
                              "frac": round(n_mine / scan_avg / 1e6 / HBM_PEAK_GBS, 4)}},
           "scan_frac_min_over_ranks": round(float(fmin.item()), 4),
           "step_alg_bytes_all_ranks": int(red[0].item()),
           "step_alg_frac_of_peak_per_gpu": round(float(red[0].item()) / (dt / args.steps) / 1e9 / HBM_PEAK_GBS
                                                  / world, 4),
           "records_consistent": bool(flags[0].item()),
           "collective": f"one all-gather per step of {len(lens_all)} x {shard.NREC + npat} int64 records "
                         f"({'RCCL' if coll_dev != 'cpu' else 'gloo'})"}
    if ver is not None:
        out["verified_vs_oracle"] = bool(flags[1].item() == 1)
        out["verify_scope"] = ("every rank: first + last stream in full (out bytes, counts"
                               + (", match bitmap" if npat else "") + ") vs the C oracle")
    return out


# ---------------------------------------------------------------- profiles ----------
def committed(cfg: str, scan_ms: float):
    """The committed rocprofv3 evidence for cfg's roofline kernel (profiles/<round>/[<box>/]
    traffic.json and summary.json, scripts/collect_profiles.py): the per-launch HBM traffic
    and the rocprof-trace fraction of the profile whose steady kernel time is nearest this
    run's, and how far apart the two times are; a match is a profile within 3 %, else the
    nearest is cited with match false.  Only the newest round holding cfg is searched: an
    older round profiled older code, whose time matching would be a coincidence.  (Round 5
    always cited the newest summary, from a different board than the driver's run.)"""
    best = None
    rounds = sorted({p.relative_to(ROOT / "profiles").parts[0]
                     for p in ROOT.glob("profiles/r*/**/summary.json")
                     if (json.loads(p.read_text()).get(cfg) or {}).get("steady_us")}, reverse=True)
    if not rounds:
        return {}
    for sm in sorted(ROOT.glob(f"profiles/{rounds[0]}/**/summary.json"), reverse=True):
        s = json.loads(sm.read_text()).get(cfg)
        if not s or not s.get("steady_us"):
            continue
        rel = abs(s["steady_us"] / 1e3 - scan_ms) / max(scan_ms, 1e-9)
        if best is None or rel < best[0] - 1e-9:
            best = (rel, sm, s)
    if best is None:
        return {}
    rel, sm, s = best
    out = {"frac_rocprof_committed": s.get("frac_rocprof_steady") or s.get("frac_rocprof"),
           "rocprof_source": str(sm.relative_to(ROOT)), "rocprof_steady_ms": round(s["steady_us"] / 1e3, 4),
           "rocprof_vs_this_run": round(rel, 4), "rocprof_match_3pct": bool(rel <= 0.03)}
    tr = sm.parent / "traffic.json"
    if not tr.exists():  # (a trace-only profile of another board: the round's counter passes, same build)
        tr = ROOT / "profiles" / rounds[0] / "traffic.json"
    if tr.exists():
        t = json.loads(tr.read_text()).get(cfg)
        if t:
            out["traffic"] = int(t["traffic_bytes"])
            out["traffic_source"] = str(tr.relative_to(ROOT))
    return out


# ---------------------------------------------------------------- main --------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also everything beside the headline's timed steps: the other configs, the full-index "
                         "timing, the cold run, the checks against the C oracle, the stage split, the CPU "
                         "baseline, the card's state, the box probe (the --no-* options below trim it)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs of the headline config as DIR/<name>.npy "
                         "(dump_outputs; rank k > 0 writes <name>.rank<k>.npy)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-write", action="store_true", help="skip C3's file write path")
    ap.add_argument("--no-capture", action="store_true", help="skip C2's host-staged capture-path timing")
    ap.add_argument("--capture-piece", type=int, default=4 << 20, help="klf_stage piece size of the capture path")
    ap.add_argument("--extra-configs", default=None,
                    help="comma list ('' = none); default c2,c1,c3,c4 at N = 1, c2,c3 (sharded) at N > 1")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps needs at least 1 and --warmup at least 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # Rehearsal knob for a one-GPU box: KLF_BENCH_BACKEND=gloo lets N ranks share cuda:0
    # (RCCL refuses two ranks on one device).  The driver's runs use RCCL, one GPU per rank.
    backend = os.environ.get("KLF_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    coll_dev = f"cuda:{local}" if backend == "nccl" else "cpu"
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    now = synth.T0 + synth.SPAN + 1  # "now" = end of the streams + 1 s
    extras = args.extra_configs
    if extras is None:
        extras = "c2,c1,c3,c4" if world == 1 else "c2,c3"
    extras = [x for x in extras.split(",") if x and x != HEADLINE] if args.full else []

    probe = box_probe(local) if args.full else None
    if world == 1:
        head = run_config(HEADLINE, args, local, now, headline=True, dump_dir=args.dump_outputs)
        value, ms = head["value_GBps"], head["ms_per_step"]
        roof = dict(head.pop("roofline"))
        cpu = head.pop("cpu_baseline", None)
    else:
        head = run_sharded(HEADLINE, args, world, rank, local, coll_dev, now)
        value, ms = head["value_GBps"], head["ms_per_step"]
        sc = head["rank0"]["scan"]
        roof = {"bound": "hbm", "kernel": sc["kernel"], "achieved": round(sc["alg_bytes_per_launch"]
                                                                           / sc["avg_launch_ms"] / 1e6, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": sc["frac"],
                "alg_bytes_per_launch": sc["alg_bytes_per_launch"], "avg_launch_ms": sc["avg_launch_ms"],
                "frac_min_over_ranks": head["scan_frac_min_over_ranks"],
                "frac_source": "rank 0's k_scan dispatch events (hipExtLaunchKernel), this run"}
        cpu = None  # (rank 0 at N = 1 only)
    if probe and "read_sum_GBps" in probe:  # the scan against what this box reads at all
        roof["frac_of_box_read_rate"] = round(roof["achieved"] / probe["read_sum_GBps"], 4)
    roof["traffic"] = None
    if args.full:
        roof.update(committed(HEADLINE, roof["avg_launch_ms"]))
    # the headline's evidence where the driver keeps it (its record keeps `config` and
    # `roofline`, not `extra`, and cuts long strings): short keys, numbers and flags
    cfg = {"workload": head["workload_short"], "streams": head["streams"], "global_bytes": head["bytes"],
           "parallelism": f"stream table LPT-sharded over {world} GPU(s), one process per GPU"}
    for k in ("line_index", "step_alg_bytes", "step_alg_frac_of_peak", "device_ms_per_step",
              "step_alg_frac_of_peak_device", "step_alg_bytes_all_ranks", "step_alg_frac_of_peak_per_gpu",
              "scan_frac_min_over_ranks", "records_consistent", "verified_vs_oracle"):
        if k in head:
            cfg[k] = head[k]
    if "verify" in head:
        cfg["verify_scope"] = head["verify"].get("scope_short", head["verify"].get("scope", ""))[:110]
    elif "verify_scope" in head:
        cfg["verify_scope"] = head["verify_scope"][:110]
    if isinstance(head.get("cold"), dict):
        cfg["cold_ratio"] = head["cold"].get("ratio")
        cfg["cold_ms"] = head["cold"].get("cold_ms")
    if isinstance(head.get("gpu_state"), dict):
        cfg["gpu_after"] = head["gpu_state"].get("after")
    res = {
        "metric": METRIC,
        "value": value,
        "unit": "GB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "full": bool(args.full),
        "ms_per_step": ms,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic: seeded kubelet log streams (31-B RFC3339Nano prefix, monotonic timestamps over "
                "60 min); C5: 1-32 KiB JSON lines",
        "config": cfg,
        "roofline": roof,
        "cpu_baseline": cpu,
        "extra": {"headline": head, "configs": {}, "box_probe": probe},
    }
    for name in extras:
        try:
            if world == 1:
                res["extra"]["configs"][name] = run_config(name, args, local, now)
            else:
                res["extra"]["configs"][name + "_sharded"] = run_sharded(name, args, world, rank, local, coll_dev, now)
        except Exception as ex:  # noqa: BLE001 -- an extra config's failure is reported, not fatal
            if world > 1:
                raise
            res["extra"]["configs"][name] = {"error": f"{type(ex).__name__}: {ex}"[:400]}
            log(f"[{name}] failed: {ex}")
        torch.cuda.empty_cache()
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
