#!/usr/bin/env python3
"""The BED index scan (csrc/beddev.hip: bsc_bed_count_kernel, the scan, bsc_bed_write_kernel) beside the table encoder it indexes, in the
same run on the same arrays, and bam2bcf -O b --meth with and without --meth-index file to file.  tools/bench_meth.py's sibling.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM; per table (per cytosine, combined strand): the encoder (bsc_meth_sites_device /
    bsc_meth_cpg_sites_device) and bsc_bed_scan_device over the table it left, in turn, --repeats times each behind --warmup — ms per call
    (HIP events), entries, lines.  The scan's intervals are cut as the encoder's tiles cut them in size: the block entry scans by the
    encoder's own tile offsets, which stay inside the context; here every k-th line start, k = the table's lines per 64 positions, taken
    from the table on the device.
(2) per kernel (--trace-dir DIR): the kernel times of a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d DIR`, a run of
    its own, read from the trace it left: median ms per kernel name.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O b --meth t.bed.gz without and with --meth-index
    tbi, and through --parent-exe (the parent commit's binary) without it, --runs runs each in turn: seconds without the context, every
    run reported; the table and the main file of the indexed run are checked to be those of the run without it, and methbed.fetch through
    the .tbi is checked against a scan of the whole inflated table.

    python tools/bench_meth_index.py [--positions N] [--repeats 20] [--files [--parent-exe PATH]] [--trace-dir DIR] [--out JSON]
"""
import argparse
import csv
import glob
import gzip
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bs_call_amd as B  # noqa: E402
from bs_call_amd import methbed  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

KERNELS = ("bsc_bed_count_kernel", "bsc_bed_write_kernel", "bsc_meth_size_kernel", "bsc_meth_write_kernel", "bsc_meth_cpg_size_kernel",
           "bsc_meth_cpg_write_kernel")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def device_part(a):
    import ctypes as C

    tpl, seq = B.synth_reads_host(M.SEED, 5_000, M.BLOCK, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    n1 = y - x + 1
    ref = B.synth_ref_host(M.SEED, x, n1 + 2)
    reps = max(1, -(-a.positions // n1))
    n = n1 * reps
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    res = {"positions": n, "block_positions": n1, "copies_of_the_block": reps, "coverage": 30, "repeats": a.repeats, "warmup": a.warmup, "min_shift": 14}
    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_core1 = torch.zeros(n1 * 64, dtype=torch.uint8, device="cuda")
        d_aux1 = torch.zeros(n1 * 64, dtype=torch.uint8, device="cuda")
        c.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core1.data_ptr(), d_aux1.data_ptr())
        torch.cuda.synchronize()
        d_core, d_aux = d_core1.repeat(reps), d_aux1.repeat(reps)
        del d_core1, d_aux1
        cap = n * 16 + 4096
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(5, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(3, dtype=torch.int64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        encs = {"per_cytosine": lambda: c.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_out.data_ptr(), cap, d_tot.data_ptr()),
                "combined": lambda: c.meth_cpg_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_out.data_ptr(), cap, d_tot.data_ptr())}
        for k, enc in encs.items():
            enc()
            torch.cuda.synchronize()
            tot = [int(v) for v in d_tot.cpu()]
            assert tot[0] <= cap, "the table did not fit"
            # NOTE the repeated block's positions start over with every copy: the scan is told so by interval borders at the copies' seams
            # (a start below the one before it inside an interval is an error), which every k-th line start does not promise — so the
            # borders are the line starts k apart WITHIN a copy, and every copy's first line
            nl = torch.nonzero(d_out[: tot[0]] == 10).flatten() + 1  # the offsets behind every newline: the next line's start
            starts = torch.cat([torch.zeros(1, dtype=nl.dtype, device="cuda"), nl[:-1]])
            per_copy = tot[1] // reps
            assert per_copy * reps == tot[1], "the copies do not hold the same lines"
            k_lines = max(1, round(tot[1] / (n / 64)))
            idx = torch.arange(tot[1], device="cuda")
            pick = (idx % per_copy) % k_lines == 0
            d_sync = torch.cat([starts[pick], torch.tensor([tot[0]], dtype=nl.dtype, device="cuda")]).contiguous()
            n_sync = int(d_sync.numel()) - 1
            cap_e = n_sync + 2 * ((n * reps) >> 14) + 2 * reps + 16
            d_ent = torch.zeros(cap_e * 3, dtype=torch.int64, device="cuda")
            del nl, starts, idx, pick

            def scan():
                rc = c._L.bsc_bed_scan_device(c._h, C.c_void_p(d_out.data_ptr()), tot[0], C.c_void_p(d_sync.data_ptr()), n_sync, 14,
                                              C.c_void_p(d_ent.data_ptr()), cap_e, C.c_void_p(d_st.data_ptr()), st)
                assert rc == 0, c._L.bsc_last_error()

            for _ in range(a.warmup):
                enc()
                scan()
            torch.cuda.synchronize()
            ms_e, ms_s = [], []
            for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for both
                ms_e.append(timed(enc))
                ms_s.append(timed(scan))
            stt = [int(v) for v in d_st.cpu()]
            assert stt[2] == 0 and stt[1] == tot[1] and stt[0] <= cap_e, stt
            res[k] = {"table_bytes": tot[0], "lines": tot[1], "intervals": n_sync, "lines_per_interval": k_lines, "entries": stt[0],
                      "encoder_ms_median": round(float(np.median(ms_e)), 4), "encoder_ms_min": round(min(ms_e), 4), "encoder_ms_max": round(max(ms_e), 4),
                      "scan_ms_median": round(float(np.median(ms_s)), 4), "scan_ms_min": round(min(ms_s), 4), "scan_ms_max": round(max(ms_s), 4)}
            res[k]["scan_over_encoder"] = round(res[k]["scan_ms_median"] / res[k]["encoder_ms_median"], 3)
            del d_sync, d_ent
    return res


def trace_part(d):
    """Median kernel time per kernel name from the kernel trace(s) rocprofv3 left under d."""
    dur = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                dur.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    if not dur:
        raise SystemExit("no kernel trace under " + d)
    out = {}
    for full, v in dur.items():
        name = full.split("(")[0].replace(".kd", "").strip()
        if name in KERNELS:
            out[name] = {"dispatches": len(v), "ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
        elif "scan" in full.lower():
            out.setdefault("scan_kernels", {})[full[:80]] = {"dispatches": len(v), "ms_median": round(float(np.median(v)), 4)}
    return out


def fetch_check(table_path, n_queries=40):
    """methbed.fetch through the index beside table_path against one pass over the whole inflated table."""
    with open(table_path, "rb") as f:
        data = gzip.decompress(f.read())
    rng = np.random.default_rng(17)
    first = data[: data.index(b"\n")].split(b"\t")
    contig = first[0].decode()
    last_start = int(data[data.rindex(b"\n", 0, len(data) - 1) + 1 :].split(b"\t")[1])
    qs = [(int(s), int(s) + int(w)) for s, w in zip(rng.integers(0, last_start, n_queries), rng.choice([1, 2, 100, 16_384, 200_000], n_queries))]
    qs += [(16_383, 16_384), (16_384, 16_385), (0, 1 << 14), (last_start, last_start + 2)]
    # the whole table, every line: its two numbers (numpy's reader) and its offsets (the newlines)
    import io

    starts, ends = np.loadtxt(io.BytesIO(data), delimiter="\t", usecols=(1, 2), dtype=np.int64, unpack=True, comments=None)
    nl = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10) + 1
    offs = np.concatenate([[0], nl])
    assert len(starts) == len(nl)
    want = []
    for qa, qb in qs:
        hit = np.flatnonzero((starts < qb) & (ends > qa))
        want.append([data[offs[i] : offs[i + 1]] for i in hit])
    ix = methbed.read_index(table_path + ".tbi")
    ok = all(methbed.fetch(table_path, contig, qa, qb, index_path=ix) == w for (qa, qb), w in zip(qs, want))
    return {"queries": len(qs), "lines_returned": sum(len(w) for w in want), "fetch_equals_whole_table_scan": ok, "table_bytes_inflated": len(data)}


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_meth_index")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    modes = {"Ob_meth": (exe, ["-O", "b", "--meth", os.path.join(d, "plain.bed.gz")]),
             "Ob_meth_index_tbi": (exe, ["-O", "b", "--meth", os.path.join(d, "indexed.bed.gz"), "--meth-index", "tbi"])}
    if a.parent_exe:
        modes["parent_Ob_meth"] = (a.parent_exe, ["-O", "b", "--meth", os.path.join(d, "parent.bed.gz")])
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([modes[mode][0], *modes[mode][1], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"))
        dt = time.time() - t0
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        st = json.loads(r.stderr.strip().splitlines()[-1])
        e = res.setdefault(mode, {"runs": []})
        e["runs"].append({"process_wall_s": round(dt, 3), "wall_without_context_s": st["wall_without_context_s"], "block_call_s": st["block_call_s"],
                          "encode_write_s": st["encode_write_s"]})
        e["bytes"] = os.path.getsize(ob)
        print(mode, e["runs"][-1], flush=True)
    for k in modes:
        walls = [r_["wall_without_context_s"] for r_ in res[k]["runs"]]
        res[k]["best_wall_without_context_s"], res[k]["worst_wall_without_context_s"] = min(walls), max(walls)
        res[k]["table_bytes"] = os.path.getsize(modes[k][1][3])
    res["Ob_meth_index_tbi"]["index_bytes"] = os.path.getsize(os.path.join(d, "indexed.bed.gz.tbi"))
    same = lambda x, y_: M.sha_file(os.path.join(d, x)) == M.sha_file(os.path.join(d, y_))
    res["table_unchanged_by_the_index"] = same("plain.bed.gz", "indexed.bed.gz")
    res["main_file_unchanged_by_the_index"] = same("Ob_meth.out", "Ob_meth_index_tbi.out")
    if a.parent_exe:
        res["table_and_main_file_equal_the_parent_s"] = same("plain.bed.gz", "parent.bed.gz") and same("Ob_meth.out", "parent_Ob_meth.out")
    plain, idx = res["Ob_meth"], res["Ob_meth_index_tbi"]
    res["index_minus_plain_best_s"] = round(idx["best_wall_without_context_s"] - plain["best_wall_without_context_s"], 3)
    res["plain_runs_spread_s"] = round(plain["worst_wall_without_context_s"] - plain["best_wall_without_context_s"], 3)
    res["difference_resolved"] = abs(res["index_minus_plain_best_s"]) > res["plain_runs_spread_s"]
    res["fetch"] = fetch_check(os.path.join(d, "indexed.bed.gz"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=50_000_000)
    ap.add_argument("--file-positions", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--parent-exe", default=None, help="the parent commit's bam2bcf, for the runs without the index")
    ap.add_argument("--trace-dir", default=None, help="read the kernel trace a traced run of this tool left there")
    ap.add_argument("--skip-device", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d")}
    if not a.skip_device:
        res["device"] = device_part(a)
        print(json.dumps(res), flush=True)
    if a.trace_dir:
        res["kernels"] = trace_part(a.trace_dir)
    if a.files:
        res["bam2bcf"] = files_part(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
