#!/usr/bin/env python3
"""The per-region fragment methylation summary (csrc/fragdev.hip: one walk behind the read-level table's site pass and scan) on resident reads,
against the epiallele table's and the PAT table's device calls over the same arrays in the same run, and bam2bcf -O b with and without
--meth-frags --meth-window 1000 file to file.  tools/bench_epi.py's sibling.

(1) device: one block of --positions (default 50 M) at 30x, the device-resident reads of bench.py's roofline_reads (bs_call_amd.reads.
    synth_block), the templates, read bytes and reference codes in HBM.  --repeats times each behind --warmup, in turn, by HIP events:
      epi            bsc_epi_device: site pass, scan, heads, the epiallele walk — the walk to compare with
      pat            bsc_pat_device: site pass, scan, slots, walk, sort, collapse
      pat_pull       bsc_pat_device and its records copied to page-locked host memory: what a user does today before the regions meet the reads
      frag_windows   bsc_frag_device under the 1 kb windows of the block (the region summary's first set)
      frag_random    bsc_frag_device under 100 000 random intervals of 200 .. 5 000 bases (its second set)
    The accumulators and totals of a first part of the block are checked against the host form (csrc/frag.c) over the same templates.
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d
    DIR` left — a run of its own.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O b without and with --meth-frags --meth-window 1000,
    and through another build's binary (--parent-exe); --runs runs each in turn, every run reported.

    python tools/bench_frag.py [--positions N] [--repeats 20] [--files [--parent-exe EXE]] [--trace-dir DIR] [--out JSON]
"""
import argparse
import csv
import glob
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
from bs_call_amd import reads as R  # noqa: E402
from bs_call_amd.caller import frag_regions_host  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

PAR = {"min_sites": 3, "u_max_pct": 25, "m_min_pct": 75}
EPI_PAR = {"min_cov": 10}
PAT_PAR = {"min_sites": 1}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def region_sets(x, y):
    """The region summary's two sets over the block: the 1 kb windows, and 100 000 random intervals of 200 .. 5 000 bases, sorted."""
    starts = np.arange((x - 1) // 1000 * 1000, y, 1000, dtype=np.int64)
    windows = np.stack([starts, starts + 1000], axis=1)
    rng = np.random.default_rng(100_000)
    s = rng.integers(x - 1, y, 100_000)
    rnd = np.stack([s, s + rng.integers(200, 5001, 100_000)], axis=1)
    rnd = rnd[np.lexsort((rnd[:, 1], rnd[:, 0]))]
    return {"windows": windows.astype(np.uint32), "random": rnd.astype(np.uint32)}


def device_part(a):
    x = 1000
    tpl, seq, y = R.synth_block(M.SEED + 2, x, a.positions, 30, chunk=1_000_000)
    n = y - x + 1
    ref = B.synth_ref_host(M.SEED + 2, x, n + 2)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    sets = region_sets(x, y)
    res = {"positions": n, "coverage": 30, "templates": len(tpl), "read_bytes": int(seq.size), "repeats": a.repeats, "warmup": a.warmup, "params": PAR,
           "regions": {k: len(v) for k, v in sets.items()}}
    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_tot = z(64)
        # a first part of the block: the device's accumulators against the host form over the same templates
        m = min(n, 300_000)
        k = int(np.searchsorted(tpl["pos"][:, 0], x + m))  # (the templates come in the order of their start positions)
        for name, regs in sets.items():
            part = regs[regs[:, 0] < x + m][:2_000]
            want, w_tot = frag_regions_host(tpl[:k], seq, x, x + m - 1, ref[: m + 2], part, 20, PAR)
            c.frag_attach(part)
            c.frag_device(d_tpl.data_ptr(), k, d_seq.data_ptr(), seq.size, x, x + m - 1, d_ref.data_ptr(), d_tot.data_ptr(), params=PAR, stream=stream)
            torch.cuda.synchronize()
            assert tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64)[:8]) == w_tot, "the totals differ from the host form's"
            assert c.frag_read().tolist() == want.tolist(), "the accumulators differ from the host form's"
            res.setdefault("checked_against_the_host_form", {})[name] = {"positions": m, "templates": k, "regions": len(part), "fragments": w_tot[1]}
        cap = n // 2 + 1
        d_win, d_n = z(72 * cap), z(8)
        # the PAT table's room: asked for by a first call
        d_nr, d_pt = z(8), z(64)
        c.pat_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), 0, 0, d_nr.data_ptr(), d_pt.data_ptr(), params=PAT_PAR,
                     stream=stream)
        torch.cuda.synchronize()
        n_rec = int(d_nr.cpu().numpy().view(np.uint64)[0])
        d_rec = z(24 * (n_rec + 1))
        h_rec = torch.empty(24 * (n_rec + 1), dtype=torch.uint8).pin_memory()
        run_epi = lambda: c.epi_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_win.data_ptr(), cap, d_n.data_ptr(),
                                       d_tot.data_ptr(), params=EPI_PAR, stream=stream)
        run_pat = lambda: c.pat_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_rec.data_ptr(), n_rec, d_nr.data_ptr(),
                                       d_pt.data_ptr(), params=PAT_PAR, stream=stream)
        run_frag = lambda: c.frag_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_tot.data_ptr(), params=PAR,
                                         stream=stream)

        def pat_pull():
            run_pat()
            h_rec.copy_(d_rec, non_blocking=True)

        ms = {}
        for name, fn in (("epi", run_epi), ("pat", run_pat), ("pat_pull", pat_pull)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
        for name, regs in sets.items():
            c.frag_attach(regs)
            for _ in range(a.warmup):
                run_frag()
            torch.cuda.synchronize()
            c.frag_reset()
            run_frag()
            torch.cuda.synchronize()
            res["frag_" + name + "_totals"] = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)[:8]]
            acc = c.frag_read()
            res["frag_" + name + "_regions_with_fragments"] = int((acc[:, 0] > 0).sum())
            for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for all
                for k_, fn in (("epi", run_epi), ("pat", run_pat), ("pat_pull", pat_pull), ("frag_" + name, run_frag)):
                    ms.setdefault(k_, []).append(timed(fn))
        res.update({k_: stats(v) for k_, v in ms.items()})
        med = lambda k_: res[k_]["ms_median"]
        res.update({"pat_records": n_rec, "pat_record_bytes": 24 * n_rec, "accumulator_bytes": {k_: 64 * len(v) for k_, v in sets.items()},
                    "frag_windows_over_epi": round(med("frag_windows") / med("epi"), 4), "frag_random_over_epi": round(med("frag_random") / med("epi"), 4),
                    "frag_windows_over_pat_pull": round(med("frag_windows") / med("pat_pull"), 4),
                    "frag_random_over_pat_pull": round(med("frag_random") / med("pat_pull"), 4)})
    return res


def trace_part(d):
    """Median kernel times from the kernel trace(s) rocprofv3 left under d, this feature's and its neighbours' kernels by name."""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                rows.append((row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
    if not rows:
        raise SystemExit("no kernel trace under " + d)
    short = lambda full: full.replace("void ", "").split("(")[0].split("<")[0].replace(".kd", "").strip()
    out = {}
    for full, ms in rows:
        name = short(full)
        if name.startswith(("bsc_cr_", "bsc_epi_", "bsc_pat_", "bsc_frag_")):
            out.setdefault(name, []).append(ms)
    res = {}
    for k, v in out.items():  # (the checked part's dispatches are the small ones: keep those within a factor of four of the largest)
        big = [t for t in v if t >= 0.25 * max(v)]
        res[k] = dict(stats(big), dispatches=len(big))
    return res


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_frag")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    tsv = os.path.join(d, "out.frags.tsv")
    modes = {"Ob": [exe, "-O", "b"], "Ob_meth_frags": [exe, "-O", "b", "--meth-window", "1000", "--meth-frags", tsv]}
    if a.parent_exe:
        modes["Ob_parent"] = [a.parent_exe, "-O", "b"]
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([*modes[mode], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"), timeout=600)
        dt = time.time() - t0
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        st = json.loads(r.stderr.strip().splitlines()[-1])
        e = res.setdefault(mode, {"runs": []})
        e["runs"].append({"process_wall_s": round(dt, 3), "wall_without_context_s": st["wall_without_context_s"], "block_call_s": st["block_call_s"],
                          "encode_write_s": st["encode_write_s"]})
        e["stdout"] = r.stdout.strip()
        print(mode, e["runs"][-1], flush=True)
    for k in modes:
        walls = [r_["wall_without_context_s"] for r_ in res[k]["runs"]]
        res[k]["best_wall_without_context_s"], res[k]["worst_wall_without_context_s"] = min(walls), max(walls)
    res["Ob"]["main_bytes"] = os.path.getsize(os.path.join(d, "Ob.out"))
    res["Ob_meth_frags"]["table_bytes"] = os.path.getsize(tsv)
    res["main_file_unchanged"] = all(M.sha_file(os.path.join(d, "Ob.out")) == M.sha_file(os.path.join(d, k + ".out")) for k in modes)
    res["report_unchanged"] = all(open(os.path.join(d, "Ob.json")).read() == open(os.path.join(d, k + ".json")).read() for k in modes)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=50_000_000)
    ap.add_argument("--file-positions", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--parent-exe", default=None, help="with --files: another build's bam2bcf, run in turn beside this one's")
    ap.add_argument("--trace-dir", default=None, help="read the kernel trace a traced run of this tool left there")
    ap.add_argument("--skip-device", action="store_true", help="with --trace-dir or --files: leave the device part out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if not a.skip_device:
        res["device"] = device_part(a)
        print(json.dumps(res), flush=True)
    if a.trace_dir:
        res["kernels"] = trace_part(a.trace_dir)
    if a.files:
        res["bam2bcf"] = files_part(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
