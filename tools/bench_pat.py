#!/usr/bin/env python3
"""The per-read CpG pattern table, PAT (csrc/patdev.hip: the slot pass, the walk, the heads, the text encoder, with rocPRIM's radix sort of
csrc/sort.hip between walk and heads, behind the read-level table's site pass and scan) on resident reads, against the epiallele table
(bsc_epi_device, csrc/epidev.hip — a file this feature does not touch, so that kernel is the parent commit's) over the same arrays in the
same run, and bam2bcf -O b with and without --meth-pat file to file.  tools/bench_epi.py's sibling.

(1) device: one block of --positions (default 50 M) at 30x, the device-resident reads of bench.py's roofline_reads (bs_call_amd.reads.
    synth_block), the templates, read bytes and reference codes in HBM.  --repeats times each behind --warmup, in turn, by HIP events:
      epi            bsc_epi_device: site pass, scan, heads, the epiallele walk — the yardstick
      pat            bsc_pat_device: site pass, scan, slot pass, scan, the wait for the slot count, walk, sort, heads
      pat_text       bsc_pat_text_device over the walk's records and device count
    The records and totals of a first part of the block are checked against the host form (csrc/pat.c) over the same templates.
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d
    DIR` left — a run of its own: bsc_pat_slots_kernel, bsc_pat_walk_kernel, the sort's kernels (what runs between the walk and
    bsc_pat_flags_kernel, summed per call), bsc_pat_flags / _heads / _recs_kernel, bsc_pat_size / _write_kernel, bsc_epi_walk_kernel.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O b without and with --meth-pat and, with
    --parent-exe, through another build's binary; --runs runs each in turn: seconds without the context, every run reported.

    python tools/bench_pat.py [--positions N] [--repeats 20] [--files [--parent-exe EXE]] [--trace-dir DIR] [--out JSON]
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
from bs_call_amd.caller import pat_recs_host  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

EPI_PAR = {"min_cov": 10}
PAR = {"min_sites": 1}
REC = 24  # sizeof(bsc_pat_rec)
EPI_REC = 72


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def device_part(a):
    x = 1000
    tpl, seq, y = R.synth_block(M.SEED + 2, x, a.positions, 30, chunk=1_000_000)
    n = y - x + 1
    ref = B.synth_ref_host(M.SEED + 2, x, n + 2)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")  # noqa: E731
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    res = {"positions": n, "coverage": 30, "templates": len(tpl), "read_bytes": int(seq.size), "repeats": a.repeats, "warmup": a.warmup, "params": PAR, "epi_params": EPI_PAR}
    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        # a first part of the block: the device's records against the host form over the same templates
        m = min(n, 300_000)
        k = int(np.searchsorted(tpl["pos"][:, 0], x + m))  # (the templates come in the order of their start positions)
        want, w_n, w_tot = pat_recs_host(tpl[:k], seq, x, x + m - 1, ref[: m + 2], 20, PAR)
        d_r1, d_n, d_tot = z(REC * (w_n + 1)), z(8), z(64)
        c.pat_device(d_tpl.data_ptr(), k, d_seq.data_ptr(), seq.size, x, x + m - 1, d_ref.data_ptr(), d_r1.data_ptr(), w_n, d_n.data_ptr(), d_tot.data_ptr(),
                     params=PAR, stream=stream)
        torch.cuda.synchronize()
        assert int(d_n.cpu().numpy().view(np.uint64)[0]) == w_n, "the count differs from the host form's"
        assert tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64)) == w_tot, "the totals differ from the host form's"
        assert d_r1.cpu().numpy()[: REC * w_n].tobytes() == want.tobytes(), "the records differ from the host form's"
        res["checked_against_the_host_form"] = {"positions": m, "templates": k, "records": w_n}
        del d_r1
        cap = len(tpl) + len(tpl) // 8 + 1  # a piece a template and a few more
        e_cap = n // 2 + 1
        d_rec, d_win = z(REC * cap), z(EPI_REC * e_cap)
        d_n2, d_tot2 = z(8), z(64)
        c.pat_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_rec.data_ptr(), cap, d_n.data_ptr(), d_tot.data_ptr(),
                     params=PAR, stream=stream)
        torch.cuda.synchronize()
        n_rec = int(d_n.cpu().numpy().view(np.uint64)[0])
        assert n_rec <= cap, "more records than the room"
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
        text_cap = 64 * n_rec + 4096
        d_text, d_t2 = z(text_cap), z(16)
        fns = {
            "epi": lambda: c.epi_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_win.data_ptr(), e_cap, d_n2.data_ptr(),
                                        d_tot2.data_ptr(), params=EPI_PAR, stream=stream),
            "pat": lambda: c.pat_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_rec.data_ptr(), cap, d_n.data_ptr(),
                                        d_tot.data_ptr(), params=PAR, stream=stream),
            "pat_text": lambda: c.pat_text_device(d_rec.data_ptr(), d_n.data_ptr(), cap, b"chr1", 0, d_text.data_ptr(), text_cap, d_t2.data_ptr(), params=PAR,
                                                  stream=stream),
        }
        ms = {k_: [] for k_ in fns}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for all
            for k_, fn in fns.items():
                ms[k_].append(timed(fn))
        t2 = [int(v) for v in d_t2.cpu().numpy().view(np.uint64)]
        assert t2[0] <= text_cap and [int(v) for v in d_tot.cpu().numpy().view(np.uint64)] == tot
        res.update({k_: stats(v) for k_, v in ms.items()})
        bytes_in = int(seq.size) + 40 * len(tpl) + n + 2  # every read byte, template and reference code once
        med = lambda k_: res[k_]["ms_median"]  # noqa: E731
        res.update({"records": n_rec, "record_bytes": REC * n_rec, "lines": t2[1], "table_bytes": t2[0], "totals": tot,
                    "pieces_per_record": round(tot[1] / max(n_rec, 1), 3), "input_bytes": bytes_in, "pat_over_epi": round(med("pat") / med("epi"), 4)})
    return res


def trace_part(d):
    """Median kernel times from the kernel trace(s) rocprofv3 left under d: this feature's kernels by name; what runs between the walk and the
    flags pass is the sort, summed per call."""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
    if not rows:
        raise SystemExit("no kernel trace under " + d)
    rows.sort()
    short = lambda full: full.replace("void ", "").split("(")[0].split("<")[0].replace(".kd", "").strip()  # noqa: E731
    out, in_sort, acc, n_k = {}, False, 0.0, 0
    for _, full, ms in rows:
        name = short(full)
        if name == "bsc_pat_flags_kernel" and in_sort:
            out.setdefault("sort_kernels_between_walk_and_flags", []).append(acc)
            out.setdefault("sort_kernel_dispatches_per_call", []).append(n_k)
            in_sort = False
        if name.startswith("bsc_pat_") or name in ("bsc_epi_walk_kernel", "bsc_epi_init_kernel", "bsc_cr_site_kernel"):
            out.setdefault(name, []).append(ms)
        elif in_sort:
            acc += ms
            n_k += 1
        if name == "bsc_pat_walk_kernel":
            in_sort, acc, n_k = True, 0.0, 0
    res = {}
    for k, v in out.items():  # (the checked part's dispatches are the small ones: keep those within a factor of four of the largest)
        if k == "sort_kernel_dispatches_per_call":
            res[k] = max(v)
            continue
        big = [t for t in v if t >= 0.25 * max(v)]
        res[k] = dict(stats(big), dispatches=len(big))
    return res


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_pat")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    table = os.path.join(d, "out.pat.gz")
    modes = {"Ob": (exe, ["-O", "b"]), "Ob_meth_pat": (exe, ["-O", "b", "--meth-pat", table])}
    if a.parent_exe:
        modes["parent_Ob"] = (a.parent_exe, ["-O", "b"])
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([modes[mode][0], *modes[mode][1], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"), timeout=600)
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
    res["Ob_meth_pat"]["table_bytes"] = os.path.getsize(table)
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
    ap.add_argument("--parent-exe", default=None, help="with --files: another build's bam2bcf, run -O b beside this build's")
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
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
