#!/usr/bin/env python3
"""The combined-strand CpG table's encoder (csrc/methdev.hip: bsc_meth_cpg_size_kernel / _write_kernel) beside the per-cytosine encoder,
in the same run on the same arrays, and bam2bcf --meth with and without --meth-merge file to file.  tools/bench_meth.py's sibling.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM: bsc_meth_sites_device (BSC_METH_CPG) and bsc_meth_cpg_sites_device in turn, --repeats times each
    behind --warmup — ms per call (HIP events: the size pass, the scan and the write pass), lines, pairs, bytes out.
(2) per kernel (--trace-dir DIR): the kernel times of a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d DIR`, a run of
    its own (tracing slows the host: its per-call times are not used), read from the trace it left: median ms per kernel name.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through the SAME bam2bcf -O u without a table, with --meth and with
    --meth --meth-merge, --runs runs each in turn: seconds without the context (best of the runs), bytes; the main file of either table
    run is checked to be the file of the run without it.

    python tools/bench_meth_cpg.py [--positions N] [--repeats 20] [--files] [--trace-dir DIR] [--out JSON]
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

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

KERNELS = ("bsc_meth_size_kernel", "bsc_meth_write_kernel", "bsc_meth_cpg_size_kernel", "bsc_meth_cpg_write_kernel")


def device_part(a):
    tpl, seq = B.synth_reads_host(M.SEED, 5_000, M.BLOCK, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    n1 = y - x + 1
    ref = B.synth_ref_host(M.SEED, x, n1 + 2)
    reps = max(1, -(-a.positions // n1))
    n = n1 * reps
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    res = {"positions": n, "block_positions": n1, "copies_of_the_block": reps, "coverage": 30, "repeats": a.repeats, "warmup": a.warmup}
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
        fns = {"per_cytosine": lambda: c.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_out.data_ptr(), cap, d_tot.data_ptr()),
               "combined": lambda: c.meth_cpg_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_out.data_ptr(), cap, d_tot.data_ptr())}
        ms = {k: [] for k in fns}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for both
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        for k, fn in fns.items():
            d_tot.zero_()
            fn()
            torch.cuda.synchronize()
            tot = [int(v) for v in d_tot.cpu()]
            assert tot[0] <= cap, "the stream did not fit"
            med = float(np.median(ms[k]))
            res[k] = {"ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4), "bytes_out": tot[0], "lines": tot[1],
                      "sum_a": tot[2], "sum_b": tot[3]}
            if k == "combined":
                res[k]["pairs"] = tot[4]
        assert (res["combined"]["sum_a"], res["combined"]["sum_b"]) == (res["per_cytosine"]["sum_a"], res["per_cytosine"]["sum_b"])
        assert res["combined"]["lines"] == res["per_cytosine"]["lines"] - res["combined"]["pairs"]
        res["combined_over_per_cytosine_ms"] = round(res["combined"]["ms_median"] / res["per_cytosine"]["ms_median"], 3)
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
    if all(k in out for k in KERNELS):
        for pre in ("bsc_meth", "bsc_meth_cpg"):
            out[pre + "_size_plus_write_ms"] = round(out[pre + "_size_kernel"]["ms_median"] + out[pre + "_write_kernel"]["ms_median"], 4)
        out["combined_over_per_cytosine"] = round(out["bsc_meth_cpg_size_plus_write_ms"] / out["bsc_meth_size_plus_write_ms"], 3)
    else:
        out["kernel_names_seen"] = sorted(k[:80] for k in dur)
    return out


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_meth_cpg")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    modes = {"Ou": ["-O", "u"], "Ou_meth": ["-O", "u", "--meth", os.path.join(d, "percyt.bed")],
             "Ou_meth_merge": ["-O", "u", "--meth", os.path.join(d, "merged.bed"), "--meth-merge"]}
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([exe, *modes[mode], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"))
        dt = time.time() - t0
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        st = json.loads(r.stderr.strip().splitlines()[-1])
        e = res.setdefault(mode, {"runs": []})
        e["runs"].append({"process_wall_s": round(dt, 3), "wall_without_context_s": st["wall_without_context_s"], "block_call_s": st["block_call_s"],
                          "encode_write_s": st["encode_write_s"]})
        e["bytes"] = os.path.getsize(ob)
        e["stdout"] = r.stdout.strip()
        print(mode, e["runs"][-1], flush=True)
    for k in modes:
        walls = [r_["wall_without_context_s"] for r_ in res[k]["runs"]]
        res[k]["best_wall_without_context_s"], res[k]["worst_wall_without_context_s"] = min(walls), max(walls)
    res["Ou_meth"]["table_bytes"] = os.path.getsize(os.path.join(d, "percyt.bed"))
    res["Ou_meth_merge"]["table_bytes"] = os.path.getsize(os.path.join(d, "merged.bed"))
    res["main_file_unchanged_by_either_table"] = all(M.sha_file(os.path.join(d, "Ou.out")) == M.sha_file(os.path.join(d, k + ".out")) for k in ("Ou_meth", "Ou_meth_merge"))
    res["report_unchanged_by_either_table"] = all(open(os.path.join(d, "Ou.json")).read() == open(os.path.join(d, k + ".json")).read() for k in ("Ou_meth", "Ou_meth_merge"))
    res["merge_over_plain"] = round(res["Ou_meth_merge"]["best_wall_without_context_s"] / res["Ou"]["best_wall_without_context_s"], 3)
    res["merge_over_per_cytosine"] = round(res["Ou_meth_merge"]["best_wall_without_context_s"] / res["Ou_meth"]["best_wall_without_context_s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=50_000_000)
    ap.add_argument("--file-positions", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--trace-dir", default=None, help="read the kernel trace a traced run of this tool left there")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": device_part(a)}
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
