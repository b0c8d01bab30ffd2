#!/usr/bin/env python3
"""The allele-specific methylation table (csrc/asmdev.hip: the SNP pass, the windows, the records' heads, the walk, Fisher's test, the text
encoder) on resident reads, beside the read-level CpG table's entry (bsc_cpg_reads_device, whose walk is the comparison) and the variant
selection (bsc_variants_sites_device) over the same arrays in the same run, and bam2bcf -O b with and without --meth-asm file to file.
tools/bench_cpg_reads.py's sibling.

(1) device: one block of --positions (default 50 M) at 30x, the device-resident reads of bench.py's roofline_reads (bs_call_amd.reads.
    synth_block); the dense records are the block's own: bsc_reads_chain_device over the same reads leaves them in HBM, with the
    heterozygous calls the synthetic reads give.  --repeats times each behind --warmup, in turn, by HIP events:
      cpg_reads      bsc_cpg_reads_device: site pass, scan, heads, walk
      var_select     bsc_variants_sites_device: select, scan, pack
      asm            bsc_asm_device: site pass, SNP pass, windows, heads, walk, Fisher's test (it waits twice for a count)
      asm_text       bsc_asm_text_device over the records and the device count
    The records and totals of a first part of the block are checked against the host form (csrc/asm.c) over the same templates and records.
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d
    DIR` left — a run of its own: every bsc_asm_* kernel, bsc_cr_walk_kernel, bsc_cr_site_kernel and bsc_var_select_kernel.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O b without and with --meth-asm; --runs runs each in
    turn: seconds without the context, best and worst.  --parent-exe PATH: a third mode, the same plain run through another build's binary.

    python tools/bench_asm.py [--positions N] [--repeats 20] [--files] [--trace-dir DIR] [--out JSON]
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
from bs_call_amd.abi import VCF_CORE  # noqa: E402
from bs_call_amd.caller import asm_pairs_host  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

PAR = {"min_phred": 20, "pass_only": 0, "max_dist": 500, "min_cov": 2}
CR_PAR = {"min_sites": 4, "min_cov": 1}


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
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    res = {"positions": n, "coverage": 30, "templates": len(tpl), "read_bytes": int(seq.size), "repeats": a.repeats, "warmup": a.warmup, "params": PAR}
    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_core, d_aux = z(64 * n), z(64 * n)
        c.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core.data_ptr(), d_aux.data_ptr(), reg_stop=y,
                             stream=stream)
        c.block_status(stream)
        # a first part of the block: the device's records against the host form over the same templates and the same dense records
        m = min(n, 300_000)
        k = int(np.searchsorted(tpl["pos"][:, 0], x + m))  # (the templates come in the order of their start positions)
        core1 = d_core[: 64 * m].cpu().numpy().view(VCF_CORE)
        want, w_n, w_tot = asm_pairs_host(tpl[:k], seq, x, x + m - 1, ref[: m + 2], core1, None, c.tables()[1], 20, PAR)
        d_p1, d_n, d_tot = z(32 * (w_n + 1)), z(8), z(64)
        c.asm_device(d_tpl.data_ptr(), k, d_seq.data_ptr(), seq.size, x, x + m - 1, d_ref.data_ptr(), d_core.data_ptr(), None, d_p1.data_ptr(), w_n, d_n.data_ptr(),
                     d_tot.data_ptr(), params=PAR, stream=stream)
        torch.cuda.synchronize()
        assert int(d_n.cpu().numpy().view(np.uint64)[0]) == w_n, "the count differs from the host form's"
        assert tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64)) == w_tot, "the totals differ from the host form's"
        assert d_p1.cpu().numpy()[: 32 * w_n].tobytes() == want.tobytes(), "the records differ from the host form's"
        res["checked_against_the_host_form"] = {"positions": m, "templates": k, "snps": w_tot[0], "records": w_n}
        del d_p1
        # the whole block: the count first, then the room
        c.asm_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core.data_ptr(), None, None, 0, d_n.data_ptr(), d_tot.data_ptr(),
                     params=PAR, stream=stream)
        torch.cuda.synchronize()
        n_pairs = int(d_n.cpu().numpy().view(np.uint64)[0])
        d_pairs = z(32 * (n_pairs + 1))
        n_sites_cap = n // 2 + 1
        d_sites, d_sn, d_stot = z(40 * n_sites_cap), z(8), z(64)
        sel_cap = n // 64 + 65536
        d_recs, d_vn, d_vtot = z(128 * sel_cap), z(8), z(80)
        text_cap = 80 * n_pairs + 4096
        d_text, d_t2 = z(text_cap), z(16)
        fns = {
            "cpg_reads": lambda: c.cpg_reads_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_sites.data_ptr(), n_sites_cap,
                                                    d_sn.data_ptr(), d_stot.data_ptr(), params=CR_PAR, stream=stream),
            "var_select": lambda: c.variants_sites_device(d_core.data_ptr(), d_aux.data_ptr(), None, n, d_recs.data_ptr(), sel_cap, d_vn.data_ptr(), d_vtot.data_ptr(),
                                                          stream=stream),
            "asm": lambda: c.asm_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core.data_ptr(), None, d_pairs.data_ptr(),
                                        n_pairs, d_n.data_ptr(), d_tot.data_ptr(), params=PAR, stream=stream),
            "asm_text": lambda: c.asm_text_device(d_pairs.data_ptr(), d_n.data_ptr(), n_pairs, b"chr1", d_text.data_ptr(), text_cap, d_t2.data_ptr(), params=PAR,
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
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
        t2 = [int(v) for v in d_t2.cpu().numpy().view(np.uint64)]
        assert t2[0] <= text_cap and tot[1] == n_pairs
        res.update({k_: stats(v) for k_, v in ms.items()})
        med = lambda k_: res[k_]["ms_median"]
        res.update({"snps": tot[0], "records": n_pairs, "lines": t2[1], "table_bytes": t2[0], "totals": tot,
                    "variant_records": int(d_vn.cpu().numpy().view(np.uint64)[0]), "asm_over_cpg_reads": round(med("asm") / med("cpg_reads"), 4)})
    return res


def trace_part(d):
    """Median kernel times from the kernel trace(s) rocprofv3 left under d, by kernel name."""
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].replace("void ", "").split("(")[0].split("<")[0].replace(".kd", "").strip()
                if name.startswith("bsc_asm_") or name in ("bsc_cr_walk_kernel", "bsc_cr_site_kernel", "bsc_cr_init_kernel", "bsc_var_select_kernel"):
                    out.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6)
    if not out:
        raise SystemExit("no kernel trace under " + d)
    res = {}
    for k, v in out.items():  # (the checked part's dispatches are the small ones: keep those within a factor of four of the largest)
        big = [t for t in v if t >= 0.25 * max(v)]
        res[k] = dict(stats(big), dispatches=len(big))
    return res


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_asm")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    tsv = os.path.join(d, "out.asm.tsv.gz")
    modes = {"Ob": (exe, ["-O", "b"]), "Ob_meth_asm": (exe, ["-O", "b", "--meth-asm", tsv])}
    if a.parent_exe:
        modes["Ob_parent"] = (a.parent_exe, ["-O", "b"])
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
    res["Ob_meth_asm"]["table_bytes"] = os.path.getsize(tsv)
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
    ap.add_argument("--parent-exe", default=None, help="with --files: another build's bam2bcf, run plain in turn with this one's")
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
