#!/usr/bin/env python3
"""The variant-only call set (csrc/variantsdev.hip: the select and pack kernels around the context's scan, then the BCF encoder over the
selection) on resident arrays, against the methylation table's size pass (bsc_meth_size_kernel, csrc/methdev.hip — a file this feature
does not touch, so the library's kernel is the parent commit's) on the same arrays in the same run, and bam2bcf -O b with and without
--variants file to file.  tools/bench_bigwig_cov.py's sibling.

(1) device: the per-position arrays and the byte per position the reads-in chain leaves for a 2 M-position block at 30x, repeated on the
    device to --positions (default 50 M) and resident in HBM.  --repeats times each behind --warmup, in turn, by HIP events:
      select_pack_emit   bsc_variants_sites_device with the chain's byte per position: select, scan, pack
      select_pack_core   the same with d_emit = NULL: core.emit alone gates, every position's head is read
      encode             bsc_bcf_block_device over the packed selection and its device count
      meth_sites         bsc_meth_sites_device (size pass, scan, write pass; it takes no emit-byte array) — the entry whose size pass is
                         the comparison
    The selection of ONE copy of the block is checked against the host form over the same arrays.
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d
    DIR` left — a run of its own: bsc_var_select_kernel by call (with and without the emit bytes: the calls alternate, the trace is cut
    at every select kernel), the scan's kernels behind it, bsc_var_pack_kernel, the encoder's kernels, bsc_meth_size_kernel.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O b without and with --variants; --runs runs each
    in turn: seconds without the context, best and worst.

    python tools/bench_variants.py [--positions N] [--repeats 20] [--files] [--trace-dir DIR] [--out JSON]
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
from bs_call_amd import variants  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)


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
    tpl, seq = B.synth_reads_host(M.SEED, 5_000, M.BLOCK, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    n1 = y - x + 1
    ref = B.synth_ref_host(M.SEED, x, n1 + 2)
    reps = max(1, -(-a.positions // n1))
    n = n1 * reps
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    res = {"positions": n, "block_positions": n1, "copies_of_the_block": reps, "coverage": 30, "repeats": a.repeats, "warmup": a.warmup}
    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_core1, d_aux1, d_len1 = z(n1 * 64), z(n1 * 64), z(n1)
        c.reads_chain_len_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core1.data_ptr(), d_aux1.data_ptr(),
                                 d_len1.data_ptr())
        torch.cuda.synchronize()
        # one copy of the block: the device's selection against the rule over the same arrays
        recs = np.concatenate([d_core1.cpu().numpy().reshape(-1, 64), d_aux1.cpu().numpy().reshape(-1, 64)], axis=1).reshape(-1).view(B.VCF_REC)
        emit1 = d_len1.cpu().numpy()[:n1]
        assert ((emit1 != 0) == (recs["core"]["emit"] != 0)).all(), "the chain's byte per position is not the records' emit flag"
        idx = variants.select(recs)
        want_tot = variants.totals(recs[idx])
        d_r1, d_n, d_tot = z(128 * (len(idx) + 1)), z(8), z(80)
        for emit in (d_len1.data_ptr(), None):
            c.variants_sites_device(d_core1.data_ptr(), d_aux1.data_ptr(), emit, n1, d_r1.data_ptr(), len(idx), d_n.data_ptr(), d_tot.data_ptr())
            torch.cuda.synchronize()
            assert int(d_n.cpu().numpy().view(np.uint64)[0]) == len(idx), "the count differs from the rule's"
            assert tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64)) == want_tot, "the totals differ from the rule's"
            assert d_r1.cpu().numpy()[: 128 * len(idx)].tobytes() == recs[idx].tobytes(), "the records differ from the rule's"
        emitted1 = int((emit1 != 0).sum())
        d_core, d_aux, d_len = d_core1.repeat(reps), d_aux1.repeat(reps), d_len1[:n1].repeat(reps)
        del d_core1, d_aux1, d_len1, d_r1
        sel = len(idx) * reps
        d_recs = z(128 * (sel + 1))
        enc_cap = 256 * sel + 4096
        d_enc, d_etot = z(enc_cap), z(24)
        meth_cap = 48 * emitted1 * reps + 4096
        d_meth, d_mtot = z(meth_cap), z(32)
        A = (d_core.data_ptr(), d_aux.data_ptr())
        fns = {
            "select_pack_emit": lambda: c.variants_sites_device(*A, d_len.data_ptr(), n, d_recs.data_ptr(), sel, d_n.data_ptr(), d_tot.data_ptr()),
            "select_pack_core": lambda: c.variants_sites_device(*A, None, n, d_recs.data_ptr(), sel, d_n.data_ptr(), d_tot.data_ptr()),
            "encode": lambda: c.bcf_block_device(d_recs.data_ptr(), d_n.data_ptr(), sel, 0, d_enc.data_ptr(), enc_cap, d_etot.data_ptr()),
            "meth_sites": lambda: c.meth_sites_device(*A, n, b"chr1", d_meth.data_ptr(), meth_cap, d_mtot.data_ptr()),
        }
        ms = {k: [] for k in fns}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for all
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        assert int(d_n.cpu().numpy().view(np.uint64)[0]) == sel
        etot = [int(v) for v in d_etot.cpu().numpy().view(np.uint64)]
        mtot = [int(v) for v in d_mtot.cpu().numpy().view(np.uint64)]
        assert etot[0] <= enc_cap and etot[2] == sel and mtot[0] <= meth_cap
        res.update({k: stats(v) for k, v in ms.items()})
        res.update({"emitted_positions": emitted1 * reps, "selected_records": sel, "selected_per_thousand_emitted": round(1000.0 * len(idx) / max(emitted1, 1), 3),
                    "totals_of_one_block": want_tot, "variant_stream_bytes": etot[0], "meth_table_bytes": mtot[0]})
        med = lambda k: res[k]["ms_median"]
        res["select_pack_emit_over_meth_sites"] = round(med("select_pack_emit") / med("meth_sites"), 4)
        res["select_pack_emit_over_core"] = round(med("select_pack_emit") / med("select_pack_core"), 4)
    return res


def trace_part(d):
    """Median kernel times from the kernel trace(s) rocprofv3 left under d, the selection's kernels by call."""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
    if not rows:
        raise SystemExit("no kernel trace under " + d)
    rows.sort()
    short = lambda full: full.replace("void ", "").split("(")[0].replace(".kd", "").strip()
    out, cur, k_sel = {}, None, 0
    for _, full, ms in rows:
        name = short(full)
        if name == "bsc_var_select_kernel":  # the timed calls alternate: with the emit bytes, without
            cur = "select_pack_emit" if k_sel % 2 == 0 else "select_pack_core"
            k_sel += 1
        elif name.startswith("bsc_") and not name.startswith("bsc_var_"):
            cur = None
        if name.startswith("bsc_var_") or (cur and not name.startswith("bsc_")):
            key = name if name.startswith("bsc_") else "scan_kernels"
            out.setdefault(cur or "?", {}).setdefault(key, []).append(ms)
            if name == "bsc_var_pack_kernel":
                cur = None  # the scan lies between the two kernels: what follows the pack pass is another call's
        elif name in ("bsc_meth_size_kernel", "bsc_meth_write_kernel") or name.startswith("bsc_bcf_"):
            out.setdefault("other", {}).setdefault(name, []).append(ms)
    big = {}  # (the one-block check's dispatches are the small ones: keep those within a factor of four of the largest)
    for call, ks in out.items():
        for k, v in ks.items():
            top = max(v)
            big.setdefault(call, {})[k] = [t for t in v if t >= 0.25 * top]
    res = {call: {k: dict(stats(v), dispatches=len(v)) for k, v in ks.items()} for call, ks in big.items()}
    try:
        sel = res["select_pack_emit"]["bsc_var_select_kernel"]["ms_median"]
        size = res["other"]["bsc_meth_size_kernel"]["ms_median"]
        res["select_emit_over_meth_size"] = round(sel / size, 4)
        res["select_core_over_meth_size"] = round(res["select_pack_core"]["bsc_var_select_kernel"]["ms_median"] / size, 4)
    except KeyError:
        pass
    return res


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_variants")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    var = os.path.join(d, "out.var.bcf")
    modes = {"Ob": ["-O", "b"], "Ob_variants": ["-O", "b", "--variants", var], "Ob_index_variants": ["-O", "b", "--index", "--variants", var + ".2"]}
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([exe, *modes[mode], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"), timeout=600)
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
    res["Ob_variants"]["variant_bytes"] = os.path.getsize(var)
    res["main_file_unchanged"] = M.sha_file(os.path.join(d, "Ob.out")) == M.sha_file(os.path.join(d, "Ob_variants.out"))
    res["variant_file_same_with_index"] = M.sha_file(var) == M.sha_file(var + ".2")
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
    ap.add_argument("--trace-dir", default=None, help="read the kernel trace a traced run of this tool left there")
    ap.add_argument("--skip-device", action="store_true", help="with --trace-dir: only read the trace")
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
