#!/usr/bin/env python3
"""The device's methylation-table encoder (csrc/methdev.hip) beside its VCF text encoder, and bam2bcf --meth file to file.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM: bsc_meth_sites_device with BSC_METH_CPG and with BSC_METH_ALL (its size pass, the scan and its write
    pass: one call), and bsc_vcf_text_sites_device on the same arrays as the yardstick — ms (HIP events, median of --repeats runs behind
    --warmup), lines, bytes out, output GB/s (output bytes only: the reads of the arrays are not in it).
(2) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c, as tools/bench_vcf_text.py makes it) through the SAME bam2bcf with and
    without --meth, -O u and -O b, --runs runs each in turn: seconds without the context, bytes written; the main file of a --meth run is
    checked to be the file of the run without it, the -O b table to inflate to the -O u table.

    python tools/bench_meth.py [--positions N] [--repeats 20] [--files] [--out JSON]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bs_call_amd as B  # noqa: E402

BLOCK = 2_000_000
SEED = 88172645463325252


def device_part(a):
    tpl, seq = B.synth_reads_host(SEED, 5_000, BLOCK, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    n1 = y - x + 1
    ref = B.synth_ref_host(SEED, x, n1 + 2)
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
        cap = n * 100 + 4096
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")

        def meth(contexts):
            c.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_out.data_ptr(), cap, d_tot.data_ptr(), params={"contexts": contexts})

        def text():
            c.vcf_text_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_out.data_ptr(), cap, d_tot.data_ptr())

        for name, fn in (("meth_sites_cpg", lambda: meth(0)), ("meth_sites_all", lambda: meth(1)), ("text_sites", text)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            tot = [int(v) for v in d_tot.cpu()]
            assert tot[0] <= cap, "the stream did not fit"
            med = float(np.median(ms))
            res[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes_out": tot[0],
                         "lines": tot[2] if name == "text_sites" else tot[1], "out_GBs": round(tot[0] / med / 1e6, 1)}
        for k in ("meth_sites_cpg", "meth_sites_all"):
            res[k + "_over_text_ms"] = round(res[k]["ms_median"] / res["text_sites"]["ms_median"], 3)
    return res


def sha_file(p, gz=False):
    h = hashlib.sha256()
    dec = zlib.decompressobj(31) if gz else None
    with open(p, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            while dec is not None and chunk:
                h.update(dec.decompress(chunk))
                chunk = dec.unused_data
                if chunk:
                    dec = zlib.decompressobj(31)
            if dec is None:
                h.update(chunk)
    return h.hexdigest()


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_meth")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    modes = {"Ou": ["-O", "u"], "Ou_meth": ["-O", "u", "--meth", os.path.join(d, "Ou.bed")], "Ob": ["-O", "b"],
             "Ob_meth": ["-O", "b", "--meth", os.path.join(d, "Ob.bed.gz")]}
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
                          "encode_write_s": st["encode_write_s"], "waiting_for_inflate_s": st["device_reader"]["waiting_for_inflate_s"],
                          "pwrite_s": st["output_thread"]["pwrite_s"]})
        e["bytes"] = os.path.getsize(ob)
        e["stdout"] = r.stdout.strip()
        print(mode, e["runs"][-1], flush=True)
    for k in modes:
        walls = [r_["wall_without_context_s"] for r_ in res[k]["runs"]]
        res[k]["best_wall_without_context_s"], res[k]["worst_wall_without_context_s"] = min(walls), max(walls)
    res["Ou_meth"]["table_bytes"] = os.path.getsize(os.path.join(d, "Ou.bed"))
    res["Ob_meth"]["table_bytes"] = os.path.getsize(os.path.join(d, "Ob.bed.gz"))
    res["main_file_unchanged_by_meth"] = all(sha_file(os.path.join(d, k + ".out")) == sha_file(os.path.join(d, k + "_meth.out")) for k in ("Ou", "Ob"))
    res["report_unchanged_by_meth"] = all(open(os.path.join(d, k + ".json")).read() == open(os.path.join(d, k + "_meth.json")).read() for k in ("Ou", "Ob"))
    res["Ob_table_inflates_to_Ou_table"] = sha_file(os.path.join(d, "Ob.bed.gz"), gz=True) == sha_file(os.path.join(d, "Ou.bed"))
    for k in ("Ou", "Ob"):
        res[k + "_meth_over_plain"] = round(res[k + "_meth"]["best_wall_without_context_s"] / res[k]["best_wall_without_context_s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=50_000_000)
    ap.add_argument("--file-positions", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": device_part(a)}
    print(json.dumps(res), flush=True)
    if a.files:
        res["bam2bcf"] = files_part(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
