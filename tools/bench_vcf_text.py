#!/usr/bin/env python3
"""The device's VCF text encoder (csrc/vcftextdev.hip) beside its BCF encoder, and bam2bcf --format vcf file to file.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM: bsc_vcf_text_sites_device and bsc_bcf_sites_len_device — ms (HIP events, median of --repeats runs
    behind --warmup), bytes out, output GB/s (output bytes only: the reads of the arrays are not in it) and that as a fraction of the HBM peak.
    --parent-lib: a libbscall_amd.so built from the parent commit; the BCF encoder is then ALSO measured from that build, in a process of
    its own, for the comparison the text encoder's target is stated against.
(2) host: bsc_vcf_format_rec, one thread, on the records of that same block (one ctypes call per record: an upper bound of ctypes + snprintf).
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c, as tools/bench_bgzf.py makes it) through bam2bcf --format vcf -O u,
    --format vcf -O b and plain -O u (--parent-exe: the parent commit's bam2bcf for that one), two runs each: seconds without the context,
    bytes written; the -O b text is checked to inflate to the -O u text.
(4) --kernel-stats DIR: the per-kernel split — the *kernel_stats.csv that `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
    python tools/bench_vcf_text.py --device-only` left (a run of its own: the profiler's overhead is in that run's wall times, not in (1)).

    python tools/bench_vcf_text.py [--positions N] [--repeats 20] [--files] [--parent-lib SO] [--parent-exe EXE] [--kernel-stats DIR] [--out JSON]
"""
import argparse
import csv
import ctypes as C
import glob
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

HBM_PEAK_GBS = 8000.0  # MI355X
BLOCK = 2_000_000
SEED = 88172645463325252


def device_part(a, bcf_only=False):
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
        d_len1 = torch.zeros(n1, dtype=torch.uint8, device="cuda")
        c.reads_chain_len_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core1.data_ptr(), d_aux1.data_ptr(),
                                 d_len1.data_ptr())
        torch.cuda.synchronize()
        d_core, d_aux = d_core1.repeat(reps), d_aux1.repeat(reps)
        d_len = torch.cat([d_len1.repeat(reps), torch.zeros(64, dtype=torch.uint8, device="cuda")])
        del d_core1, d_aux1, d_len1
        cap = n * 100 + 4096
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(3, dtype=torch.int64, device="cuda")

        def text():
            c.vcf_text_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_out.data_ptr(), cap, d_tot.data_ptr())

        def bcf():
            c.bcf_sites_len_device(d_core.data_ptr(), d_aux.data_ptr(), d_len.data_ptr(), n, 0, d_out.data_ptr(), cap, d_tot.data_ptr())

        for name, fn in ((("bcf_sites_len", bcf),) if bcf_only else (("text_sites", text), ("bcf_sites_len", bcf))):
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
            res[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes_out": tot[0], "records": tot[2],
                         "out_GBs": round(tot[0] / med / 1e6, 1), "out_bytes_fraction_of_hbm_peak": round(tot[0] / med / 1e6 / HBM_PEAK_GBS, 4)}
        if bcf_only or a.device_only:
            return res
        # (2) the host formatter, one thread, on the records of the same block
        recs = c.block_records(tpl, seq, x, y, ref)
        buf, base, L = C.create_string_buffer(2048), recs.ctypes.data, c._L
        t0 = time.perf_counter()
        for i in range(len(recs)):
            L.bsc_vcf_format_rec(base + 128 * i, b"chr1", None, buf, 2048)
        dt = time.perf_counter() - t0
        assert len(recs) * reps == res["text_sites"]["records"]
        res["host_formatter"] = {"records": len(recs), "seconds": round(dt, 3), "records_per_s": round(len(recs) / dt),
                                 "what": "bsc_vcf_format_rec on the block's records, one thread, one ctypes call per record (ctypes + snprintf: an upper bound)"}
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
    d = os.environ.get("BENCH_TMP", "/tmp/bench_vcf_text")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    modes = {"vcf_Ou": (exe, ["--format", "vcf", "-O", "u"]), "vcf_Ob": (exe, ["--format", "vcf", "-O", "b"]),
             "bcf_Ou": (a.parent_exe or exe, ["-O", "u"])}
    res["bcf_Ou_built_from"] = "the parent commit" if a.parent_exe else "this tree"
    for mode in ("bcf_Ou", "vcf_Ou", "vcf_Ob") * 2:
        e_, args = modes[mode]
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([e_, *args, bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"))
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
        res[k]["best_wall_without_context_s"] = min(r_["wall_without_context_s"] for r_ in res[k]["runs"])
    res["vcf_Ob_inflates_to_vcf_Ou_bytes"] = sha_file(os.path.join(d, "vcf_Ob.out"), gz=True) == sha_file(os.path.join(d, "vcf_Ou.out"))
    res["same_counters_printed"] = len({res[k]["stdout"] for k in modes}) == 1
    for k in ("vcf_Ou", "vcf_Ob"):
        res[k + "_over_bcf_Ou"] = round(res[k]["best_wall_without_context_s"] / res["bcf_Ou"]["best_wall_without_context_s"], 3)
    return res


def kernel_stats(d):
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(p) as f:
            for row in csv.DictReader(f):
                nm = row["Name"]
                if "vtext" in nm or "bsc_bcf_" in nm:
                    short = nm.split("(")[0].replace("void ", "")[:80]
                    out[short] = {"calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 4), "min_ms": round(float(row["MinNs"]) / 1e6, 4),
                                  "max_ms": round(float(row["MaxNs"]) / 1e6, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=50_000_000)
    ap.add_argument("--file-positions", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--bcf-only", action="store_true", help="the BCF encoder alone (what --parent-lib runs in the parent's build)")
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": device_part(a, bcf_only=a.bcf_only)}
    print(json.dumps(res), flush=True)
    if a.bcf_only:
        return
    if a.parent_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bcf-only", "--positions", str(a.positions), "--repeats", str(a.repeats), "--warmup",
                            str(a.warmup)], capture_output=True, text=True, env=dict(os.environ, BSCALL_AMD_LIB=os.path.abspath(a.parent_lib)))
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        res["device"]["bcf_sites_len_parent_build"] = json.loads(r.stdout.strip().splitlines()[-1])["device"]["bcf_sites_len"]
    dv = res["device"]
    ref_bcf = dv.get("bcf_sites_len_parent_build", dv["bcf_sites_len"])
    dv["text_over_bcf_output_bytes_per_s"] = round(dv["text_sites"]["out_GBs"] / ref_bcf["out_GBs"], 3)
    if a.kernel_stats:
        res["kernels_under_rocprofv3"] = kernel_stats(a.kernel_stats)
    if a.files:
        res["bam2bcf"] = files_part(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
