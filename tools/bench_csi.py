#!/usr/bin/env python3
"""The CSI index made beside the compressed file (csrc/csidev.hip, bsc_csi_*): (1) the scan alone on a resident stream of the device
encoders at 30x — a 2 M-position block's BCF stream and the same block's VCF text, by tile offsets rebuilt the way the encoders leave them
(the first record at or behind every 64th position): ms per call (median of the repeats, with the spread), bytes read (the stream twice: a
counting and a writing pass), fraction of the HBM peak; (2) integration/bam2bcf -O b with and without --index, from the same binary,
alternating, file to file at 50 Mb / 30x (tools/make_wgbs_bam.c): median and spread of >= 5 runs each, and the .csi checked to open with
vcf.read_csi and to answer one window's query with records of that window only.
usage: python tools/bench_csi.py [out.json [positions [runs]]]     (files under $BENCH_TMP, default /tmp/bench_csi) -> profiles/csi_50Mb.json"""
import json
import os
import statistics
import struct
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bs_call_amd as B  # noqa: E402
from bs_call_amd import vcf  # noqa: E402
from bs_call_amd.caller import CSI_BCF, CSI_VCF  # noqa: E402

out_json = sys.argv[1] if len(sys.argv) > 1 else None
n_pos = int(sys.argv[2]) if len(sys.argv) > 2 else 50_000_000
n_runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
HBM_PEAK = 8.0e12
THREADS = min(16, len(os.sched_getaffinity(0)))
res = {"threads": THREADS, "min_shift": 14}


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def tile_offsets(pos0, starts, n_bytes):
    """pos0 / starts: every record's 0-based position and stream offset -> the first record at or behind every multiple of 64 positions,
    counted from the block's first position, and the stream's length: what tile_off of the encoders holds."""
    x = int(pos0[0]) // 64 * 64
    tiles = (int(pos0[-1]) - x) // 64 + 1
    k = np.searchsorted(pos0, x + 64 * np.arange(tiles), side="left")
    return np.concatenate([np.append(starts, n_bytes)[k], [n_bytes]]).astype(np.int64)


# (1) the scan alone
seed = 88172645463325252
tpl, seq = B.synth_reads_host(seed, 5_000, 2_000_000, 30)
x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
res["scan"] = {}
with B.SiteCaller() as c:
    ref = B.synth_ref_host(seed, x, y - x + 3)
    blob, n_rec = c.block_bcf(tpl, seq, x, y, ref, 0)
    recs = c.block_records(tpl, seq, x, y, ref)
    text = ("\n".join(vcf.format_records_c(recs, "chr1")) + "\n").encode()
    for name, fmt, s in (("bcf", CSI_BCF, bytes(blob)), ("vcf_text", CSI_VCF, text)):
        if fmt == CSI_BCF:
            starts, at = [], 0
            while at < len(s):
                starts.append(at)
                at += 8 + sum(struct.unpack_from("<II", s, at))
            starts = np.array(starts, np.int64)
        else:
            a = np.frombuffer(s, np.uint8)
            starts = np.concatenate([[0], np.flatnonzero(a == 10)[:-1] + 1]).astype(np.int64)
        pos0 = recs["core"]["pos"].astype(np.int64) - 1
        assert len(starts) == len(pos0)
        sync = torch.from_numpy(tile_offsets(pos0, starts, len(s))).to("cuda")
        d = torch.frombuffer(bytearray(s), dtype=torch.uint8).to("cuda")
        ent, n_ent, n_records, err = c.csi_scan_device(fmt, d.data_ptr(), len(s), sync.data_ptr(), len(sync) - 1, 14)
        assert err == 0 and n_records == len(pos0) and n_ent == len(ent)
        ms = []
        for _ in range(12):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.csi_scan_device(fmt, d.data_ptr(), len(s), sync.data_ptr(), len(sync) - 1, 14)  # (waits for the device itself)
            ms.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ms[2:])
        res["scan"][name] = {"stream_bytes": len(s), "records": int(n_records), "intervals": len(sync) - 1, "entries": int(n_ent), "ms_per_call_with_launch_and_wait": spread(ms[2:]),
                             "bytes_read": 2 * len(s), "fraction_of_hbm_peak": round(2 * len(s) / (med * 1e-3) / HBM_PEAK, 4)}
        print(name, res["scan"][name], flush=True)

# (2) bam2bcf -O b with and without --index
d = os.environ.get("BENCH_TMP", "/tmp/bench_csi")
os.makedirs(d, exist_ok=True)
gen = os.path.join(d, "make_wgbs_bam")
subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
t0 = time.time()
subprocess.check_output([gen, bam, fa, str(n_pos), "30", "88172645463325253", str(THREADS), "1", "0", "1", "0"])
res["bam2bcf"] = {"positions": n_pos, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
for fmt_opts, key in (([], "bcf"), (["--format", "vcf"], "vcf")):
    e = res["bam2bcf"][key] = {"plain": [], "index": []}
    for run in range(n_runs + 1):  # (the first pair warms the page cache and is left out)
        for mode in ("plain", "index"):
            ob, orp = os.path.join(d, "%s.%s.out" % (key, mode)), os.path.join(d, "%s.%s.json" % (key, mode))
            for f_ in (ob, orp, ob + ".csi"):
                if os.path.exists(f_):
                    os.remove(f_)
            r = subprocess.run([exe, "-O", "b"] + fmt_opts + (["--index"] if mode == "index" else []) + [bam, fa, ob, orp], capture_output=True, text=True,
                               env=dict(os.environ, BAM2BCF_TIMING="1"))
            if r.returncode != 0:
                print(r.stderr[-2000:])
                raise SystemExit(1)
            st = json.loads(r.stderr.strip().splitlines()[-1])
            if run:
                e[mode].append(st["wall_without_context_s"])
    e["same_data_file"] = open(os.path.join(d, key + ".plain.out"), "rb").read() == open(os.path.join(d, key + ".index.out"), "rb").read()
    ix = vcf.read_csi(os.path.join(d, key + ".index.out.csi"))
    got = vcf.fetch(os.path.join(d, key + ".index.out"), 0, 5 << 14, 6 << 14, index=ix)
    e["csi_bytes"] = os.path.getsize(os.path.join(d, key + ".index.out.csi"))
    e["records_of_window_5"] = len(got)
    e["wall_without_context_s"] = {m: spread(e[m]) for m in ("plain", "index")}
    e["index_minus_plain_median_s"] = round(statistics.median(e["index"]) - statistics.median(e["plain"]), 4)
    e["plain_spread_s"] = round(max(e["plain"]) - min(e["plain"]), 4)
    print(key, e["wall_without_context_s"], e["index_minus_plain_median_s"], e["plain_spread_s"], flush=True)
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as f:
        json.dump(res, f, indent=1)
