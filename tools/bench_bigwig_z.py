#!/usr/bin/env python3
"""The device zlib encoder for the bigWig track's sections (csrc/zlibdev.hip) on a resident stream, beside the BGZF encoder on the same
bytes in the same process, and bam2bcf with and without --meth-bigwig-compress file to file.  tools/bench_bigwig.py's sibling.

(1) device: the bigWig stream bsc_bigwig_sites_device makes for a 2 M-position block at 30x, its whole sections repeated on the device to
    --positions (default 50 M) worth of sites, S = 1024.  --repeats times each behind --warmup, in turn, by HIP events:
      zlib           bsc_zlib_pieces_device at stride 8216: the deflate kernel, the scan, the gather
      bgzf           bsc_bgzf_write_device + bsc_bgzf_take of the same bytes (0xFF00-byte members): the yardstick for time
    The streams of ONE copy of the block are inflated by zlib and compared; the ratios are to zlib level 1 and level 6 per section on that copy.
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d DIR` left.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O u with --meth-bigwig, and with --meth-bigwig-compress
    beside it; --runs runs each in turn: seconds without the context, best and worst.
(4) --synthetic: no device — sections of the header's layout from synthetic sites (CpG pairs, geometric gaps of mean 16, Poisson-15 coverage,
    levels from the 1001-entry table) through zlib at level 1 (S = 256, 1024, 8157), level 6 and Z_HUFFMAN_ONLY: the ratios the issue set out from.

    python tools/bench_bigwig_z.py [--positions N] [--repeats 10] [--files] [--trace-dir DIR] [--synthetic] [--out JSON]
"""
import argparse
import importlib.util
import json
import os
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECE = 24 + 8 * 1024
KERNELS = ("bsc_zlib_deflate_small_kernel", "bsc_zlib_scan_kernel", "bsc_zlib_gather_kernel", "bsc_bgzf_deflate_kernel", "bsc_bgzf_scan_kernel",
           "bsc_bgzf_gather_kernel")


def synthetic_part():
    rng = np.random.default_rng(1)
    n = 200_000
    gaps = rng.geometric(1 / 16.0, n // 2) + 1
    first = np.cumsum(gaps)
    starts = np.stack([first, first + 1], axis=1).reshape(-1).astype(np.uint32)  # CpG pairs
    cov = np.maximum(rng.poisson(15, n), 1)
    level = np.repeat(rng.beta(5, 1.5, n // 2), 2)
    a = rng.binomial(cov, level)
    m = (2000 * a + cov) // (2 * cov)
    val = (np.arange(1001, dtype=np.float64) / 10.0).astype(np.float32)[m]
    items = np.zeros(n, dtype=[("s", "<u4"), ("v", "<f4")])
    items["s"], items["v"] = starts, val

    def sections(S):
        out = []
        for k in range(0, n, S):
            part = items[k : k + S]
            out.append(struct.pack("<IIIIIBBH", 0, int(part["s"][0]), int(part["s"][-1]) + 1, 0, 1, 2, 0, len(part)) + part.tobytes())
        return out

    def huff(b):
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        return co.compress(b) + co.flush()

    res = {}
    for S in (256, 1024, 8157):
        secs = sections(S)
        res["level1_S%d" % S] = round(sum(map(len, secs)) / sum(len(zlib.compress(s, 1)) for s in secs), 3)
    secs = sections(1024)
    raw = sum(map(len, secs))
    res["level6_S1024"] = round(raw / sum(len(zlib.compress(s, 6)) for s in secs), 3)
    res["huffman_only_S1024"] = round(raw / sum(len(huff(s)) for s in secs), 3)
    return res


def device_part(a):
    import torch

    import bs_call_amd as B

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

    tpl, seq = B.synth_reads_host(M.SEED, 5_000, M.BLOCK, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    n1 = y - x + 1
    ref = B.synth_ref_host(M.SEED, x, n1 + 2)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    res = {"block_positions": n1, "coverage": 30, "items_per_section": 1024, "repeats": a.repeats, "warmup": a.warmup}
    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_core, d_aux = z(n1 * 64), z(n1 * 64)
        c.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core.data_ptr(), d_aux.data_ptr())
        n_sec = n1 // 1024 + 1
        d_out, d_sec, d_zoom, d_tot = z(24 * n_sec + 8 * n1), z(40 * n_sec), z(40 * (n1 // 1024 + 2)), z(48)
        c.bigwig_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n1, x, 0, d_out.data_ptr(), d_out.numel(), d_sec.data_ptr(), n_sec, d_zoom.data_ptr(),
                              n1 // 1024 + 2, d_tot.data_ptr())
        torch.cuda.synchronize()
        nb, sites1 = (int(v) for v in d_tot.cpu().numpy().view(np.uint64)[:2])
        del d_core, d_aux, d_tpl, d_seq
        whole = nb // PIECE * PIECE  # the block's whole sections
        raw1 = d_out.cpu().numpy()[:whole].tobytes()
        reps = max(1, -(-a.positions // n1))
        d_src = d_out[:whole].repeat(reps)
        n = whole * reps
        n_p = n // PIECE
        res.update({"positions": n1 * reps, "copies_of_the_block": reps, "sites": (whole // PIECE) * 1024 * reps, "sections": n_p, "stream_bytes": n})
        d_z, d_zs, d_zt = z(n + 11 * n_p), z(4 * n_p), z(16)
        bg = c.bgzf()
        state = {}

        def run_bgzf():
            bg.write_device(d_src.data_ptr(), n)
            state["bgzf_bytes"] = len(bg.take())

        fns = {"zlib": lambda: c.zlib_pieces_device(d_src.data_ptr(), n, PIECE, d_z.data_ptr(), d_z.numel(), d_zs.data_ptr(), n_p, d_zt.data_ptr())}
        ms = {"zlib": [], "bgzf": []}
        for _ in range(a.warmup):
            fns["zlib"]()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            ms["zlib"].append(timed(fns["zlib"]))
        # the BGZF writer waits for its sizes and hands the members to the host: time its device work by the clock around the write alone
        for k in range(a.warmup + a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bg.write_device(d_src.data_ptr(), n)
            c.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            state["bgzf_bytes"] = len(bg.take())
            if k >= a.warmup:
                ms["bgzf"].append(dt)
        bg.close()
        zt = [int(v) for v in d_zt.cpu().numpy().view(np.uint64)[:2]]
        assert zt[1] == n_p and zt[0] <= d_z.numel()
        zs = d_zs.cpu().numpy().view(np.uint32)[:n_p]
        one = whole // PIECE
        blob, at = d_z.cpu().numpy()[: int(zs[:one].sum())].tobytes(), 0
        for k in range(one):  # one copy of the block, inflated
            assert zlib.decompress(blob[at : at + int(zs[k])]) == raw1[k * PIECE : (k + 1) * PIECE], "a stream does not inflate to its section"
            at += int(zs[k])
        lvl1 = sum(len(zlib.compress(raw1[k : k + PIECE], 1)) for k in range(0, whole, PIECE))
        lvl6 = sum(len(zlib.compress(raw1[k : k + PIECE], 6)) for k in range(0, whole, PIECE))
        res.update({k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()})
        res["bgzf"]["how"] = "host clock around bsc_bgzf_write_device + bsc_synchronize: its batches wait for their sizes on the host"
        res.update({"compressed_bytes": zt[0], "bgzf_bytes": state["bgzf_bytes"], "ratio": round(n / zt[0], 4),
                    "one_copy": {"raw": whole, "device": len(blob), "zlib_level_1": lvl1, "zlib_level_6": lvl6},
                    "device_over_level_1": round(len(blob) / lvl1, 4), "device_over_level_6": round(len(blob) / lvl6, 4),
                    "zlib_ns_per_input_byte": round(float(np.median(ms["zlib"])) * 1e6 / n, 5),
                    "bgzf_ns_per_input_byte": round(float(np.median(ms["bgzf"])) * 1e6 / n, 5)})
    return res


def files_part(a):
    from bs_call_amd import bigwig

    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_bigwig_z")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    modes = {"bigwig": ["-O", "u", "--meth-bigwig", os.path.join(d, "plain.bw")],
             "bigwig_compress": ["-O", "u", "--meth-bigwig", os.path.join(d, "z.bw"), "--meth-bigwig-compress"]}
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        r = subprocess.run([exe, *modes[mode], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"))
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        st = json.loads(r.stderr.strip().splitlines()[-1])
        res.setdefault(mode, {"runs": []})["runs"].append(st["wall_without_context_s"])
    for k in modes:
        res[k]["best_wall_without_context_s"], res[k]["worst_wall_without_context_s"] = min(res[k]["runs"]), max(res[k]["runs"])
    res["bigwig"]["bytes"], res["bigwig_compress"]["bytes"] = os.path.getsize(os.path.join(d, "plain.bw")), os.path.getsize(os.path.join(d, "z.bw"))
    fp, fz = bigwig.read(os.path.join(d, "plain.bw")), bigwig.read(os.path.join(d, "z.bw"))
    res["same_summary"] = fp.summary == fz.summary and fp.section_count == fz.section_count
    res["main_file_unchanged"] = open(os.path.join(d, "bigwig.out"), "rb").read() == open(os.path.join(d, "bigwig_compress.out"), "rb").read()
    lo, hi = (min(res["bigwig_compress"]["runs"]), max(res["bigwig_compress"]["runs"])), (min(res["bigwig"]["runs"]), max(res["bigwig"]["runs"]))
    res["difference"] = "unresolved: the ranges overlap" if lo[0] <= hi[1] and hi[0] <= lo[1] else "resolved: the ranges do not overlap"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=50_000_000)
    ap.add_argument("--file-positions", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--synthetic", action="store_true", help="the CPU experiment alone: zlib on synthetic sections, no device")
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"synthetic_zlib_ratios": synthetic_part()}
    print(json.dumps(res), flush=True)
    if not a.synthetic:
        res["device"] = device_part(a)
        print(json.dumps(res), flush=True)
        if a.trace_dir:
            spec = importlib.util.spec_from_file_location("bench_bigwig", os.path.join(ROOT, "tools", "bench_bigwig.py"))
            T = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(T)
            T.KERNELS = KERNELS  # its reader of a kernel trace, over this tool's kernels
            res["kernels"] = T.trace_part(a.trace_dir)
        if a.files:
            res["bam2bcf"] = files_part(a)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
