#!/usr/bin/env python3
"""The per-region methylation summary (csrc/methregionsdev.hip: bsc_meth_regions_tile_kernel, the four scans, bsc_meth_regions_region_kernel)
on resident arrays, beside the per-cytosine encoder's size pass on the same arrays, and bam2bcf with and without --meth-regions file to
file.  tools/bench_meth_cpg.py's sibling.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM.  Two region sets over them: windows of 1 kb (50 000 at 50 M positions) and 100 000 random
    intervals of 200 .. 5 000 bases.  Per set, --repeats times each behind --warmup, in turn, by HIP events:
      call           bsc_meth_regions_sites_device: tile pass + four scans + region pass
      tile_and_scan  the same launcher with an empty candidate range: tile pass + four scans
      scan           the four scans alone (bsc_dev_scan_u64 over the planes)
    so that tile pass = tile_and_scan - scan and region pass = call - tile_and_scan; and
      size_pass      the per-cytosine encoder's launcher with no room to write into: bsc_meth_size_kernel + one scan + a write pass that
                     skips every tile — the yardstick of the tile pass (the same record bytes read)
      copy_probe     bsc_stream_probe_ms on 8 M positions: what the memory system of this box delivers, GB/s
    The accumulators of each set are checked against a numpy prefix-sum form over the encoder's own table of the block.
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d DIR`
    left — a run of its own.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through the SAME bam2bcf -O u without the switch, with --meth-window
    1000 and with --meth-regions of the random intervals, --runs runs each in turn: seconds without the context, best and worst.

    python tools/bench_meth_regions.py [--positions N] [--repeats 20] [--files] [--trace-dir DIR] [--out JSON]
"""
import argparse
import csv
import ctypes as C
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
from bs_call_amd import _lib, methbed  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

KERNELS = ("bsc_meth_regions_tile_kernel", "bsc_meth_regions_region_kernel", "bsc_meth_size_kernel")


def region_sets(n, x0, seed=7):
    rng = np.random.default_rng(seed)
    top = x0 - 1 + n
    win = methbed.window_regions(top, 1000)
    starts = np.sort(rng.integers(0, max(top - 5000, 1), 100_000))
    rnd = np.zeros(len(starts), dtype=methbed.REGION)
    rnd["start"], rnd["end"] = starts, np.minimum(starts + rng.integers(200, 5001, len(starts)), top)
    rnd = rnd[np.lexsort((rnd["end"], rnd["start"]))]
    return {"windows_1kb": win, "random_200_5000": rnd}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def device_part(a):
    tpl, seq = B.synth_reads_host(M.SEED, 5_000, M.BLOCK, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    n1 = y - x + 1
    ref = B.synth_ref_host(M.SEED, x, n1 + 2)
    reps = max(1, -(-a.positions // n1))
    n = n1 * reps
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    res = {"positions": n, "block_positions": n1, "copies_of_the_block": reps, "coverage": 30, "repeats": a.repeats, "warmup": a.warmup}
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    with B.SiteCaller() as c:
        L = c._L
        L.bsc_dev_launch_meth_regions.restype = C.c_int
        L.bsc_dev_launch_meth_regions.argtypes = [vp, vp, vp, u64, u32, C.POINTER(_lib.MethParams), vp, vp, vp, C.c_size_t, vp, u32, u32, vp, C.c_int, vp]
        L.bsc_dev_launch_meth.restype = C.c_int
        L.bsc_dev_launch_meth.argtypes = [vp, vp, vp, vp, u64, vp, C.c_char_p, u32, C.POINTER(_lib.MethParams), vp, vp, vp, vp, C.c_size_t, vp, u64, vp, C.c_int, C.c_int, vp]
        L.bsc_dev_scan_tmp_bytes_u64.restype = C.c_int
        L.bsc_dev_scan_tmp_bytes_u64.argtypes = [u32, C.POINTER(C.c_size_t)]
        L.bsc_dev_scan_u64.restype = C.c_int
        L.bsc_dev_scan_u64.argtypes = [vp, vp, u32, vp, C.c_size_t, vp]
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_core1 = torch.zeros(n1 * 64, dtype=torch.uint8, device="cuda")
        d_aux1 = torch.zeros(n1 * 64, dtype=torch.uint8, device="cuda")
        c.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core1.data_ptr(), d_aux1.data_ptr())
        torch.cuda.synchronize()
        # the block's own table, for the check: its sites, repeated like the arrays (entry i of the long arrays is position x + i)
        d_out1 = torch.zeros(n1 * 16 + 4096, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(5, dtype=torch.int64, device="cuda")
        c.meth_sites_device(d_core1.data_ptr(), d_aux1.data_ptr(), n1, b"c", d_out1.data_ptr(), d_out1.numel(), d_tot.data_ptr())
        torch.cuda.synchronize()
        rows = methbed.parse_bed(d_out1[: int(d_tot[0])].cpu().numpy().tobytes())
        d_core, d_aux = d_core1.repeat(reps), d_aux1.repeat(reps)
        del d_core1, d_aux1, d_out1
        idx1 = (rows["start"].astype(np.int64) + 1 - x)
        idx = (idx1[None, :] + (np.arange(reps, dtype=np.int64) * n1)[:, None]).reshape(-1)
        cov = (rows["a"] + rows["b"]).astype(np.uint64)
        vals1 = np.stack([np.ones(len(rows), np.uint64), rows["a"].astype(np.uint64), rows["b"].astype(np.uint64),
                          (200 * rows["a"].astype(np.uint64) + cov) // (2 * cov)], axis=1)
        cum = np.zeros((n + 1, 4), dtype=np.uint64)
        cum[idx + 1] = np.tile(vals1, (reps, 1))  # (a position has one record: no index twice)
        cum = np.cumsum(cum, axis=0)
        n_tiles = (n + 63) // 64
        scan = C.c_size_t(0)
        assert L.bsc_dev_scan_tmp_bytes_u64(n_tiles + 1, C.byref(scan)) == 0
        z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
        d_pl, d_sc, d_tmp = z(32 * (n_tiles + 1)), z(32 * (n_tiles + 1)), z(scan.value)
        d_mtb, d_mto, d_mll = z(8 * (n_tiles + 1)), z(8 * (n_tiles + 1)), z(128 * (n_tiles + 1))
        mp = _lib.MethParams()
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        stride = 8 * (n_tiles + 1)

        def scans():
            for k in range(4):
                assert L.bsc_dev_scan_u64(d_pl.data_ptr() + k * stride, d_sc.data_ptr() + k * stride, n_tiles + 1, d_tmp.data_ptr(), scan.value, None) == 0

        fns = {
            "tile_and_scan": lambda: L.bsc_dev_launch_meth_regions(d_core.data_ptr(), d_aux.data_ptr(), None, n, x, C.byref(mp), d_pl.data_ptr(), d_sc.data_ptr(),
                                                                   d_tmp.data_ptr(), scan.value, None, 0, 0, None, cus, None),
            "scan": scans,
            "size_pass": lambda: L.bsc_dev_launch_meth(None, d_core.data_ptr(), d_aux.data_ptr(), None, n, None, b"chr1", 4, C.byref(mp), d_mtb.data_ptr(),
                                                       d_mto.data_ptr(), d_mll.data_ptr(), d_tmp.data_ptr(), scan.value, None, 0, d_tot.data_ptr(), 0, cus, None),
        }
        for name, regs in region_sets(n, x).items():
            c.meth_regions_attach(regs)
            call = lambda: c.meth_regions_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, x)
            ms = {k: [] for k in ("call", *fns)}
            for _ in range(a.warmup):
                call()
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for all
                ms["call"].append(timed(call))
                for k, fn in fns.items():
                    ms[k].append(timed(fn))
            c.meth_regions_reset()
            call()
            torch.cuda.synchronize()
            acc = c.meth_regions_read()
            lo = np.clip(regs["start"].astype(np.int64) + 1 - x, 0, n)
            hi = np.clip(regs["end"].astype(np.int64) + 1 - x, 0, n)
            want = cum[np.maximum(hi, lo)] - cum[lo]
            assert (acc == want).all(), "the accumulators differ from the table's prefix sums"
            e = {k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()}
            med = lambda k: e[k]["ms_median"]
            e.update({"regions": int(len(regs)), "regions_with_sites": int((acc[:, 0] > 0).sum()), "sites_summed": int(acc[:, 0].sum()),
                      "tile_pass_ms": round(med("tile_and_scan") - med("scan"), 4), "region_pass_ms": round(med("call") - med("tile_and_scan"), 4),
                      "size_pass_minus_one_scan_ms": round(med("size_pass") - med("scan") / 4, 4)})
            res[name] = e
        c.meth_regions_attach([])
        del d_core, d_aux
        # the copy probe: the calling kernel's traffic (104 + 1 bytes in, 200 + 1 out per position) by a kernel that does nothing else
        pn = 8_000_000
        d_cts, d_r, d_o, d_s = z(pn * 104), z(pn + 64), z(pn * 200), z(pn + 64)
        pms = c.stream_probe_ms(d_cts.data_ptr(), d_r.data_ptr(), pn, d_o.data_ptr(), d_s.data_ptr(), 5)
        res["copy_probe"] = {"positions": pn, "ms": round(pms, 4), "GB_per_s": round(pn * 306 / pms / 1e6, 1) if pms > 0 else None}
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


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_meth_regions")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    with open(fa) as f:
        contig = f.readline()[1:].split()[0]
    bed = os.path.join(d, "random.bed")
    rnd = region_sets(a.file_positions, 1)["random_200_5000"]
    with open(bed, "w") as f:
        for k, r in enumerate(rnd):
            f.write("%s\t%d\t%d\tr%d\n" % (contig, r["start"], r["end"], k))
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    modes = {"Ou": ["-O", "u"], "Ou_window_1kb": ["-O", "u", "--meth-window", "1000", "--meth-regions-out", os.path.join(d, "win.tsv")],
             "Ou_regions_random": ["-O", "u", "--meth-regions", bed, "--meth-regions-out", os.path.join(d, "rnd.tsv")]}
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
    res["Ou_window_1kb"]["summary_bytes"] = os.path.getsize(os.path.join(d, "win.tsv"))
    res["Ou_regions_random"]["summary_bytes"] = os.path.getsize(os.path.join(d, "rnd.tsv"))
    res["main_file_unchanged"] = all(M.sha_file(os.path.join(d, "Ou.out")) == M.sha_file(os.path.join(d, k + ".out")) for k in ("Ou_window_1kb", "Ou_regions_random"))
    res["report_unchanged"] = all(open(os.path.join(d, "Ou.json")).read() == open(os.path.join(d, k + ".json")).read() for k in ("Ou_window_1kb", "Ou_regions_random"))
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
