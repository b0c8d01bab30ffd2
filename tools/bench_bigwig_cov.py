#!/usr/bin/env python3
"""The coverage bigWig track beside the level track (csrc/bwcovdev.hip: the write and reduce kernels over the track mask, behind the tile,
heads and windows kernels of csrc/bigwigdev.hip) on resident arrays, against the level track's own five kernels on the same arrays in the
same run, and bam2bcf with and without --cov-bigwig file to file.  tools/bench_bigwig.py's sibling.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM.  --repeats times each behind --warmup, in turn, by HIP events:
      level_entry    bsc_bigwig_sites_device: the level track's five kernels and two scans — the baseline
      mask1 / mask2 / mask3   bsc_bigwig_tracks_device with the level track, the coverage track, both
    then, on the two streams mask 3 left: bsc_zlib_pieces_device at stride 24 + 8 * 1024 of the level stream and of the coverage stream,
    in turn (the deflate of a block's sections), with the bytes in and out.
    The streams, the summaries and the totals of ONE copy of the block are checked against the host forms over the same arrays.
(2) per kernel (--trace-dir DIR): median kernel times per call from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format
    csv -d DIR` left — a run of its own.  The calls share three kernels by name, so the trace is cut at every tile kernel and a piece
    belongs to the call whose write kernel it holds.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O u without a track, with --meth-bigwig, with
    --cov-bigwig, with both; --runs runs each in turn: seconds without the context, best and worst.

    python tools/bench_bigwig_cov.py [--positions N] [--repeats 20] [--files] [--trace-dir DIR] [--out JSON]
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
from bs_call_amd import _lib, bigwig  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

CALL_OF_WRITE = {"bsc_bigwig_write_kernel": "level_entry", "bsc_bwcov_write_kernel<1u>": "mask1", "bsc_bwcov_write_kernel<2u>": "mask2",
                 "bsc_bwcov_write_kernel<3u>": "mask3"}


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
        d_core1, d_aux1 = z(n1 * 64), z(n1 * 64)
        c.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core1.data_ptr(), d_aux1.data_ptr())
        torch.cuda.synchronize()
        # one copy of the block: mask 3's result against the two host forms over the same arrays
        recs = np.concatenate([d_core1.cpu().numpy().reshape(-1, 64), d_aux1.cpu().numpy().reshape(-1, 64)], axis=1).reshape(-1).view(B.VCF_REC)
        want = {"level": bigwig.sections_recs_host(recs, 0), "coverage": bigwig.sections_recs_host(recs, 0, track="coverage")}
        sites1 = int(want["level"][1]["count"].sum())
        rooms1 = (24 * (sites1 // 1024 + 1) + 8 * sites1, len(want["level"][1]) + 1, len(want["level"][2]) + 1)
        bufs = {k: (z(rooms1[0]), z(40 * rooms1[1]), z(40 * rooms1[2])) for k in want}
        desc = lambda b, r: _lib.BwTrackOut(b[0].data_ptr(), r[0], b[1].data_ptr(), r[1], b[2].data_ptr(), r[2])
        d_tot = z(48)
        c.bigwig_tracks_device(d_core1.data_ptr(), d_aux1.data_ptr(), n1, x, 0, 3, desc(bufs["level"], rooms1), desc(bufs["coverage"], rooms1), d_tot.data_ptr())
        torch.cuda.synchronize()
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
        assert tot[:4] == [len(want["level"][0]), sites1, len(want["level"][1]), len(want["level"][2])], "the totals differ from the host form's"
        for k, b in bufs.items():
            assert b[0].cpu().numpy()[: tot[0]].tobytes() == want[k][0], "the %s stream differs from the host form's" % k
            assert b[1].cpu().numpy()[: 40 * tot[2]].tobytes() == want[k][1].tobytes() and b[2].cpu().numpy()[: 40 * tot[3]].tobytes() == want[k][2].tobytes(), k
        d_core, d_aux = d_core1.repeat(reps), d_aux1.repeat(reps)
        del d_core1, d_aux1, bufs
        sites = sites1 * reps
        rooms = (24 * (sites // 1024 + 1) + 8 * sites, sites // 1024 + 1, n // 1024 + 2)
        lv, cv = (z(rooms[0]), z(40 * rooms[1]), z(40 * rooms[2])), (z(rooms[0]), z(40 * rooms[1]), z(40 * rooms[2]))
        dl, dc = desc(lv, rooms), desc(cv, rooms)
        A = (d_core.data_ptr(), d_aux.data_ptr(), n, x, 0)
        fns = {
            "level_entry": lambda: c.bigwig_sites_device(*A, lv[0].data_ptr(), rooms[0], lv[1].data_ptr(), rooms[1], lv[2].data_ptr(), rooms[2], d_tot.data_ptr()),
            "mask1": lambda: c.bigwig_tracks_device(*A, 1, dl, None, d_tot.data_ptr()),
            "mask2": lambda: c.bigwig_tracks_device(*A, 2, None, dc, d_tot.data_ptr()),
            "mask3": lambda: c.bigwig_tracks_device(*A, 3, dl, dc, d_tot.data_ptr()),
        }
        ms = {k: [] for k in fns}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for all
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
        assert tot[1] == sites and tot[0] <= rooms[0] and tot[2] <= rooms[1] and tot[3] <= rooms[2]
        res.update({k: stats(v) for k, v in ms.items()})
        res.update({"sites": sites, "sections": tot[2], "windows": tot[3], "stream_bytes": tot[0]})
        med = lambda k: res[k]["ms_median"]
        res["mask3_over_mask1_plus_mask2"] = round(med("mask3") / (med("mask1") + med("mask2")), 4)
        res["mask3_over_level_entry"] = round(med("mask3") / med("level_entry"), 4)
        res["mask1_over_level_entry"] = round(med("mask1") / med("level_entry"), 4)
        # the deflate of the two streams mask 3 left, sections of 1024 sites
        piece, np_ = 24 + 8 * 1024, tot[2]
        d_z, d_zs, d_zt = z(tot[0] + 11 * np_), z(4 * np_), z(16)
        zf = {k: (lambda s=s: c.zlib_pieces_device(s.data_ptr(), tot[0], piece, d_z.data_ptr(), d_z.numel(), d_zs.data_ptr(), np_, d_zt.data_ptr()))
              for k, s in (("level", lv[0]), ("coverage", cv[0]))}
        zms, zbytes = {k: [] for k in zf}, {}
        for k, fn in zf.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            zbytes[k] = int(d_zt.cpu().numpy().view(np.uint64)[0])
        for _ in range(a.repeats):
            for k, fn in zf.items():
                zms[k].append(timed(fn))
        res["deflate"] = {k: dict(stats(zms[k]), bytes_in=tot[0], bytes_out=zbytes[k], ratio=round(zbytes[k] / tot[0], 4)) for k in zf}
    return res


def trace_part(d):
    """Median kernel time per call and kernel from the kernel trace(s) rocprofv3 left under d."""
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
    if not rows:
        raise SystemExit("no kernel trace under " + d)
    rows.sort()
    short = lambda full: full.replace("void ", "").split("(")[0].replace(".kd", "").strip()
    pieces, cur = [], None
    for _, full, ms in rows:
        name = short(full)
        if name == "bsc_bigwig_tile_kernel":
            cur = {}
            pieces.append(cur)
        elif "bsc_zlib" in name or "bsc_chain" in name:
            cur = None  # the deflate and the chain are no part of a call's piece
        if cur is None:
            continue
        key = name if name.startswith("bsc_") else "scan_kernels"
        cur[key] = cur.get(key, 0.0) + ms
    big = max(p["bsc_bigwig_tile_kernel"] for p in pieces)
    out = {}
    for p in pieces:
        call = next((CALL_OF_WRITE[k] for k in p if k in CALL_OF_WRITE), None)
        if call is None or p["bsc_bigwig_tile_kernel"] < 0.25 * big:  # (the one-block check's dispatches)
            continue
        for k, v in p.items():
            out.setdefault(call, {}).setdefault(k, []).append(v)
    return {call: dict({k: dict(stats(v), dispatches=len(v)) for k, v in ks.items()},
                       sum_of_medians_ms=round(sum(float(np.median(v)) for v in ks.values()), 4)) for call, ks in out.items()}


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_bigwig_cov")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    bw, cw = os.path.join(d, "out.bw"), os.path.join(d, "out.cov.bw")
    modes = {"Ou": ["-O", "u"], "Ou_bigwig": ["-O", "u", "--meth-bigwig", bw], "Ou_cov": ["-O", "u", "--cov-bigwig", cw],
             "Ou_bigwig_cov": ["-O", "u", "--meth-bigwig", bw + ".2", "--cov-bigwig", cw + ".2"]}
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
        e["stdout"] = r.stdout.strip()
        print(mode, e["runs"][-1], flush=True)
    for k in modes:
        walls = [r_["wall_without_context_s"] for r_ in res[k]["runs"]]
        res[k]["best_wall_without_context_s"], res[k]["worst_wall_without_context_s"] = min(walls), max(walls)
    res["Ou_cov"]["cov_bytes"] = os.path.getsize(cw)
    res["Ou_bigwig"]["bigwig_bytes"] = os.path.getsize(bw)
    f = bigwig.read(cw)
    res["Ou_cov"].update({"zoom_levels": f.header["zoomLevels"], "sections": f.section_count, "sites": f.summary["basesCovered"],
                          "mean_depth": round(f.summary["sumData"] / max(f.summary["basesCovered"], 1), 3)})
    res["tracks_of_one_call_equal_the_single_tracks"] = (M.sha_file(bw) == M.sha_file(bw + ".2") and M.sha_file(cw) == M.sha_file(cw + ".2"))
    res["main_file_unchanged"] = all(M.sha_file(os.path.join(d, "Ou.out")) == M.sha_file(os.path.join(d, k + ".out")) for k in modes)
    res["report_unchanged"] = all(open(os.path.join(d, "Ou.json")).read() == open(os.path.join(d, k + ".json")).read() for k in modes)
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
