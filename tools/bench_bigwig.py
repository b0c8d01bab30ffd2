#!/usr/bin/env python3
"""The methylation bigWig track (csrc/bigwigdev.hip: tile, write, heads, windows and reduce kernels with two scans) on resident arrays,
beside the per-cytosine table's encoder on the same arrays in the same run, and bam2bcf with and without --meth-bigwig file to file.
tools/bench_meth_regions.py's sibling.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM.  --repeats times each behind --warmup, in turn, by HIP events:
      bigwig         bsc_bigwig_sites_device: the five kernels and the two scans (default parameters: 1024 sites a section, windows of 1024)
      table          bsc_meth_sites_device: bsc_meth_size_kernel + one scan + the write kernel — the yardstick (the same record bytes read)
      copy_probe     bsc_stream_probe_ms on 8 M positions: what the memory system of this box delivers, GB/s
    The stream, the summaries and the totals of ONE copy of the block are checked against the host form over the same arrays.
    Bytes: algorithmic = what the result needs read and written once (16 bytes of every position's record, 16 of a site's counts, the
    stream, the summaries); moved = the kernels' accesses as written (two passes over the records, the compact sites written once and read
    three times, the tile and window counts and their scans).
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d DIR`
    left — a run of its own.
(3) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O u without the switch, with --meth-bigwig, with
    --meth, and — --parent-exe — through the parent commit's bam2bcf without the switch; --runs runs each in turn: seconds without the
    context, best and worst.

    python tools/bench_bigwig.py [--positions N] [--repeats 20] [--files] [--parent-exe PATH] [--trace-dir DIR] [--out JSON]
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
from bs_call_amd import bigwig  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

KERNELS = ("bsc_bigwig_tile_kernel", "bsc_bigwig_write_kernel", "bsc_bigwig_heads_kernel", "bsc_bigwig_windows_kernel", "bsc_bigwig_reduce_kernel",
           "bsc_meth_size_kernel", "bsc_meth_write_kernel")


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
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    res = {"positions": n, "block_positions": n1, "copies_of_the_block": reps, "coverage": 30, "repeats": a.repeats, "warmup": a.warmup}
    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_core1, d_aux1 = z(n1 * 64), z(n1 * 64)
        c.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core1.data_ptr(), d_aux1.data_ptr())
        torch.cuda.synchronize()
        # one copy of the block: the device's result against the host form over the same arrays
        recs = np.concatenate([d_core1.cpu().numpy().reshape(-1, 64), d_aux1.cpu().numpy().reshape(-1, 64)], axis=1).reshape(-1).view(B.VCF_REC)
        want = bigwig.sections_recs_host(recs, 0)
        sites1 = int(want[1]["count"].sum())
        d_out, d_sec, d_zoom, d_tot = z(24 * (sites1 // 1024 + 1) + 8 * sites1), z(40 * (len(want[1]) + 1)), z(40 * (len(want[2]) + 1)), z(48)
        c.bigwig_sites_device(d_core1.data_ptr(), d_aux1.data_ptr(), n1, x, 0, d_out.data_ptr(), d_out.numel(), d_sec.data_ptr(), len(want[1]) + 1,
                              d_zoom.data_ptr(), len(want[2]) + 1, d_tot.data_ptr())
        torch.cuda.synchronize()
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
        assert tot[:4] == [len(want[0]), sites1, len(want[1]), len(want[2])], "the totals differ from the host form's"
        assert d_out.cpu().numpy()[: tot[0]].tobytes() == want[0], "the stream differs from the host form's"
        assert d_sec.cpu().numpy()[: 40 * tot[2]].tobytes() == want[1].tobytes() and d_zoom.cpu().numpy()[: 40 * tot[3]].tobytes() == want[2].tobytes()
        d_core, d_aux = d_core1.repeat(reps), d_aux1.repeat(reps)
        del d_core1, d_aux1, d_out, d_sec, d_zoom
        sites = sites1 * reps
        n_sec, n_win = sites // 1024 + 1, n // 1024 + 2
        d_out, d_sec, d_zoom = z(24 * n_sec + 8 * sites), z(40 * n_sec), z(40 * n_win)
        d_tab, d_ttot = z(sites * 100 + 4096), z(40)
        fns = {
            "bigwig": lambda: c.bigwig_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, x, 0, d_out.data_ptr(), d_out.numel(), d_sec.data_ptr(), n_sec,
                                                    d_zoom.data_ptr(), n_win, d_tot.data_ptr()),
            "table": lambda: c.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chr1", d_tab.data_ptr(), d_tab.numel(), d_ttot.data_ptr()),
        }
        ms = {k: [] for k in fns}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for both
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
        ttot = [int(v) for v in d_ttot.cpu().numpy().view(np.uint64)[:2]]
        assert tot[1] == sites == ttot[1] and tot[0] <= d_out.numel() and tot[2] <= n_sec and tot[3] <= n_win and ttot[0] <= d_tab.numel()
        n_tiles = (n + 63) // 64
        res.update({k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()})
        res.update({"sites": sites, "sections": tot[2], "windows": tot[3], "stream_bytes": tot[0], "table_bytes": ttot[0],
                    "stream_over_table": round(tot[0] / ttot[0], 4),
                    "algorithmic_bytes": 16 * n + 16 * sites + tot[0] + 40 * (tot[2] + tot[3]),
                    "moved_bytes": 2 * (16 * n + 16 * sites) + 8 * sites * 4 + tot[0] + 40 * (tot[2] + tot[3]) + 4 * tot[3] + 8 * 8 * n_tiles})
        res["bigwig_GB_per_s_on_moved_bytes"] = round(res["moved_bytes"] / res["bigwig"]["ms_median"] / 1e6, 1)
        del d_core, d_aux
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
            big = [t for t in v if t >= 0.25 * max(v)]  # the 50 M-position dispatches, not the one-block check's
            out[name] = {"dispatches": len(big), "ms_median": round(float(np.median(big)), 4), "ms_min": round(min(big), 4), "ms_max": round(max(big), 4)}
        elif "scan" in full.lower():
            out.setdefault("scan_kernels", {})[full[:80]] = {"dispatches": len(v), "ms_median": round(float(np.median(v)), 4)}
    return out


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_bigwig")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    modes = {"Ou": (exe, ["-O", "u"]), "Ou_bigwig": (exe, ["-O", "u", "--meth-bigwig", os.path.join(d, "out.bw")]),
             "Ou_meth": (exe, ["-O", "u", "--meth", os.path.join(d, "out.meth")])}
    if a.parent_exe:
        modes["parent_Ou"] = (a.parent_exe, ["-O", "u"])
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([modes[mode][0], *modes[mode][1], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"))
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
    res["Ou_bigwig"]["bigwig_bytes"] = os.path.getsize(os.path.join(d, "out.bw"))
    res["Ou_meth"]["table_bytes"] = os.path.getsize(os.path.join(d, "out.meth"))
    f = bigwig.read(os.path.join(d, "out.bw"))
    res["Ou_bigwig"].update({"zoom_levels": f.header["zoomLevels"], "sections": f.section_count, "sites": f.summary["basesCovered"]})
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
    ap.add_argument("--parent-exe", default=None, help="the parent commit's bam2bcf, run without the switch beside this one's")
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
