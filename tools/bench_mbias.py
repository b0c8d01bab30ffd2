#!/usr/bin/env python3
"""The M-bias table (csrc/mbiasdev.hip: one walk over the raw templates) on resident reads, against the two passes that read the same read
bytes — the read-profile pass of the pre-processing and HOT LOOP A (files this feature does not touch, so those kernels are the parent
commit's) — in the same run, and bam2bcf -O b with and without --mbias file to file.  tools/bench_cpg_reads.py's sibling.

(1) device: one block of --positions (default 50 M) at 30x, the device-resident reads of bench.py's roofline_reads (bs_call_amd.reads.
    synth_block) as RAW templates with empty mismatch lists, their read bytes and the reference codes in HBM.  --repeats times each behind
    --warmup, in turn, by HIP events:
      mbias           bsc_mbias_device into a zeroed table (n_cycles 512)
      prep            bsc_prepare_templates_device without a read profile
      prep_profile    the same with one: the read-profile pass is the difference
      accumulate      bsc_accumulate_device over the prepared templates: the pile-up's walk of the same read bytes
    The table and totals of a first part of the block are checked against the host form (csrc/mbias.c) over the same templates.
(2) file to file (--files): a 50 Mb / 30x BAM (tools/make_wgbs_bam.c) through bam2bcf -O b without and with --mbias and, with --parent-exe,
    through the parent commit's binary; --runs runs each in turn: seconds without the context, every run reported, best and worst.

    python tools/bench_mbias.py [--positions N] [--repeats 20] [--files [--parent-exe PATH]] [--out JSON]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bs_call_amd as B  # noqa: E402
from bs_call_amd import _lib, reads as R  # noqa: E402
from bs_call_amd.abi import MISMS, PREP_PARAMS, PREP_STATS, RAW_TEMPLATE  # noqa: E402
from bs_call_amd.caller import ReadProfile, mbias_host  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_meth", os.path.join(ROOT, "tools", "bench_meth.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

HBM_PEAK_GBPS = 8000.0  # bench.py's
N_CYCLES = 512


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def as_raw(tpl):
    """Prepared templates as the raw ones they came from: no list, the span the read's length."""
    raw = np.zeros(len(tpl), dtype=RAW_TEMPLATE)
    for f in ("pos", "len", "off", "mapq", "orientation", "bs_strand"):
        raw[f] = tpl[f]
    raw["reference_span"] = tpl["len"]
    return raw


def device_part(a):
    x = 1000
    tpl, seq, y = R.synth_block(M.SEED + 2, x, a.positions, 30, chunk=1_000_000)
    n = y - x + 1
    ref = B.synth_ref_host(M.SEED + 2, x, n + 2)
    raw = as_raw(tpl)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    res = {"positions": n, "coverage": 30, "templates": len(tpl), "read_bytes": int(seq.size), "repeats": a.repeats, "warmup": a.warmup, "n_cycles": N_CYCLES}
    cells = 12 * N_CYCLES * 2
    with B.SiteCaller() as c:
        L, h = c._L, c._h
        d_raw, d_tpl, d_seq, d_ref, d_ms = up(raw), up(tpl), up(seq), up(ref), z(16)
        d_counts, d_tot = torch.zeros(cells, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
        # a first part of the block: the device's table against the host form over the same templates
        m = min(n, 300_000)
        k = int(np.searchsorted(tpl["pos"][:, 0], x + m))  # (the templates come in the order of their start positions)
        want, w_tot = mbias_host(raw[:k], seq, np.zeros(0, MISMS), x, x + m - 1, ref[: m + 2], 20, N_CYCLES)
        c.mbias_device(d_raw.data_ptr(), k, d_seq.data_ptr(), seq.size, d_ms.data_ptr(), 0, x, x + m - 1, d_ref.data_ptr(), d_counts.data_ptr(), d_tot.data_ptr(),
                       params=N_CYCLES, stream=stream)
        torch.cuda.synchronize()
        assert d_counts.cpu().numpy().tobytes() == want.tobytes(), "the table differs from the host form's"
        assert tuple(int(v) for v in d_tot.cpu().numpy()) == tuple(int(v) for v in w_tot), "the totals differ from the host form's"
        res["checked_against_the_host_form"] = {"positions": m, "templates": k, "counted": int(w_tot[2])}
        d_pile = z((n + 63) // 64 * 64 * 104)
        d_ptpl, d_pseq = z(len(tpl) * 40), z(int(seq.size) + 16)
        par = np.zeros(1, dtype=PREP_PARAMS)
        par["min_qual"][0] = 20
        used, st = C.c_uint64(0), np.zeros(1, dtype=PREP_STATS)
        prof = ReadProfile()

        def prep(with_profile):
            pf = _lib.ReadProfile(d_ref.data_ptr(), x, n + 2, prof.counts.ctypes.data, prof.counts.shape[0], 0) if with_profile else None
            rc = L.bsc_prepare_templates_device(h, d_raw.data_ptr(), len(raw), d_seq.data_ptr(), seq.size, d_ms.data_ptr(), 0, par.ctypes.data, d_ptpl.data_ptr(),
                                                d_pseq.data_ptr(), int(seq.size) + 16, C.byref(used), st.ctypes.data, None if pf is None else C.byref(pf), stream)
            assert rc == 0, L.bsc_last_error()

        def run_mbias():
            d_counts.zero_()
            d_tot.zero_()
            c.mbias_device(d_raw.data_ptr(), len(raw), d_seq.data_ptr(), seq.size, d_ms.data_ptr(), 0, x, y, d_ref.data_ptr(), d_counts.data_ptr(), d_tot.data_ptr(),
                           params=N_CYCLES, stream=stream)

        fns = {
            "mbias": run_mbias,
            "prep": lambda: prep(False),
            "prep_profile": lambda: prep(True),
            "accumulate": lambda: c.accumulate_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_pile.data_ptr(), stream),
        }
        ms = {k_: [] for k_ in fns}
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # in turn: what drifts between two repeats drifts for all
            for k_, fn in fns.items():
                ms[k_].append(timed(fn))
        c.block_status(stream)  # (raises where the accumulate stage refused a template)
        tot = [int(v) for v in d_tot.cpu().numpy()]
        res.update({k_: stats(v) for k_, v in ms.items()})
        bytes_in = int(seq.size) + 72 * len(raw) + n + 2  # every read byte, raw template and reference code once
        med = lambda k_: res[k_]["ms_median"]
        res.update({"totals": tot, "input_bytes": bytes_in, "mbias_input_GBps": round(bytes_in / med("mbias") / 1e6, 1),
                    "mbias_fraction_of_hbm_peak": round(bytes_in / med("mbias") / 1e6 / HBM_PEAK_GBPS, 4),
                    "read_profile_pass_ms": round(med("prep_profile") - med("prep"), 4),
                    "mbias_over_accumulate": round(med("mbias") / med("accumulate"), 4)})
    return res


def files_part(a):
    threads = min(16, len(os.sched_getaffinity(0)))
    d = os.environ.get("BENCH_TMP", "/tmp/bench_mbias")
    os.makedirs(d, exist_ok=True)
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.file_positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.file_positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    tsv = os.path.join(d, "out.mbias.tsv")
    modes = {"Ob": [exe, "-O", "b"], "Ob_mbias": [exe, "-O", "b", "--mbias", tsv]}
    if a.parent_exe:
        modes["Ob_parent"] = [a.parent_exe, "-O", "b"]
    for mode in tuple(modes) * a.runs:
        ob, orp = os.path.join(d, mode + ".out"), os.path.join(d, mode + ".json")
        for f_ in (ob, orp):
            if os.path.exists(f_):
                os.remove(f_)
        t0 = time.time()
        r = subprocess.run([*modes[mode], bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"), timeout=600)
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
    res["Ob_mbias"]["table_bytes"] = os.path.getsize(tsv)
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
    ap.add_argument("--parent-exe", default=None, help="with --files: the parent commit's bam2bcf, run in turn with this tree's")
    ap.add_argument("--skip-device", action="store_true", help="with --files: leave the device part out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"date": time.strftime("%Y-%m-%d"), "machine": torch.cuda.get_device_name(0) if torch.cuda.is_available() else platform.node()}
    if not a.skip_device:
        res["device"] = device_part(a)
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
