#!/usr/bin/env python3
"""What a dbSNP index costs per block on the host path and with the contig kept on the device (bsc_dbsnp_attach, csrc/dbsnpdev.hip), in one
process on one box, and bam2bcf -D file to file.  Writes profiles/dbsnp_dev.json.

Input: tools/make_dbsnp_index.py's synthetic index of one contig (chrS), --positions long (default 20 M) at one site per --spacing bp
(default 5: about today's dbSNP on human chromosomes), walked in blocks of --block positions (default 5 M).
  (a) host, per block — today's pipeline.run(dbsnp=...): bsc_dbsnp_flags, bsc_dbsnp_names' size pass and its fill pass, one thread, and
      the uploads of both results (pageable memory -> HBM on the NULL stream, waited for)
  (b) attach, once per contig: bsc_dbsnp_load_contig, then bsc_dbsnp_attach (the flattening + one upload)
  (c) device, per block: the flags kernel and the names kernel (HIP events, median of --repeats behind --warmup), the bytes each moves
      (counted from the flat layout: bins and entries read, bytes written) and that as a fraction of the HBM peak; the outputs are compared
      with (a)'s, byte for byte
  (d) --files: a 30x BAM of the same contig (tools/make_wgbs_bam.c) through bam2bcf without -D, bam2bcf -D, and
      pipeline.run(dbsnp=..., device_reader=True) with dbsnp_device False and True: seconds (bam2bcf: without the context), and that the
      -D stream equals the pipeline's

    python tools/bench_dbsnp_dev.py [--positions N] [--spacing 5] [--block N] [--repeats 20] [--files] [--out profiles/dbsnp_dev.json]
"""
import argparse
import ctypes as C
import hashlib
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
from bs_call_amd import dbsnp as D  # noqa: E402
from bs_call_amd import pipeline  # noqa: E402
from bs_call_amd.dbsnp import DbSnpIndex  # noqa: E402

spec = importlib.util.spec_from_file_location("make_dbsnp_index", os.path.join(ROOT, "tools", "make_dbsnp_index.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
HBM_PEAK_GBS = 8000.0  # MI355X


def med(v):
    return round(float(np.median(v)), 4)


def index_part(a, idx):
    res = {"positions": a.positions, "spacing": a.spacing, "block": a.block}
    blocks = [(x, min(a.block, a.positions - x + 1)) for x in range(1, a.positions + 1, a.block)]
    with DbSnpIndex(idx) as db, B.SiteCaller() as c:
        t0 = time.perf_counter()
        n_snps = db.load_contig("chrS")
        t_load = time.perf_counter() - t0
        t0 = time.perf_counter()
        assert c.dbsnp_attach(db) == n_snps
        t_attach = time.perf_counter() - t0
        res["sites"] = n_snps
        res["attach_once_per_contig"] = {"bsc_dbsnp_load_contig_s": round(t_load, 4), "bsc_dbsnp_attach_s": round(t_attach, 4),
                                         "what": "attach = the flattening on one thread + hipMalloc + one upload, waited for"}
        L = db._L
        host, dev = [], []
        for x, n in blocks:
            # (a) the host path of pipeline.run(dbsnp=...)
            t0 = time.perf_counter()
            flags = db.flags(x, n)
            t1 = time.perf_counter()
            ck, cnb = C.c_uint32(0), C.c_uint64(0)
            assert L.bsc_dbsnp_names(db._h, x, n, None, None, None, 0, 0, C.byref(ck), C.byref(cnb)) == 0
            t2 = time.perf_counter()
            k, nb = [ck.value], [cnb.value]
            pos, off, by = np.zeros(k[0], np.uint32), np.zeros(k[0] + 1, np.uint32), np.zeros(nb[0] + 1, np.uint8)
            assert L.bsc_dbsnp_names(db._h, x, n, pos.ctypes.data, off.ctypes.data, by.ctypes.data, k[0], nb[0], C.byref(ck), C.byref(cnb)) == 0
            t3 = time.perf_counter()
            up = [torch.from_numpy(v).to("cuda") for v in (flags, pos.view(np.int32), off.view(np.int32), by)]
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            host.append({"x": x, "n": n, "names": int(k[0]), "name_bytes": int(nb[0]), "flags_s": round(t1 - t0, 4), "names_size_pass_s": round(t2 - t1, 4),
                         "names_fill_pass_s": round(t3 - t2, 4), "uploads_s": round(t4 - t3, 4), "total_s": round(t4 - t0, 4)})
            # (c) the kernels
            kk, nbb = c.dbsnp_count(x, n)
            assert (kk, nbb) == (int(k[0]), int(nb[0]))
            d_fl = torch.empty(n, dtype=torch.uint8, device="cuda")
            d_pos, d_off, d_by = torch.empty(max(kk, 1), dtype=torch.int32, device="cuda"), torch.empty(kk + 1, dtype=torch.int32, device="cuda"), torch.empty(max(nbb, 1), dtype=torch.uint8, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            fns = {"flags": lambda: c.dbsnp_flags_device(x, n, d_fl.data_ptr(), s),
                   "names": lambda: c.dbsnp_names_device(x, n, d_pos.data_ptr(), d_off.data_ptr(), d_by.data_ptr(), kk, nbb, s)}
            ms = {}
            for name, fn in fns.items():
                for _ in range(a.warmup):
                    fn()
                torch.cuda.synchronize()
                ms[name] = []
                for _ in range(a.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
            same = torch.equal(d_fl, up[0]) and torch.equal(d_pos[:kk], up[1]) and torch.equal(d_off, up[2]) and torch.equal(d_by[:nbb], up[3][:nbb])
            assert same, "the device's flags / names differ from the host reader's"
            # bytes: flags — 16 bytes of masks per bin read, a byte per position written; names — per entry the entry word (2), its pool offset (4),
            # its text offset (4), its digit bytes (about name bytes / 2), its bin's mask and first-entry word (12, shared by the bin's entries, and the
            # binary search's probes, which stay in cache: not counted) read; pos (4), off (4) and the name bytes written
            b_flags = n + (n // 64 + 2) * 16
            b_names = kk * (2 + 4 + 4 + 4 + 4) + nbb + nbb // 2 + (n // 64 + 2) * 12
            dev.append({"x": x, "n": n, "flags_ms": med(ms["flags"]), "names_ms": med(ms["names"]), "flags_bytes": b_flags, "names_bytes": b_names,
                        "flags_fraction_of_hbm_peak": round(b_flags / med(ms["flags"]) / 1e6 / HBM_PEAK_GBS, 4),
                        "names_fraction_of_hbm_peak": round(b_names / med(ms["names"]) / 1e6 / HBM_PEAK_GBS, 4), "equal_to_the_host_reader": True})
            del up, d_fl, d_pos, d_off, d_by
        res["host_per_block"] = host
        res["device_per_block"] = dev
        res["host_total_s"] = round(sum(h["total_s"] for h in host), 4)
        res["device_total_ms"] = round(sum(d["flags_ms"] + d["names_ms"] for d in dev), 4)
        c.dbsnp_detach()
    return res


def sha(p):
    h = hashlib.sha256()
    with open(p, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def files_part(a, idx, d):
    from bs_call_amd.bam import fasta_contig

    threads = min(16, len(os.sched_getaffinity(0)))
    gen = os.path.join(d, "make_wgbs_bam")
    subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
    bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
    t0 = time.time()
    subprocess.check_output([gen, bam, fa, str(a.positions), "30", "88172645463325253", str(threads), "1", "0", "1", "0"])
    res = {"positions": a.positions, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    for mode, args in (("bam2bcf", []), ("bam2bcf_D", ["-D", idx])) * 2:
        ob, orp = os.path.join(d, mode + ".bcf"), os.path.join(d, mode + ".json")
        t0 = time.time()
        r = subprocess.run([exe, *args, bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"))
        dt = time.time() - t0
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(1)
        st = json.loads(r.stderr.strip().splitlines()[-1])
        e = res.setdefault(mode, {"runs": []})
        e["runs"].append({"process_wall_s": round(dt, 3), "wall_without_context_s": st["wall_without_context_s"], "reference_s": st["reference_s"],
                          "block_call_s": st["block_call_s"], "encode_write_s": st["encode_write_s"]})
        e["bytes"], e["stdout"] = os.path.getsize(ob), r.stdout.strip()
        print(mode, e["runs"][-1], flush=True)
    for k in ("bam2bcf", "bam2bcf_D"):
        res[k]["best_wall_without_context_s"] = min(r_["wall_without_context_s"] for r_ in res[k]["runs"])
    res["D_over_plain"] = round(res["bam2bcf_D"]["best_wall_without_context_s"] / res["bam2bcf"]["best_wall_without_context_s"], 3)
    codes = {"chrS": fasta_contig(fa, "chrS")}
    with DbSnpIndex(idx) as db:
        for what, on in (("pipeline_dbsnp_host", False), ("pipeline_dbsnp_device", True)):
            ob = os.path.join(d, what + ".bcf")
            t0 = time.time()
            pipeline.run(bam, codes, ob, date=(1, 1, 2000), compressed=False, benchmark_mode=True, device_reader=True, dbsnp=db, dbsnp_device=on)
            res[what] = {"wall_s": round(time.time() - t0, 3), "what": "pipeline.run(dbsnp=db, device_reader=True, dbsnp_device=%s), context creation included" % on}
            print(what, res[what], flush=True)
    res["bam2bcf_D_equals_the_pipeline_s_bytes"] = sha(os.path.join(d, "bam2bcf_D.bcf")) == sha(os.path.join(d, "pipeline_dbsnp_host.bcf")) == sha(os.path.join(d, "pipeline_dbsnp_device.bcf"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=20_000_000)
    ap.add_argument("--spacing", type=int, default=5)
    ap.add_argument("--block", type=int, default=5_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--files", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbsnp_dev.json"))
    a = ap.parse_args()
    d = os.environ.get("BENCH_TMP", "/tmp/bench_dbsnp_dev")
    os.makedirs(d, exist_ok=True)
    idx = os.path.join(d, "chrS.idx")
    t0 = time.time()
    W.write_index(idx, {"chrS": W.synthetic_sites(a.positions, a.spacing)})
    res = {"index": {"write_s": round(time.time() - t0, 1), "bytes": os.path.getsize(idx)}}
    res["index_on_the_device"] = index_part(a, idx)
    print(json.dumps(res), flush=True)
    if a.files:
        res["file_to_file"] = files_part(a, idx, d)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
