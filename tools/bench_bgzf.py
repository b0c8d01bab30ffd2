#!/usr/bin/env python3
"""BGZF on the device (csrc/bgzfdev.hip): (1) the compressor alone on a resident BCF stream of >= 1 GB made by the device encoder at 30x
(a 2 M-position block's stream, repeated on the device): GB/s of input and the ratio; (2) host zlib levels 1 and 6 on a sample of the same
members, 16 threads at the most; (3) integration/bam2bcf -O b against -O u file to file at 50 Mb / 30x (tools/make_wgbs_bam.c, 16 threads
at the most), the -O b file checked to inflate to the -O u file's bytes.
usage: python tools/bench_bgzf.py [out.json [positions]]     (writes its files under $BENCH_TMP, default /tmp/bench_bgzf)"""
import concurrent.futures as cf
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

out_json = sys.argv[1] if len(sys.argv) > 1 else None
n_pos = int(sys.argv[2]) if len(sys.argv) > 2 else 50_000_000
M = 0xFF00
THREADS = min(16, len(os.sched_getaffinity(0)))
res = {"threads": THREADS}

# (1) the compressor alone
seed = 88172645463325252
tpl, seq = B.synth_reads_host(seed, 5_000, 2_000_000, 30)
x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
with B.SiteCaller() as c:
    blob, n_rec = c.block_bcf(tpl, seq, x, y, B.synth_ref_host(seed, x, y - x + 3), 0)
    one = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda")
    reps = -(-(1 << 30) // len(one))
    stream = one.repeat(reps)
    torch.cuda.synchronize()
    n = stream.numel()
    times, out = [], None
    for _ in range(4):
        z = c.bgzf()
        t0 = time.perf_counter()
        z.write_device(stream.data_ptr(), n)
        times.append(time.perf_counter() - t0)
        out = z.take() + z.close()
    sample = stream[: 512 * M].cpu().numpy().tobytes()
best = min(times[1:])
res["device"] = {"input_bytes": n, "bcf_records_per_copy": int(n_rec), "copies": reps, "seconds": [round(t, 4) for t in times], "GB_per_s": round(n / best / 1e9, 2),
                 "output_bytes": len(out), "ratio": round(n / len(out), 3)}
print("device", res["device"], flush=True)


# (2) host zlib on 512 members of the same stream
def member(args):
    lvl, k = args
    co = zlib.compressobj(lvl, zlib.DEFLATED, -15)
    return 18 + len(co.compress(sample[k : k + M]) + co.flush()) + 8


res["host_zlib"] = {}
for lvl in (1, 6):
    with cf.ThreadPoolExecutor(THREADS) as ex:
        t0 = time.perf_counter()
        sizes = list(ex.map(member, [(lvl, k) for k in range(0, len(sample), M)]))
        dt = time.perf_counter() - t0
    res["host_zlib"]["level%d" % lvl] = {"sample_bytes": len(sample), "threads": THREADS, "MB_per_s": round(len(sample) / dt / 1e6, 1),
                                         "ratio": round(len(sample) / sum(sizes), 3)}
print("host", res["host_zlib"], flush=True)

# (3) bam2bcf -O b against -O u, file to file
d = os.environ.get("BENCH_TMP", "/tmp/bench_bgzf")
os.makedirs(d, exist_ok=True)
gen = os.path.join(d, "make_wgbs_bam")
subprocess.check_call(["gcc", "-O2", "-o", gen, os.path.join(ROOT, "tools", "make_wgbs_bam.c"), "-lz", "-lpthread", "-lm"])
bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "ref.fa")
t0 = time.time()
subprocess.check_output([gen, bam, fa, str(n_pos), "30", "88172645463325253", str(THREADS), "1", "0", "1", "0"])
res["bam2bcf"] = {"positions": n_pos, "coverage": 30, "generate_s": round(time.time() - t0, 1)}
exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
for mode in ("u", "b", "u", "b"):
    ob, orp = os.path.join(d, mode + ".bcf"), os.path.join(d, mode + ".json")
    for f_ in (ob, orp):
        if os.path.exists(f_):
            os.remove(f_)
    t0 = time.time()
    r = subprocess.run([exe, "-O", mode, bam, fa, ob, orp], capture_output=True, text=True, env=dict(os.environ, BAM2BCF_TIMING="1"))
    dt = time.time() - t0
    if r.returncode != 0:
        print(r.stderr[-2000:])
        raise SystemExit(1)
    st = json.loads(r.stderr.strip().splitlines()[-1])
    e = res["bam2bcf"].setdefault("O" + mode, {"runs": []})
    e["runs"].append({"process_wall_s": round(dt, 3), "wall_without_context_s": st["wall_without_context_s"], "encode_write_s": st["encode_write_s"],
                      "pwrite_s": st["output_thread"]["pwrite_s"]})
    e["bytes"] = os.path.getsize(ob)
    print(mode, e["runs"][-1], flush=True)


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


b2 = res["bam2bcf"]
b2["Ob_inflates_to_Ou_bytes"] = sha_file(os.path.join(d, "b.bcf"), gz=True) == sha_file(os.path.join(d, "u.bcf"))
for k in ("Ou", "Ob"):
    b2[k]["best_wall_without_context_s"] = min(r_["wall_without_context_s"] for r_ in b2[k]["runs"])
b2["Ob_over_Ou"] = round(b2["Ob"]["best_wall_without_context_s"] / b2["Ou"]["best_wall_without_context_s"], 3)
b2["ratio"] = round(b2["Ou"]["bytes"] / b2["Ob"]["bytes"], 3)
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as f:
        json.dump(res, f, indent=1)
