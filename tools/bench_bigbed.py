#!/usr/bin/env python3
"""The bigBed item encoder (csrc/bigbeddev.hip) and the deflate over its blocks (csrc/zlibdev.hip: bsc_zlib_ranges_device) on resident
arrays, beside the per-cytosine table's encoder on the same arrays in the same process.  tools/bench_bigwig.py's sibling.

(1) device: the per-position arrays the reads-in chain leaves for a 2 M-position block at 30x, repeated on the device to --positions
    (default 50 M) and resident in HBM.  --repeats times each behind --warmup, in turn, by HIP events:
      bigbed         bsc_bigbed_sites_device: size kernel, two scans, write kernel, heads, scan, windows, zoom (B = 512)
      table          bsc_meth_sites_device: bsc_meth_size_kernel + one scan + the write kernel — the yardstick (the same record bytes read)
      ranges         bsc_zlib_ranges_device over the blocks of the stream `bigbed` left: deflate, scan, gather, and the entry's one wait
    One copy of the block is checked first: the device's stream, blocks and windows against the host form, every zlib stream of its blocks
    inflated, and the ratio of the device's bytes to Python zlib level 1 (and 6) over the same blocks.
(2) per kernel (--trace-dir DIR): median kernel times from the trace a run of (1) under `rocprofv3 --kernel-trace --output-format csv -d DIR` left.

    python tools/bench_bigbed.py [--positions N] [--repeats 10] [--trace-dir DIR] [--out JSON]
"""
import argparse
import importlib.util
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B_ITEMS = 512
KERNELS = ("bsc_bigbed_size_kernel", "bsc_bigbed_write_kernel", "bsc_bigbed_heads_kernel", "bsc_bigbed_windows_kernel", "bsc_bigbed_zoom_kernel",
           "bsc_meth_size_kernel", "bsc_meth_write_kernel", "bsc_zlib_deflate_ranges_large_kernel", "bsc_zlib_scan_kernel", "bsc_zlib_gather_kernel")


def device_part(a):
    import torch

    import bs_call_amd as B
    from bs_call_amd import bigbed

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
    reps = max(1, -(-a.positions // n1))
    n = n1 * reps
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    max_piece = B_ITEMS * bigbed.ITEM_MAX
    res = {"positions": n, "block_positions": n1, "copies_of_the_block": reps, "coverage": 30, "items_per_block": B_ITEMS, "repeats": a.repeats,
           "warmup": a.warmup}

    def offsets_of(d_blk, n_blk, n_bytes):
        """The blocks' byte offsets, and the stream's length behind them, as the u64 array the ranges call takes."""
        off = d_blk[: 24 * n_blk].view(torch.int64).reshape(-1, 3)[:, 2]
        return torch.cat([off, torch.tensor([n_bytes], dtype=torch.int64, device="cuda")]).contiguous()

    with B.SiteCaller() as c:
        d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
        d_core1, d_aux1 = z(n1 * 64), z(n1 * 64)
        c.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core1.data_ptr(), d_aux1.data_ptr())
        torch.cuda.synchronize()
        # one copy of the block: the device's result against the host form over the same arrays, its blocks deflated and inflated
        recs = np.concatenate([d_core1.cpu().numpy().reshape(-1, 64), d_aux1.cpu().numpy().reshape(-1, 64)], axis=1).reshape(-1).view(B.VCF_REC)
        want = bigbed.blocks_recs_host(recs, 0, None, {"items_per_block": B_ITEMS})
        sites1 = int(want[1]["count"].sum())
        d_out, d_blk, d_zoom, d_tot = z(len(want[0]) + 16), z(24 * (len(want[1]) + 1)), z(24 * (len(want[2]) + 1)), z(32)
        c.bigbed_sites_device(d_core1.data_ptr(), d_aux1.data_ptr(), n1, x, 0, d_out.data_ptr(), len(want[0]) + 16, d_blk.data_ptr(), len(want[1]) + 1,
                              d_zoom.data_ptr(), len(want[2]) + 1, d_tot.data_ptr(), bb_params={"items_per_block": B_ITEMS})
        torch.cuda.synchronize()
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)[:4]]
        assert tot == [len(want[0]), sites1, len(want[1]), len(want[2])], "the totals differ from the host form's"
        assert d_out.cpu().numpy()[: tot[0]].tobytes() == want[0], "the stream differs from the host form's"
        assert d_blk.cpu().numpy()[: 24 * tot[2]].tobytes() == want[1].tobytes() and d_zoom.cpu().numpy()[: 24 * tot[3]].tobytes() == want[2].tobytes()
        d_offs1 = offsets_of(d_blk, tot[2], tot[0])
        d_z1, d_zs1, d_zt1 = z(tot[0] + 11 * tot[2]), z(4 * tot[2]), z(24)
        c.zlib_ranges_device(d_out.data_ptr(), d_offs1.data_ptr(), tot[2], max_piece, d_z1.data_ptr(), d_z1.numel(), d_zs1.data_ptr(), tot[2], d_zt1.data_ptr())
        torch.cuda.synchronize()
        zt1 = [int(v) for v in d_zt1.cpu().numpy().view(np.uint64)[:3]]
        zs1 = d_zs1.cpu().numpy().view(np.uint32)[: tot[2]]
        blob, at, offs = d_z1.cpu().numpy()[: zt1[0]].tobytes(), 0, [int(v) for v in want[1]["off"]] + [len(want[0])]
        lvl1 = lvl6 = 0
        for k in range(tot[2]):
            piece = want[0][offs[k] : offs[k + 1]]
            assert zlib.decompress(blob[at : at + int(zs1[k])]) == piece, "a stream does not inflate to its block"
            at += int(zs1[k])
            lvl1 += len(zlib.compress(piece, 1))
            lvl6 += len(zlib.compress(piece, 6))
        res["one_copy"] = {"sites": sites1, "blocks": tot[2], "windows": tot[3], "raw": tot[0], "device": zt1[0], "zlib_level_1": lvl1, "zlib_level_6": lvl6,
                           "device_over_level_1": round(zt1[0] / lvl1, 4), "device_over_level_6": round(zt1[0] / lvl6, 4), "ratio": round(tot[0] / zt1[0], 4)}
        d_core, d_aux = d_core1.repeat(reps), d_aux1.repeat(reps)
        del d_core1, d_aux1, d_out, d_blk, d_zoom, d_z1, d_zs1
        sites = sites1 * reps
        n_blk, n_win = sites // B_ITEMS + 1, n // 1024 + 2
        d_out, d_blk, d_zoom = z(sites * 100 + 4096), z(24 * n_blk), z(24 * n_win)
        d_tab, d_ttot = z(sites * 100 + 4096), z(40)
        fns = {
            "bigbed": lambda: c.bigbed_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, x, 0, d_out.data_ptr(), d_out.numel(), d_blk.data_ptr(), n_blk,
                                                    d_zoom.data_ptr(), n_win, d_tot.data_ptr(), bb_params={"items_per_block": B_ITEMS}),
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
        tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)[:4]]
        ttot = [int(v) for v in d_ttot.cpu().numpy().view(np.uint64)[:2]]
        assert tot[1] == sites == ttot[1] and tot[0] <= d_out.numel() and tot[2] <= n_blk and tot[3] <= n_win and ttot[0] <= d_tab.numel()
        del d_core, d_aux, d_tab
        d_offs = offsets_of(d_blk, tot[2], tot[0])
        d_z, d_zs, d_zt = z(tot[0] + 11 * tot[2]), z(4 * tot[2]), z(24)
        run = lambda: c.zlib_ranges_device(d_out.data_ptr(), d_offs.data_ptr(), tot[2], max_piece, d_z.data_ptr(), d_z.numel(), d_zs.data_ptr(), tot[2],
                                           d_zt.data_ptr())
        ms["ranges"] = []
        for _ in range(a.warmup):
            run()
        for _ in range(a.repeats):
            ms["ranges"].append(timed(run))
        zt = [int(v) for v in d_zt.cpu().numpy().view(np.uint64)[:3]]
        assert zt[1] == tot[2] and zt[2] == 0 and zt[0] <= d_z.numel()
        res.update({k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in ms.items()})
        res.update({"sites": sites, "blocks": tot[2], "windows": tot[3], "stream_bytes": tot[0], "table_bytes": ttot[0], "compressed_bytes": zt[0],
                    "stream_over_table": round(tot[0] / ttot[0], 4), "ratio": round(tot[0] / zt[0], 4),
                    "bigbed_over_table_time": round(float(np.median(ms["bigbed"])) / float(np.median(ms["table"])), 4),
                    "ranges_ns_per_input_byte": round(float(np.median(ms["ranges"])) * 1e6 / tot[0], 5)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": device_part(a)}
    print(json.dumps(res), flush=True)
    if a.trace_dir:
        spec = importlib.util.spec_from_file_location("bench_bigwig", os.path.join(ROOT, "tools", "bench_bigwig.py"))
        T = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(T)
        T.KERNELS = KERNELS  # its reader of a kernel trace, over this tool's kernels
        res["kernels"] = T.trace_part(a.trace_dir)
        print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
