"""The methylation bigWig track on the host (csrc/bigwig.c): the host form of a block's stream and summaries against the Python form of the
rule (bs_call_amd/bigwig.py) — every value of m and a hand-checked rounding table —, the finished file against the independent builder of
tests/bigwig_ref.py byte for byte over section counts, contig counts, block cuts and zoom level counts, the reader's R-tree walk against a
linear scan, the refusals, and the writer under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bigwig_ref as R
from bs_call_amd import _lib, bigwig
from bs_call_amd.caller import BscError
from methregions_ref import random_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")


def same_block(got, want):
    assert got[0] == want[0]
    assert R.sum_rows(got[1]) == R.sum_rows(want[1]) and R.sum_rows(got[2]) == R.sum_rows(want[2])


# ---- 1. the host form against the Python form -------------------------------------------------------------------------------------------------
# a, b -> m = 1000 a / (a + b) rounded half up, worked by hand
ROUNDING = [(1, 1999, 1), (1, 2000, 0), (3, 1997, 2), (1, 7, 125), (1, 15, 63), (15, 1, 938), (1, 2, 333), (2, 1, 667), (1, 199, 5), (1, 200, 5),
            (1, 201, 5), (1, 399, 3), (3, 397, 8), (0, 5, 0), (5, 0, 1000), (2**32 - 1, 2**32 - 1, 500), (2**32 - 1, 1, 1000), (1, 2**32 - 1, 0),
            (1999, 1, 1000), (3999, 2, 1000), (3998, 2, 1000), (1997, 3, 999)]


def test_value_table_and_rounding():
    # 1000 a / (a + b): 1000/2000 = 0.5 -> 1; 1000/2001 -> 0; 3000/2000 = 1.5 -> 2; 125; 62.5 -> 63; 937.5 -> 938; 333.3 -> 333; 666.7 -> 667;
    # 1000/200 = 5; 1000/201 = 4.975 -> 5; 1000/202 = 4.950 -> 5; 1000/400 = 2.5 -> 3; 3000/400 = 7.5 -> 8; 0; 1000; 500; 999.9999998 -> 1000;
    # 0.0000002 -> 0; 1999000/2000 = 999.5 -> 1000; 3999000/4001 = 999.5001 -> 1000; 3998000/4000 = 999.5 -> 1000; 1997000/2000 = 998.5 -> 999
    recs = R.records_of([(10 + 3 * i, a, b) for i, (a, b, _) in enumerate(ROUNDING)])
    raw, sec, zoom = bigwig.sections_recs_host(recs, 0, bw_params={"items_per_section": 65535, "reduction": 1})
    assert [int(z["min_m"]) for z in zoom] == [m for _, _, m in ROUNDING] == [int(z["max_m"]) for z in zoom]
    same_block((raw, sec, zoom), bigwig.sections_of_recs(recs, 0, None, 65535, 1))
    # every value of m, 0 .. 1000: a = m of 1000 reads; the float written is (float)(m / 10.0)
    recs = R.records_of([(5 + i, m, 1000 - m) for i, m in enumerate(range(1001))])
    raw, sec, zoom = bigwig.sections_recs_host(recs, 3, bw_params={"items_per_section": 1001, "reduction": 4096})
    assert len(raw) == 24 + 8 * 1001 and len(sec) == 1
    for m in range(1001):
        s, v = struct.unpack_from("<I4s", raw, 24 + 8 * m)
        assert s == 4 + m and v == struct.pack("<f", m / 10.0) == np.float32(np.float64(m) / np.float64(10.0)).tobytes()
    assert R.sum_rows(sec) == [(4, 1005, 1001, 0, 1000, 0, 500500, sum(m * m for m in range(1001)))]
    assert struct.unpack_from("<IIIIIBBH", raw, 0) == (3, 4, 1005, 0, 1, 2, 0, 1001)


@pytest.mark.parametrize("S,red", [(1, 1), (3, 7), (64, 100), (1024, 1024), (65535, 2**32 - 1)])
def test_host_form_equals_the_python_form(S, red):
    rng = np.random.default_rng(100 + S)
    for n, x0, par in ((0, 1, {}), (1, 1, {}), (700, 1, {}), (700, 5000, {"contexts": 1, "min_cov": 3}), (300, 2**32 - 300, {"min_phred": 20, "pass_only": 1})):
        recs = random_records(rng, n, x0, wide=True)
        want = bigwig.sections_of_recs(recs, 9, par, S, red)
        got = bigwig.sections_recs_host(recs, 9, par, {"items_per_section": S, "reduction": red})
        same_block(got, want)
        if n >= 300:
            assert len(want[1]) >= (2 if S < 100 and not par else 1) and len(want[0]) == 24 * len(want[1]) + 8 * int(want[1]["count"].sum())
            # a room one short in each of the three: refused, the needs reported, nothing written (the guard bytes are checked inside)
            room = (len(want[0]), len(want[1]), len(want[2]))
            for k in range(3):
                short = tuple(v - (1 if j == k else 0) for j, v in enumerate(room))
                with pytest.raises(BscError):
                    bigwig.sections_recs_host(recs, 9, par, {"items_per_section": S, "reduction": red}, room=short)
            same_block(bigwig.sections_recs_host(recs, 9, par, {"items_per_section": S, "reduction": red}, room=room), want)
    if red == 7:
        assert any(int(z["count"]) > 1 for z in want[2])


def test_defaults_and_bad_parameters():
    L = _lib.load()
    p = _lib.BwParams(1, 1)
    L.bsc_bw_params_default(p)
    assert (p.items_per_section, p.reduction) == (1024, 1024)
    recs = R.records_of([(10, 1, 1)])
    for bad in ({"items_per_section": 0}, {"items_per_section": 65536}, {"reduction": 0}):
        with pytest.raises(BscError):
            bigwig.sections_recs_host(recs, 0, None, bad)
    with pytest.raises(BscError):
        bigwig.sections_recs_host(recs, 0, {"contexts": 2})


# ---- 2. the finished file against the independent builder ------------------------------------------------------------------------------------
def write_file(path, refs, blocks, S, red):
    with bigwig.Writer(path, refs, S, red) as w:
        for tid, sites in blocks:
            w.add(tid, *bigwig.sections_of_sites(sites, tid, S, red))
        w.finish()
    return open(path, "rb").read()


def spaced(rng, n, first=0, step=1):
    """n (start, m) sites at first, first + step, .. with random m."""
    return [(first + k * step, int(m)) for k, m in enumerate(rng.integers(0, 1001, n))]


FILE_CASES = {
    "no site at all": ([("chr1", 1000)], [], 1024, 1024, 1),
    "one site": ([("chr1", 1000)], [(0, [(17, 333)])], 1024, 1024, 1),
    "S = 1": ([("chr1", 1000), ("chr2", 500)], [(0, "r40"), (1, "r7")], 1, 16, 1),
    "S = 3": ([("chr1", 1000), ("chr2", 500)], [(0, "r40"), (1, "r7")], 3, 16, 1),
    "S = 1024": ([("chr1", 100000)], [(0, "r2500")], 1024, 64, 1),
    "256 sections": ([("chr1", 100000)], [(0, "r256")], 1, 1024, 1),
    "257 sections": ([("chr1", 100000)], [(0, "r257")], 1, 1024, 1),
    "256^2 + 1 sections": ([("a", 100000), ("b", 100000)], [(0, "r30000"), (0, "r20000"), (1, "r15537")], 1, 1024, 1),
    "a window two blocks share": ([("chr1", 1000)], [(0, [(100, 1), (101, 2)]), (0, [(102, 3), (199, 1000)]), (0, [(200, 0)])], 2, 100, 1),
    "a window at the contig's last base": ([("chr1", 1000), ("chr2", 4096)], [(0, [(998, 5), (999, 7)]), (1, [(0, 1), (4095, 2)])], 1024, 1000, 1),
    "two levels": ([("chr1", 1000)], [(0, "r300")], 1024, 1, 2),
    "eight levels": ([("chr1", 257 * 16384 + 5)], [(0, "s257")], 1024, 1, 8),
    "seven levels, the last of 256 records": ([("chr1", 256 * 16384 + 5000)], [(0, "s256"), (0, [(255 * 16384 + 2048, 9)])], 1024, 1, 7),  # merged at width 4096
    "a reduction whose level widths pass 2^32": ([("chr%d" % k, 4_000_000_000) for k in range(300)], [(k, [(3_999_999_999, k)]) for k in range(300)],
                                                  7, 2**31, 8),
}


@pytest.mark.parametrize("case", list(FILE_CASES))
def test_file_equals_the_reference_builder(tmp_path, case):
    refs, blocks, S, red, levels = FILE_CASES[case]
    rng = np.random.default_rng(len(case))
    made, first = [], {}
    for tid, sites in blocks:
        if isinstance(sites, str):  # rN: N adjacent sites behind the contig's last; sN: N sites 16384 apart
            n, step = int(sites[1:]), 1 if sites[0] == "r" else 16384
            sites = spaced(rng, n, first.get(tid, 3), step)
        first[tid] = sites[-1][0] + 1
        made.append((tid, sites))
    got = write_file(str(tmp_path / "t.bw"), refs, made, S, red)
    want = R.build(refs, made, S, red)
    assert got == want
    f = bigwig.BigWig(got)
    assert f.header["zoomLevels"] == levels and f.section_count == sum(-(-len(s) // S) for _, s in made)
    n_sites = sum(len(s) for _, s in made)
    assert f.summary["basesCovered"] == n_sites and len(f.chroms) == len(refs)
    for tid, sites in made[:3]:
        name = refs[tid][0]
        every = [s for t, ss in made if t == tid for s in ss]
        assert [(s, e) for s, e, _ in f.intervals(name)] == [(s, s + 1) for s, _ in every]
        assert [struct.pack("<f", v) for _, _, v in f.intervals(name)] == [struct.pack("<f", m / 10.0) for _, m in every]
    if not n_sites:
        assert got[256:296] == bytes(40) and f.zoom_records(0) == []


@pytest.mark.parametrize("n_refs", [1, 2, 256, 257, 300])
def test_contig_counts_and_name_order(tmp_path, n_refs):
    refs = [("chr%d" % (k + 1) if k % 5 else "scaffold_%d_random" % k, 10_000 + k) for k in range(n_refs)]  # header order is not memcmp order
    rng = np.random.default_rng(n_refs)
    tids = sorted({0, n_refs // 2, n_refs - 1})
    blocks = [(t, spaced(rng, 20 + t, 5, 3)) for t in tids]
    got = write_file(str(tmp_path / "c.bw"), refs, blocks, 8, 32)
    assert got == R.build(refs, blocks, 8, 32)
    f = bigwig.BigWig(got)
    assert f.chroms == {n: (k, l) for k, (n, l) in enumerate(refs)} and f.chrom_count == n_refs
    for k in {0, 1, n_refs // 3, n_refs - 1} & set(range(n_refs)):  # found by key comparison from the root, as a reader searches
        assert f.chrom_lookup(refs[k][0]) == (k, refs[k][1])
    assert f.chrom_lookup("chr0") is None and f.chrom_lookup("zzz") is None
    for t, sites in blocks:
        assert [s for s, _, _ in f.intervals(refs[t][0])] == [s for s, _ in sites]
    if n_refs > 1:
        assert sorted(n for n, _ in refs) != [n for n, _ in refs]


# ---- 3. the reader -----------------------------------------------------------------------------------------------------------------------------
def test_intervals_and_zoom_records_against_a_linear_scan(tmp_path):
    rng = np.random.default_rng(77)
    refs = [("chrB", 200_000), ("chrA", 50_000)]
    sites = {0: sorted(int(v) for v in set(rng.integers(0, 200_000, 6_000).tolist())), 1: sorted(int(v) for v in set(rng.integers(0, 50_000, 900).tolist()))}
    sites = {t: [(s, int(m)) for s, m in zip(v, rng.integers(0, 1001, len(v)))] for t, v in sites.items()}
    blocks = [(0, sites[0][:2500]), (0, sites[0][2500:2501]), (0, sites[0][2501:]), (1, sites[1])]
    got = write_file(str(tmp_path / "q.bw"), refs, blocks, 5, 16)
    assert got == R.build(refs, blocks, 5, 16)
    f = bigwig.read(str(tmp_path / "q.bw"))
    assert f.header["zoomLevels"] >= 3
    for _ in range(60):
        t = int(rng.integers(0, 2))
        lo = int(rng.integers(0, refs[t][1]))
        hi = lo + int(rng.choice([0, 1, 5, 300, 40_000]))
        want = [(s, s + 1, struct.pack("<f", m / 10.0)) for s, m in sites[t] if lo <= s < hi]
        assert [(s, e, struct.pack("<f", v)) for s, e, v in f.intervals(refs[t][0], lo, hi)] == want
    assert f.intervals("chrZ") == []
    for level, (red, _, _) in enumerate(f.zooms):
        assert red == 16 * 4**level
        for t in (0, 1):
            recs = f.zoom_records(level, refs[t][0])
            assert sum(r["validCount"] for r in recs) == len(sites[t]) and [r for r in f.zoom_records(level) if r["chromId"] == t] == recs
            for r in recs[:: max(1, len(recs) // 50)]:
                inside = [m for s, m in sites[t] if r["start"] <= s < r["end"]]
                assert len(inside) == r["validCount"] and r["start"] // red == (r["end"] - 1) // red
                f32 = lambda x: struct.unpack("<f", struct.pack("<f", x))[0]
                assert (r["minVal"], r["maxVal"], r["sumData"], r["sumSquares"]) == (f32(min(inside) / 10.0), f32(max(inside) / 10.0), f32(sum(inside) / 10.0),
                                                                                   f32(sum(m * m for m in inside) / 100.0))
            lo, hi = refs[t][1] // 3, refs[t][1] // 2
            assert f.zoom_records(level, refs[t][0], lo, hi) == [r for r in recs if r["start"] < hi and lo < r["end"]]
    every = [m for t in (0, 1) for _, m in sites[t]]
    assert f.summary == {"basesCovered": len(every), "minVal": min(every) / 10.0, "maxVal": max(every) / 10.0, "sumData": sum(every) / 10.0,
                         "sumSquares": sum(m * m for m in every) / 100.0}


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_out_of_order_add_is_refused(tmp_path):
    refs = [("chr1", 1000), ("chr2", 1000)]
    blk = lambda sites, tid: bigwig.sections_of_sites(sites, tid, 4, 10)
    with bigwig.Writer(str(tmp_path / "o.bw"), refs, 4, 10) as w:
        w.add(1, *blk([(10, 1), (20, 2)], 1))
        for tid, sites in ((0, [(500, 1)]), (1, [(20, 3)]), (1, [(5, 3)]), (2, [(500, 1)])):  # a lower tid; a start below the previous end; no such contig
            with pytest.raises(BscError):
                w.add(tid, *blk(sites, tid))
        data, secs, zoom = blk([(21, 5), (22, 6), (23, 7), (24, 8), (30, 9)], 1)
        with pytest.raises(BscError):  # bytes that are not the sections'
            w.add(1, data[:-8], secs, zoom)
        bad = secs.copy()
        bad["count"][0] = 3  # a section that is not full before the last
        with pytest.raises(BscError):
            w.add(1, data, bad, zoom)
        w.add(1, data, secs, zoom)  # a start AT the previous end is in order
        w.finish()
        with pytest.raises(BscError):
            w.finish()
    want = [(1, [(10, 1), (20, 2)]), (1, [(21, 5), (22, 6), (23, 7), (24, 8), (30, 9)])]
    assert open(str(tmp_path / "o.bw"), "rb").read() == R.build(refs, want, 4, 10)
    for bad in ((0, 10), (65536, 10), (4, 0)):
        with pytest.raises(BscError):
            bigwig.Writer(str(tmp_path / "bad.bw"), refs, *bad)
    assert not os.path.exists(str(tmp_path / "bad.bw"))


def test_writer_under_sanitizers(tmp_path):
    """make bigwig-san: integration/bigwig_san.c + csrc/bigwig.c alone under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "bigwig_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "bigwig_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "bigwig.c"), "-lpthread", "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


def test_bam2bcf_refusals():
    assert os.path.exists(EXE), "run `make demo`"

    def refused(args, word):
        r = subprocess.run([EXE, *args, "in.bam", "ref.fa", "out.bcf", "out.json"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr)

    refused(["--meth-bigwig", "o.bw", "--rank", "0", "--world", "2"], "--meth-bigwig writes a single run's track")
    refused(["--meth-bigwig", "o.bw", "--merge", "2"], "--meth-bigwig writes a single run's track")
    refused(["--meth-bigwig", "o.bw", "--meth-bigwig-section", "0"], "1 .. 65535")
    refused(["--meth-bigwig", "o.bw", "--meth-bigwig-section", "65536"], "1 .. 65535")
    refused(["--meth-bigwig", "o.bw", "--meth-bigwig-zoom", "0"], "1 or more")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "--meth-bigwig out.bw" in r.stderr and "per cytosine even with --meth-merge" in r.stderr
