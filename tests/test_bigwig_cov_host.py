"""The coverage bigWig track on the host (csrc/bigwig.c: bsc_bigwig_cov_sections_recs, bsc_bigwig_open_track and a coverage writer): the
finished file, plain and compressed, against the independent builder of tests/bigwig_cov_ref.py byte for byte over section counts, contig
counts, zoom level counts and a window two adds share; sums whose float differs between one rounding and two; sums of squares beyond 2^64 in
a section, in a merged window and in the total; every refusal of the level writer, with the file's length unchanged; a coverage block added
to a level writer; the host form against the Python rule on random records; the sanitizer program.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bigwig_cov_ref as RC
import bigwig_ref as R
from bs_call_amd import bigwig
from bs_call_amd.caller import BscError
from methregions_ref import random_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
TOP = 2**32 - 1


def cov_block(sites, tid, S, red):
    """(data, sections, zoom0) of a block's (start, c) sites: bs_call_amd/bigwig.py's form, held to the reference's here."""
    data, secs, zoom = bigwig.sections_of_sites(sites, tid, S, red, track="coverage")
    want = RC.block_entries(tid, sites, S, red)
    assert (data, R.sum_rows(secs), R.sum_rows(zoom)) == want
    return data, secs, zoom


def write_file(path, refs, blocks, S, red, compress=False):
    with bigwig.Writer(path, refs, S, red, compress=compress, track="coverage") as w:
        for tid, sites in blocks:
            data, secs, zoom = cov_block(sites, tid, S, red)
            if compress:
                zdata, zs = RC.z_sections(data, S)
                w.add_z(tid, zdata, np.array(zs, dtype=np.uint32), secs, zoom)
            else:
                w.add(tid, data, secs, zoom)
        w.finish()
    return open(path, "rb").read()


def spaced(rng, n, first=0, step=1):
    """n (start, c) sites at first, first + step, .. with depths from 1 to the top of the range."""
    scale = rng.choice([1, 30, 1000, 2**24, TOP], n)
    return [(first + k * step, max(1, int(rng.random() * float(s)))) for k, s in enumerate(scale)]


# ---- 1. the value and the roundings ------------------------------------------------------------------------------------------------------------
def test_value_bytes_and_the_reference_s_rounding():
    ties = [0, 1, 2**24 - 1, 2**24, 2**24 + 1, 2**24 + 3, 2**25 + 2, 2**25 + 6, 2**31, 2**32 - 129, 2**32 - 128, TOP]
    for c in ties + [int(v) for v in np.random.default_rng(1).integers(0, 2**32, 5000)]:
        want = np.array([c], dtype=np.uint32).astype(np.float32).tobytes()  # numpy's u32 -> f32: the hardware's conversion
        assert bigwig.cov_value_bytes(c) == want == RC.f32(c), c
    assert RC.f32(2**24 + 1) == struct.pack("<f", 2.0**24) and RC.f32(2**24 + 3) == struct.pack("<f", 2.0**24 + 4) and RC.f32(2**32 - 128) == struct.pack("<f", 2.0**32)
    # 64-bit and 96-bit integers: against exact rational arithmetic
    from fractions import Fraction

    rng = np.random.default_rng(2)
    for _ in range(2000):
        v = int(rng.integers(2**40, 2**63)) * int(rng.integers(1, 2**33)) + int(rng.integers(0, 3))
        for pack, fmt in ((RC.f32, "<f"), (RC.f64, "<d")):
            x = struct.unpack(fmt, pack(v))[0]
            step = 2 ** (v.bit_length() - (24 if fmt == "<f" else 53))
            assert abs(Fraction(x) - v) * 2 <= step  # a nearest neighbour
            if abs(Fraction(x) - v) * 2 == step:  # a tie: the even one
                assert (int(x) // step) % 2 == 0


# ---- 2. the finished file ----------------------------------------------------------------------------------------------------------------------
FILE_CASES = {
    "no site at all": ([("chr1", 1000)], [], 1024, 1024, 1),
    "one section": ([("chr1", 1000)], [(0, [(17, 333)])], 1024, 1024, 1),
    "256 sections": ([("chr1", 100000)], [(0, "r256")], 1, 1024, 1),
    "257 sections": ([("chr1", 100000)], [(0, "r257")], 1, 1024, 1),
    "two contigs, S = 3": ([("chr1", 1000), ("chr2", 500)], [(0, "r40"), (1, "r7")], 3, 16, 1),
    "a window two adds share": ([("chr1", 1000)], [(0, [(100, 1), (101, TOP)]), (0, [(102, TOP), (199, 1000)]), (0, [(200, 5)])], 2, 100, 1),
    "two levels": ([("chr1", 1000)], [(0, "r300")], 1024, 1, 2),
    "eight levels": ([("chr1", 257 * 16384 + 5)], [(0, "s257")], 1024, 1, 8),
    "300 contigs": ([("chr%d" % k, 4_000_000_000) for k in range(300)], [(k, [(3_999_999_999, k + 1)]) for k in range(300)], 7, 2**31, 8),
}


def made_blocks(case):
    refs, blocks, S, red, levels = FILE_CASES[case]
    rng = np.random.default_rng(len(case))
    made, first = [], {}
    for tid, sites in blocks:
        if isinstance(sites, str):  # rN: N adjacent sites behind the contig's last; sN: N sites 16384 apart
            n, step = int(sites[1:]), 1 if sites[0] == "r" else 16384
            sites = spaced(rng, n, first.get(tid, 3), step)
        first[tid] = sites[-1][0] + 1
        made.append((tid, sites))
    return refs, made, S, red, levels


@pytest.mark.parametrize("case", list(FILE_CASES))
def test_file_equals_the_reference_builder_plain_and_compressed(tmp_path, case):
    refs, made, S, red, levels = made_blocks(case)
    got = write_file(str(tmp_path / "c.bw"), refs, made, S, red)
    assert got == RC.build(refs, made, S, red)
    f = bigwig.BigWig(got)
    n_sites = sum(len(s) for _, s in made)
    assert f.header["zoomLevels"] == levels and f.section_count == sum(-(-len(s) // S) for _, s in made) and f.summary["basesCovered"] == n_sites
    for tid, _ in made[:3]:
        every = [s for t, ss in made if t == tid for s in ss]
        assert [(s, struct.pack("<f", v)) for s, _, v in f.intervals(refs[tid][0])] == [(s, RC.f32(c)) for s, c in every]
    gz = write_file(str(tmp_path / "z.bw"), refs, made, S, red, compress=True)
    if not n_sites:
        assert gz == got and got[256:296] == bytes(40)
        return
    RC.check_z(gz, refs, made, S, red)
    fz = bigwig.BigWig(gz)
    assert fz.summary == f.summary and fz.header["uncompressBufSize"] > 0
    for l in range(levels):
        assert fz.zoom_records(l) == f.zoom_records(l)
    if "share" in case:
        rec = f.zoom_records(0)[0]
        assert rec["validCount"] == 4 and rec["sumSquares"] == struct.unpack("<f", RC.f32(1 + 2 * TOP * TOP + 10**6))[0]


# ---- 3. one rounding, not two; sums of squares beyond 2^64 --------------------------------------------------------------------------------------
def entries(start, end, count, mn, mx, total, squares):
    return np.array([(start, end, count, mn, mx, squares >> 64, total, squares % 2**64)], dtype=bigwig.BW_SUM)


def test_a_sum_is_rounded_once_from_the_integer(tmp_path):
    # floats near 2^60 are 2^37 apart; 2^60 + 2^36 is the tie between 2^60 and 2^60 + 2^37.  v lies 1 above it: once -> up.  A double keeps
    # 53 bits (steps of 2^8 there), so (double)v is the tie itself, and the second rounding takes it down to the even 2^60.
    v = 2**60 + 2**36 + 1
    assert RC.f32(v) == struct.pack("<f", 2.0**60 + 2.0**37) != struct.pack("<f", float(v))
    # the same in the 96-bit field: 2^90 + 2^66 + 2^20 (2^20 is below the double's last bit, 2^38)
    q = 2**90 + 2**66 + 2**20
    assert RC.f32(q) == struct.pack("<f", 2.0**90 + 2.0**67) != struct.pack("<f", float(q))
    # and for the total's f64: 2^95 + 2^42 + 1 lies 1 above the tie of two doubles 2^43 apart
    t = 2**95 + 2**42 + 1
    assert RC.f64(t) == struct.pack("<d", 2.0**95 + 2.0**43)
    path = str(tmp_path / "r.bw")
    with bigwig.Writer(path, [("chr1", 1000)], 4, 1000, track="coverage") as w:
        e = entries(5, 6, 1, 7, 9, v, q)
        w.add(0, bytes(32), e, e)
        w.finish()
    f = bigwig.read(path)
    rec = f.zoom_records(0)[0]
    assert struct.pack("<ff", rec["sumData"], rec["sumSquares"]) == RC.f32(v) + RC.f32(q)
    assert struct.pack("<ff", rec["minVal"], rec["maxVal"]) == struct.pack("<ff", 7.0, 9.0)
    assert struct.pack("<d", f.summary["sumSquares"]) == RC.f64(q) and f.summary["sumData"] == 2.0**60 + 2.0**36
    path = str(tmp_path / "t.bw")
    with bigwig.Writer(path, [("chr1", 1000)], 4, 1000, track="coverage") as w:
        e = entries(5, 6, 1, 7, 9, 2**63 + 2**10 + 1, t)  # (2^63 + 2^10 + 1: 1 above the tie of two doubles 2^11 apart)
        w.add(0, bytes(32), e, e)
        w.finish()
    f = bigwig.read(path)
    assert struct.pack("<dd", f.summary["sumData"], f.summary["sumSquares"]) == RC.f64(2**63 + 2**10 + 1) + RC.f64(t)
    assert f.summary["sumData"] == 2.0**63 + 2.0**11 and f.summary["minVal"] == 7.0 and f.summary["maxVal"] == 9.0


@pytest.mark.parametrize("compress", [False, True])
def test_sums_of_squares_beyond_2_64(tmp_path, compress):
    # 70 sites of c = 2^32 - 1 in a section (S = 70), two such adds in ONE window of 1000, and a third add behind it: the section's,
    # the merged window's and the total's sums of squares are all above 2^64
    refs, S, red = [("chr1", 10_000)], 70, 1000
    blocks = [(0, [(k, TOP) for k in range(70)]), (0, [(100 + k, TOP) for k in range(70)]), (0, [(2000 + k, TOP - k) for k in range(300)])]
    data, secs, zoom = cov_block(blocks[0][1], 0, S, red)
    assert int(secs["_pad"][0]) == (70 * TOP * TOP) >> 64 == 69 and int(secs["sum_m2"][0]) == (70 * TOP * TOP) % 2**64 and int(zoom["_pad"][0]) == 69
    got = write_file(str(tmp_path / "w.bw"), refs, blocks, S, red, compress)
    if compress:
        RC.check_z(got, refs, blocks, S, red)
    else:
        assert got == RC.build(refs, blocks, S, red)
    f = bigwig.BigWig(got)
    first = f.zoom_records(0)[0]
    assert first["validCount"] == 140 and struct.pack("<f", first["sumSquares"]) == RC.f32(140 * TOP * TOP) and 140 * TOP * TOP > 2**71
    total = 140 * TOP * TOP + sum((TOP - k) ** 2 for k in range(300))
    assert struct.pack("<d", f.summary["sumSquares"]) == RC.f64(total) and total > 2**72
    assert f.summary["sumData"] == float(140 * TOP + sum(TOP - k for k in range(300))) and f.summary["maxVal"] == float(TOP)


# ---- 4. refusals; the two writers side by side --------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_level_writer_with_the_length_unchanged(tmp_path):
    refs = [("chr1", 1000), ("chr2", 1000)]
    S, red = 4, 10
    blk = lambda sites, tid: cov_block(sites, tid, S, red)
    path = str(tmp_path / "o.bw")
    with bigwig.Writer(path, refs, S, red, track="coverage") as w:
        w.add(1, *blk([(10, 1), (20, 2)], 1))
        size0 = os.path.getsize(path)
        for tid, sites in ((0, [(500, 1)]), (1, [(20, 3)]), (1, [(5, 3)]), (2, [(500, 1)])):  # a lower tid; a start below the previous end; no such contig
            with pytest.raises(BscError):
                w.add(tid, *blk(sites, tid))
        data, secs, zoom = blk([(21, 5), (22, 6), (23, TOP), (24, 8), (30, 9)], 1)
        with pytest.raises(BscError):  # bytes that are not the sections'
            w.add(1, data[:-8], secs, zoom)
        bad = secs.copy()
        bad["count"][0] = 3  # a section that is not full before the last
        with pytest.raises(BscError):
            w.add(1, data, bad, zoom)
        with pytest.raises(BscError):  # sections without a window
            w.add(1, data, secs, zoom[:0])
        badz = zoom.copy()
        badz["end"][0] = badz["start"][0] + 2 * red  # a window that is not one window
        with pytest.raises(BscError):
            w.add(1, data, secs, badz)
        with pytest.raises(BscError, match="plain"):  # add_z into a plain file
            zdata, zs = RC.z_sections(data, S)
            w.add_z(1, zdata, np.array(zs, dtype=np.uint32), secs, zoom)
        assert os.path.getsize(path) == size0
        w.add(1, data, secs, zoom)  # a start AT the previous end is in order
        w.finish()
        size1 = os.path.getsize(path)
        with pytest.raises(BscError):
            w.finish()
        with pytest.raises(BscError):
            w.add(1, *blk([(40, 1)], 1))
        assert os.path.getsize(path) == size1
    want = [(1, [(10, 1), (20, 2)]), (1, [(21, 5), (22, 6), (23, TOP), (24, 8), (30, 9)])]
    assert open(path, "rb").read() == RC.build(refs, want, S, red)
    # the compressed writer's own: sizes that do not add up, a size of 0, a size above raw + 11, add behind add_z
    path = str(tmp_path / "z.bw")
    with bigwig.Writer(path, refs, S, red, compress=True, track="coverage") as w:
        data, secs, zoom = blk([(10, 1), (20, 2)], 0)
        zdata, zs = RC.z_sections(data, S)
        w.add_z(0, zdata, np.array(zs, dtype=np.uint32), secs, zoom)
        size0 = os.path.getsize(path)
        data, secs, zoom = blk([(40, 6), (41, 7)], 0)
        zdata, zs = RC.z_sections(data, S)
        for bad_data, bad_sizes, word in ((zdata + b"\0", zs, "add up"), (zdata[:-1], zs, "add up"), (b"\0", [0], "stream of"), (bytes(24 + 16 + 12), [24 + 16 + 12], "stream of")):
            with pytest.raises(BscError, match=word):
                w.add_z(0, bad_data, np.array(bad_sizes, dtype=np.uint32), secs, zoom)
        with pytest.raises(BscError, match="compressed"):
            w.add(0, data, secs, zoom)
        assert os.path.getsize(path) == size0
        w.add_z(0, zdata, np.array(zs, dtype=np.uint32), secs, zoom)
        w.finish()
    RC.check_z(open(path, "rb").read(), refs, [(0, [(10, 1), (20, 2)]), (0, [(40, 6), (41, 7)])], S, red)
    # the opening's refusals
    for bad in ((0, 10), (65536, 10), (4, 0)):
        with pytest.raises(BscError):
            bigwig.Writer(str(tmp_path / "bad.bw"), refs, *bad, track="coverage")
    with pytest.raises(ValueError):
        bigwig.Writer(str(tmp_path / "bad.bw"), refs, track="depth")
    assert not os.path.exists(str(tmp_path / "bad.bw"))
    L = bigwig._lib.load()
    import ctypes as C

    for track in (0, 3, 4):
        h = C.c_void_p(7)
        names = (C.c_char_p * 1)(b"chr1")
        lens = np.array([1000], dtype=np.uint32)
        with open(str(tmp_path / "t.bw"), "wb") as fh:
            assert L.bsc_bigwig_open_track(fh.fileno(), 1, names, lens.ctypes.data, C.byref(bigwig._lib.BwParams()), track, C.byref(h)) == -1 and h.value is None


def test_a_coverage_block_in_a_level_writer_changes_nothing(tmp_path):
    """A level writer takes a summary's integers as m: it ignores _pad (a coverage summary's high bits) as it always has, its bytes are those
    of bsc_bigwig_open's writer, and bsc_bigwig_open is bsc_bigwig_open_track with BSC_BW_LEVEL."""
    refs, S, red = [("chr1", 10_000)], 4, 100
    level_sites = [(10, 0), (11, 1000), (150, 333), (151, 5), (152, 7)]
    want = R.build(refs, [(0, level_sites)], S, red)
    for track in (None, "level"):
        path = str(tmp_path / "l.bw")
        with (bigwig.Writer(path, refs, S, red) if track is None else bigwig.Writer(path, refs, S, red, track=track)) as w:
            data, secs, zoom = bigwig.sections_of_sites(level_sites, 0, S, red)
            secs["_pad"], zoom["_pad"] = 77, 99  # what a coverage summary may carry
            w.add(0, data, secs, zoom)
            w.finish()
        assert open(path, "rb").read() == want
    # a window two adds share, both with high bits set: the level file is the level file
    blocks = [(0, [(10, 1), (11, 2)]), (0, [(12, 3), (13, 4)])]
    path = str(tmp_path / "m.bw")
    with bigwig.Writer(path, refs, S, red) as w:
        for tid, sites in blocks:
            data, secs, zoom = bigwig.sections_of_sites(sites, tid, S, red)
            secs["_pad"], zoom["_pad"] = 2**32 - 1, 2**32 - 1
            w.add(tid, data, secs, zoom)
        w.finish()
    assert open(path, "rb").read() == R.build(refs, blocks, S, red)
    # real coverage entries (depths within 0 .. 1000 so that both readings are defined) into a level writer: it reads them as tenths of a percent
    cov_sites = [(10, 30), (11, 1000), (12, 7)]
    path = str(tmp_path / "x.bw")
    with bigwig.Writer(path, refs, S, red) as w:
        data, secs, zoom = cov_block(cov_sites, 0, S, red)
        w.add(0, data, secs, zoom)
        w.finish()
    got = open(path, "rb").read()
    lv = R.build(refs, [(0, cov_sites)], S, red)
    at = 296 + len(R.chrom_tree(refs, 296)) + 8
    assert got[:at] == lv[:at] and got[at + len(data) :] == lv[at + len(data) :] and got[at : at + len(data)] == data  # all but the stream's bytes, which it never reads


# ---- 5. the host form against the Python rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,red", [(1, 1), (3, 7), (64, 100), (1024, 1024), (65535, 2**32 - 1)])
def test_host_form_equals_the_python_rule(S, red):
    rng = np.random.default_rng(300 + S)
    seen_top = seen_wide = False
    for n, x0, par in ((0, 1, {}), (1, 1, {}), (700, 1, {}), (700, 5000, {"contexts": 1, "min_cov": 3}), (300, 2**32 - 300, {"min_phred": 20, "pass_only": 1})):
        recs = random_records(rng, n, x0, wide=True)
        sites = [s for s in (bigwig.site_of_rec(r, par, "coverage") for r in recs) if s is not None]
        level_sites = [s for s in (bigwig.site_of_rec(r, par) for r in recs) if s is not None]
        assert [s for s, _ in sites] == [s for s, _ in level_sites]  # the two tracks have the same sites
        want = RC.block_entries(9, sites, S, red)
        got = bigwig.sections_recs_host(recs, 9, par, {"items_per_section": S, "reduction": red}, track="coverage")
        assert (got[0], R.sum_rows(got[1]), R.sum_rows(got[2])) == want
        lv = bigwig.sections_recs_host(recs, 9, par, {"items_per_section": S, "reduction": red})
        assert len(lv[0]) == len(got[0]) and [r[:3] for r in R.sum_rows(lv[1])] == [r[:3] for r in want[1]] and [r[:3] for r in R.sum_rows(lv[2])] == [r[:3] for r in want[2]]
        if n >= 300:
            seen_top |= any(c == TOP for _, c in sites)  # saturated depths
            seen_wide |= any(r[5] for r in want[2] + want[1])  # sums of squares beyond 2^64
            room = (len(want[0]), len(want[1]), len(want[2]))
            for k in range(3):
                short = tuple(v - (1 if j == k else 0) for j, v in enumerate(room))
                with pytest.raises(BscError):
                    bigwig.sections_recs_host(recs, 9, par, {"items_per_section": S, "reduction": red}, room=short, track="coverage")
            got = bigwig.sections_recs_host(recs, 9, par, {"items_per_section": S, "reduction": red}, room=room, track="coverage")
            assert (got[0], R.sum_rows(got[1]), R.sum_rows(got[2])) == want
    assert seen_top and (seen_wide or S < 64)  # (a run of one or three sites need not pass 2^64)
    for bad in ({"items_per_section": 0}, {"items_per_section": 65536}, {"reduction": 0}):
        with pytest.raises(BscError):
            bigwig.sections_recs_host(recs, 0, None, bad, track="coverage")
    with pytest.raises(BscError):
        bigwig.sections_recs_host(recs, 0, {"contexts": 2}, track="coverage")


def test_the_value_floats_of_the_host_form():
    sums = [1, 2**24 - 1, 2**24, 2**24 + 1, 2**24 + 3, 2**25 + 2, 2**25 + 6, 2**31, 2**32 - 129, 2**32 - 128, TOP, 2**32, 2**33 - 2]
    recs = R.records_of([(10 + i, v // 2, v - v // 2) for i, v in enumerate(sums)])
    raw, sec, zoom = bigwig.sections_recs_host(recs, 0, None, {"items_per_section": 65535, "reduction": 1}, track="coverage")
    want = np.array([min(v, TOP) for v in sums], dtype=np.uint32).astype(np.float32)
    assert [raw[24 + 8 * i + 4 : 24 + 8 * i + 8] for i in range(len(sums))] == [w.tobytes() for w in want]
    assert [int(z["min_m"]) for z in zoom] == [min(v, TOP) for v in sums] and [int(z["sum_m2"]) + (int(z["_pad"]) << 64) for z in zoom] == [min(v, TOP) ** 2 for v in sums]
    # min_cov is tested on the 64-bit sum, before the saturation
    recs = R.records_of([(10, TOP, TOP), (11, 3, 4)])
    assert len(bigwig.sections_recs_host(recs, 0, {"min_cov": TOP}, track="coverage")[2]) == 1


# ---- 6. sanitizers, the binary's refusals -------------------------------------------------------------------------------------------------------
def test_coverage_host_code_under_sanitizers(tmp_path):
    """make bigwig-cov-san: integration/bigwig_cov_san.c + csrc/bigwig.c + libz under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "bigwig_cov_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "bigwig_cov_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "bigwig.c"), "-lpthread", "-lz", "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


def test_bam2bcf_refusals():
    assert os.path.exists(EXE), "run `make demo`"

    def refused(args, word):
        r = subprocess.run([EXE, *args, "in.bam", "ref.fa", "out.bcf", "out.json"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr)

    refused(["--cov-bigwig", "c.bw", "--rank", "0", "--world", "2"], "--cov-bigwig writes a single run's track")
    refused(["--cov-bigwig", "c.bw", "--merge", "2"], "--cov-bigwig writes a single run's track")
    refused(["--cov-bigwig", "c.bw", "--meth-bigwig-section", "0"], "1 .. 65535")
    refused(["--cov-bigwig", "c.bw", "--meth-bigwig-compress", "--meth-bigwig-section", "8158"], "8157")
    r = subprocess.run([EXE, "--cov-bigwig", "c.bw", "in.bam", "ref.fa", "out.bcf", "out.json"], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, BAM2BCF_HOST_BCF="1"))
    assert r.returncode == 2 and "--cov-bigwig" in r.stderr and "BAM2BCF_HOST" in r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "--cov-bigwig cov.bw" in r.stderr
