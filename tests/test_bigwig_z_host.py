"""The compressed bigWig writer on the host (csrc/bigwig.c: bsc_bigwig_add_z, and bsc_bigwig_finish deflating the zoom blocks): the finished
file against tests/bigwig_z_ref.py — every blob, taken out by the R-trees' leaves, inflates to the bytes tests/bigwig_ref.py builds for the
same sites, and the file is byte for byte the layout around its blobs — over section counts, contig counts and zoom level counts; the
refusals, each leaving nothing written; the reader on a compressed and a plain file of the same sites; and the writer under the address and
undefined-behaviour sanitizers as a stand-alone program.  The section blobs here are Python zlib's: the device's are tests/test_gpu_bigwig_z.py's."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bigwig_ref as R
import bigwig_z_ref as Z
from bs_call_amd import bigwig
from bs_call_amd.caller import BscError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")


def z_block(sites, tid, S, red, level=1):
    """(zdata, z_sizes, sections, zoom0) of a block: every section of the plain stream through zlib.compress."""
    data, secs, zoom = bigwig.sections_of_sites(sites, tid, S, red)
    blobs = [zlib.compress(data[k : k + 24 + 8 * S], level) for k in range(0, len(data), 24 + 8 * S)]
    return b"".join(blobs), np.array([len(b) for b in blobs], dtype=np.uint32), secs, zoom


def write_z(path, refs, blocks, S, red):
    with bigwig.Writer(path, refs, S, red, compress=True) as w:
        for tid, sites in blocks:
            w.add_z(tid, *z_block(sites, tid, S, red))
        w.finish()
    return open(path, "rb").read()


def write_plain(path, refs, blocks, S, red):
    with bigwig.Writer(path, refs, S, red) as w:
        for tid, sites in blocks:
            w.add(tid, *bigwig.sections_of_sites(sites, tid, S, red))
        w.finish()
    return open(path, "rb").read()


def spaced(rng, n, first=0, step=1):
    return [(first + k * step, int(m)) for k, m in enumerate(rng.integers(0, 1001, n))]


def same_reading(a, b, refs):
    assert a.summary == b.summary and a.chroms == b.chroms and a.section_count == b.section_count and [z[0] for z in a.zooms] == [z[0] for z in b.zooms]
    for name, size in refs[:3] + refs[-1:]:
        assert a.intervals(name) == b.intervals(name) and a.intervals(name, size // 3, size // 2) == b.intervals(name, size // 3, size // 2)
        for l in range(len(a.zooms)):
            assert a.zoom_records(l, name) == b.zoom_records(l, name)
    for l in range(len(a.zooms)):
        assert a.zoom_records(l) == b.zoom_records(l)


# ---- 1. the layout ----------------------------------------------------------------------------------------------------------------------------
FILE_CASES = {
    "one section": ([("chr1", 1000)], [(0, [(17, 333)])], 1024, 1024, 1),
    "256 sections": ([("chr1", 100000)], [(0, "r256")], 1, 1024, 1),
    "257 sections": ([("chr1", 100000)], [(0, "r257")], 1, 1024, 1),
    "256^2 + 1 sections": ([("a", 100000), ("b", 100000)], [(0, "r30000"), (0, "r20000"), (1, "r15537")], 1, 1024, 1),
    "S = 1024, short last sections": ([("chr1", 100000), ("chr2", 5000)], [(0, "r2500"), (1, "r1025")], 1024, 64, 1),
    "a window two blocks share": ([("chr1", 1000)], [(0, [(100, 1), (101, 2)]), (0, [(102, 3), (199, 1000)]), (0, [(200, 0)])], 2, 100, 1),
    "a zoom block cut at a contig end": ([("chr1", 5000), ("chr2", 5000)], [(0, "r700"), (1, "r600")], 64, 1, 3),  # level 0: 512 + 188 | 512 + 88 records
    "two levels": ([("chr1", 1000)], [(0, "r300")], 1024, 1, 2),
    "eight levels": ([("chr1", 257 * 16384 + 5)], [(0, "s257")], 1024, 1, 8),
    "257 contigs": ([("chr%d" % k, 4_000_000_000) for k in range(257)], [(k, [(3_999_999_999, k)]) for k in range(257)], 7, 2**31, 8),
}


@pytest.mark.parametrize("case", list(FILE_CASES))
def test_file_is_the_layout_around_its_blobs(tmp_path, case):
    refs, blocks, S, red, levels = FILE_CASES[case]
    rng = np.random.default_rng(len(case))
    made, first = [], {}
    for tid, sites in blocks:
        if isinstance(sites, str):  # rN: N adjacent sites behind the contig's last; sN: N sites 16384 apart
            n, step = int(sites[1:]), 1 if sites[0] == "r" else 16384
            sites = spaced(rng, n, first.get(tid, 3), step)
        first[tid] = sites[-1][0] + 1
        made.append((tid, sites))
    got = write_z(str(tmp_path / "z.bw"), refs, made, S, red)
    res = Z.check(got, refs, made, S, red)
    n_sec = sum(-(-len(s) // S) for _, s in made)
    assert len(res["sections"]) == n_sec and len(res["zoom"]) == levels
    raw_blocks = [len(b[3]) for _, recs in R.pyramid(made, red) for b in Z.zoom_blocks(recs)]
    assert res["uncompress_buf_size"] == max([24 + 8 * min(S, len(s)) for _, s in made] + raw_blocks)
    if "contig end" in case:
        assert [len(b[3]) // 32 for b in Z.zoom_blocks(R.pyramid(made, red)[0][1])] == [512, 188, 512, 88]
    # ... and reads back as the plain file of the same sites does
    plain = write_plain(str(tmp_path / "p.bw"), refs, made, S, red)
    assert plain == R.build(refs, made, S, red)
    if S == 1024 and n_sec > 2:  # adjacent positions: zlib halves them
        assert len(got) < len(plain)
    same_reading(bigwig.BigWig(got), bigwig.BigWig(plain), refs)


def test_no_site_at_all_is_the_plain_file(tmp_path):
    refs = [("chr1", 1000), ("chr2", 50)]
    with bigwig.Writer(str(tmp_path / "e.bw"), refs, 8, 8, compress=True) as w:
        w.add_z(0, b"", np.zeros(0, np.uint32), np.zeros(0, bigwig.BW_SUM), np.zeros(0, bigwig.BW_SUM))
        w.finish()
    assert open(str(tmp_path / "e.bw"), "rb").read() == R.build(refs, [], 8, 8)


# ---- 2. refusals: each leaves nothing written ------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_written(tmp_path):
    refs = [("chr1", 1000), ("chr2", 1000)]
    S, red = 4, 10
    a, b = [(10, 1), (20, 2), (21, 3), (22, 4), (30, 5)], [(40, 6), (41, 7)]
    path = str(tmp_path / "r.bw")
    with bigwig.Writer(path, refs, S, red, compress=True) as w:
        w.add_z(0, *z_block(a, 0, S, red))
        size0 = os.path.getsize(path)
        zdata, zs, secs, zoom = z_block(b, 0, S, red)
        with pytest.raises(BscError, match="compressed"):  # add after add_z
            w.add(0, *bigwig.sections_of_sites(b, 0, S, red))
        with pytest.raises(BscError, match="add up"):  # the sizes' sum is not z_bytes
            w.add_z(0, zdata + b"\0", zs, secs, zoom)
        with pytest.raises(BscError, match="add up"):
            w.add_z(0, zdata[:-1], zs, secs, zoom)
        for bad in (0, 24 + 8 * 2 + 12):  # a size of 0; a size above raw + 11
            with pytest.raises(BscError, match="stream of"):
                w.add_z(0, bytes(max(bad, 1)), np.array([bad], np.uint32), secs, zoom)
        with pytest.raises(BscError):  # the summaries' checks are bsc_bigwig_add's: a start below the previous end
            w.add_z(0, *z_block([(25, 1)], 0, S, red))
        with pytest.raises(ValueError):
            w.add_z(0, zdata, zs[:0], secs, zoom)
        assert os.path.getsize(path) == size0
        top = bytes(24 + 8 * 2 + 11)  # raw + 11 is the most a stream may be (the writer does not inflate it)
        w.add_z(0, top, np.array([len(top)], np.uint32), secs, zoom)
        w.finish()
    f = bigwig.read(path)
    assert f.section_count == 3 and f.summary["basesCovered"] == 7
    # the reverse: add_z after add
    path2 = str(tmp_path / "r2.bw")
    with bigwig.Writer(path2, refs, S, red) as w:
        w.add_z(0, b"", np.zeros(0, np.uint32), np.zeros(0, bigwig.BW_SUM), np.zeros(0, bigwig.BW_SUM))  # an empty add of the other kind decides nothing
        w.add(0, *bigwig.sections_of_sites(a, 0, S, red))
        size0 = os.path.getsize(path2)
        with pytest.raises(BscError, match="plain"):
            w.add_z(0, *z_block(b, 0, S, red))
        assert os.path.getsize(path2) == size0
        w.add(0, *bigwig.sections_of_sites(b, 0, S, red))
        w.finish()
    assert open(path2, "rb").read() == R.build(refs, [(0, a), (0, b)], S, red)


# ---- 3. the reader ----------------------------------------------------------------------------------------------------------------------------
def test_reader_on_a_compressed_and_a_plain_file(tmp_path):
    rng = np.random.default_rng(78)
    refs = [("chrB", 200_000), ("chrA", 50_000)]
    sites = {0: sorted(int(v) for v in set(rng.integers(0, 200_000, 6_000).tolist())), 1: sorted(int(v) for v in set(rng.integers(0, 50_000, 900).tolist()))}
    sites = {t: [(s, int(m)) for s, m in zip(v, rng.integers(0, 1001, len(v)))] for t, v in sites.items()}
    blocks = [(0, sites[0][:2500]), (0, sites[0][2500:2501]), (0, sites[0][2501:]), (1, sites[1])]
    got = write_z(str(tmp_path / "q.bw"), refs, blocks, 5, 16)
    Z.check(got, refs, blocks, 5, 16)
    fz, fp = bigwig.BigWig(got), bigwig.BigWig(write_plain(str(tmp_path / "p.bw"), refs, blocks, 5, 16))
    assert fz.header["zoomLevels"] >= 3 and fz.header["uncompressBufSize"] == 32 * 512 and fp.header["uncompressBufSize"] == 0
    same_reading(fz, fp, refs)
    for _ in range(40):
        t = int(rng.integers(0, 2))
        lo = int(rng.integers(0, refs[t][1]))
        hi = lo + int(rng.choice([0, 1, 5, 300, 40_000]))
        want = [(s, s + 1, struct.pack("<f", m / 10.0)) for s, m in sites[t] if lo <= s < hi]
        assert [(s, e, struct.pack("<f", v)) for s, e, v in fz.intervals(refs[t][0], lo, hi)] == want
        assert fz.zoom_records(1, refs[t][0], lo, hi) == fp.zoom_records(1, refs[t][0], lo, hi)
    # a header whose uncompressBufSize is too small for one block: refused where that block is met
    small = bytearray(got)
    struct.pack_into("<I", small, 52, 32 * 512 - 1)
    f = bigwig.BigWig(bytes(small))
    assert f.intervals("chrA") == fp.intervals("chrA")  # (the sections are 64 bytes)
    with pytest.raises(ValueError, match="uncompressBufSize"):
        f.zoom_records(0)
    with pytest.raises(ValueError, match="uncompressBufSize"):
        f.zoom_records(0, "chrB")
    struct.pack_into("<I", small, 52, 24 + 8 * 5 - 1)
    with pytest.raises(ValueError, match="uncompressBufSize"):
        bigwig.BigWig(bytes(small)).intervals("chrA")


# ---- 4. sanitizers, the binary's refusals -------------------------------------------------------------------------------------------------------
def test_compressed_writer_under_sanitizers(tmp_path):
    """make bigwig-z-san: integration/bigwig_z_san.c + csrc/bigwig.c + libz under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "bigwig_z_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "bigwig_z_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "bigwig.c"), "-lpthread", "-lz", "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


def test_bam2bcf_refusals():
    assert os.path.exists(EXE), "run `make demo`"

    def refused(args, word):
        r = subprocess.run([EXE, *args, "in.bam", "ref.fa", "out.bcf", "out.json"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr)

    refused(["--meth-bigwig-compress"], "needs --meth-bigwig")
    refused(["--meth-bigwig-compress", "--meth", "o.bed"], "needs --meth-bigwig")
    refused(["--meth-bigwig", "o.bw", "--meth-bigwig-compress", "--meth-bigwig-section", "8158"], "8157")
    refused(["--meth-bigwig-section", "8158", "--meth-bigwig-compress", "--meth-bigwig", "o.bw"], "8157")
    refused(["--meth-bigwig", "o.bw", "--meth-bigwig-compress", "--rank", "0", "--world", "2"], "--meth-bigwig writes a single run's track")
    refused(["--meth-bigwig", "o.bw", "--meth-bigwig-compress", "--merge", "2"], "--meth-bigwig writes a single run's track")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "--meth-bigwig-compress" in r.stderr
