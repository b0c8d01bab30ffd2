"""The bedMethyl table as bigBed items on the host (csrc/bigbed.c: bsc_bigbed_blocks_recs) against the rule of include/bscall_amd.h in two
independent forms: the lines of bsc_meth_format_rec re-cut here (head, columns 4 .. 15, NUL), and the Python form of the rule
(bs_call_amd/bigbed.py: blocks_of_recs).  The records that attain BSC_BB_ITEM_MIN and BSC_BB_ITEM_MAX, block sizes 1 / 3 / 512, windows that
blocks share, every room one short, the way back to the table's text, and the host form under the address and undefined-behaviour
sanitizers as a stand-alone program.  No GPU."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bs_call_amd as B
from bs_call_amd import _lib, bigbed, methbed
from bs_call_amd.abi import VCF_REC
from methregions_ref import random_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()


def rows(a):
    return [tuple(int(v) for v in r) for r in a]


def recut(recs, chrom_id, par, B_items, red):
    """The rule applied to the table's own lines: contig TAB start TAB end TAB rest NEWLINE -> head + rest + NUL; blocks of B_items; windows."""
    p = _lib.MethParams(**(par or {}))
    items = []
    for r in recs:
        line = methbed.format_rec(r, "chrQ", p)
        if not line:
            continue
        contig, start, end, rest = line.split(b"\t", 3)
        assert contig == b"chrQ" and rest.endswith(b"\n") and int(end) == int(start) + 1
        items.append((int(start), struct.pack("<III", chrom_id, int(start), int(end)) + rest[:-1] + b"\0"))
    return bigbed.blocks_of_items(items, B_items, red)


def same(got, want):
    assert got[0] == want[0]
    assert rows(got[1]) == rows(want[1]) and rows(got[2]) == rows(want[2])


def test_constants_are_the_header_s():
    assert int(re.search(r"#define BSC_BB_ITEM_MAX (\d+)u", HEADER).group(1)) == bigbed.ITEM_MAX == 100
    assert int(re.search(r"#define BSC_BB_ITEM_MIN (\d+)u", HEADER).group(1)) == bigbed.ITEM_MIN == 46
    assert "#define BSC_BB_Z_ITEMS_MAX (0xFF00u / BSC_BB_ITEM_MAX)" in HEADER and bigbed.Z_ITEMS_MAX == 652  # derived, not stated twice
    assert bigbed.BB_SUM.itemsize == 24
    p = _lib.BbParams(0, 0)
    _lib.load().bsc_bb_params_default(p)
    assert (p.items_per_block, p.reduction) == (512, 1024) == (_lib.BbParams().items_per_block, _lib.BbParams().reduction)


@pytest.mark.parametrize("B_items,red", [(1, 1), (3, 7), (512, 1024), (64, 100)])
def test_host_form_equals_the_lines_recut_and_the_python_rule(B_items, red):
    rng = np.random.default_rng(9100 + B_items)
    for x0, n, wide in ((1, 700, True), (999_990, 1300, False), (2**32 - 400, 400, True)):
        recs = random_records(rng, n, x0, wide=wide)
        if not wide:  # called neighbours that are bases, so that every name occurs (random bytes give CHN almost always)
            c = recs["core"]
            c["cx_gt"] = np.ascontiguousarray(rng.choice(list(b"ACGTN"), (n, 5)).astype(np.uint8)).view("S5").reshape(-1)
            recs["core"] = c
            names = {t.split(b"\t")[0] for _, _, _, t in bigbed.items_of_stream(bigbed.blocks_recs_host(recs, 5, {"contexts": 1}, None)[0])}
            assert names == {b"CG", b"CHG", b"CHH", b"CHN"}
        for par in (None, {"contexts": 1}, {"contexts": 1, "min_cov": 3, "min_phred": 20, "pass_only": 1}):
            got = bigbed.blocks_recs_host(recs, 5, par, {"items_per_block": B_items, "reduction": red})
            same(got, recut(recs, 5, par, B_items, red))
            same(got, bigbed.blocks_of_recs(recs, 5, par, B_items, red))
            n_sites = int(got[1]["count"].sum()) if len(got[1]) else 0
            assert n_sites > n // 20 and len(got[1]) == -(-n_sites // B_items) and int(got[2]["count"].sum()) == n_sites
            assert bigbed.ITEM_MIN * n_sites <= len(got[0]) <= bigbed.ITEM_MAX * n_sites
            # and back: the table's text
            assert bigbed.lines_of_stream(got[0], {5: b"chrQ"}) == methbed.format_recs(recs, "chrQ", _lib.MethParams(**(par or {})))


def one(pos, gt, cg, cx, a, b, phred, flt):
    r = np.zeros(1, dtype=VCF_REC)
    c = r["core"]
    c["pos"], c["emit"], c["gt"], c["cg"], c["cx_gt"], c["phred"], c["flt"] = pos, 1, gt, cg, cx, phred, flt
    r["core"] = c
    r["counts"][0, 5 if gt == 4 else 6], r["counts"][0, 7 if gt == 4 else 4] = a, b
    return r


def test_the_records_that_attain_the_shortest_and_the_longest_item():
    lo = one(9, 4, b"C", b"ACGTG", 0, 9, 9, 0)
    got = bigbed.blocks_recs_host(lo, 0, None, None)
    assert len(got[0]) == bigbed.ITEM_MIN and got[0][12:] == b"CG\t9\t+\t8\t9\t0,255,0\t9\t0\t0\t9\t9\tPASS\0"
    # every column at its widest: pos = 2^32 - 1, a three-letter name, a = b ten digits (pct 50: a nine-byte itemRgb), GQ three digits
    hi = one(2**32 - 1, 7, b"H", b"CCGTA", 4_000_000_000, 4_000_000_000, 255, 128)
    got = bigbed.blocks_recs_host(hi, 2**32 - 1, {"contexts": 1}, None)
    assert len(got[0]) == bigbed.ITEM_MAX
    assert got[0] == struct.pack("<III", 2**32 - 1, 2**32 - 2, 2**32 - 1) + b"CHG\t1000\t-\t4294967294\t4294967295\t255,255,0\t8000000000\t50\t4000000000\t4000000000\t255\tmac1\0"
    same(got, bigbed.blocks_of_recs(hi, 2**32 - 1, {"contexts": 1}))
    # pct 100 cannot be longer: its itemRgb has 7 bytes and b at most 8 digits (a >= 199 b)
    full = one(2**32 - 1, 4, b"H", b"ACGTG", 2**32 - 1, 21_582_750, 255, 1)
    got = bigbed.blocks_recs_host(full, 0, {"contexts": 1}, None)
    assert b"\t255,0,0\t" in got[0] and b"\t100\t" in got[0] and len(got[0]) == bigbed.ITEM_MAX - 3
    # under BSC_METH_CPG the name is "CG": one byte less
    cg = one(2**32 - 1, 4, b"C", b"ACGTG", 4_000_000_000, 4_000_000_000, 255, 1)
    assert len(bigbed.blocks_recs_host(cg, 0, None, None)[0]) == bigbed.ITEM_MAX - 1
    # no column can be wider: the extremes of every random field stay inside the bounds
    rng = np.random.default_rng(9200)
    recs = random_records(rng, 3000, 2**32 - 3000, wide=True)
    stream = bigbed.blocks_recs_host(recs, 2**32 - 1, {"contexts": 1}, None)[0]
    lens = [12 + len(t) + 1 for _, _, _, t in bigbed.items_of_stream(stream)]
    assert bigbed.ITEM_MIN <= min(lens) and max(lens) <= bigbed.ITEM_MAX


def test_a_window_two_blocks_share_and_block_borders():
    recs = random_records(np.random.default_rng(9300), 400, 1, wide=True)
    c = recs["core"]
    c["emit"], c["gt"], c["cg"] = 1, 4, b"C"
    recs["core"] = c
    recs["counts"] = np.maximum(recs["counts"], 1)
    data, blk, zoom = bigbed.blocks_recs_host(recs, 0, None, {"items_per_block": 3, "reduction": 100})
    assert rows(zoom) == [(0, 100, 100, 0, 0), (100, 200, 100, 0, 0), (200, 300, 100, 0, 0), (300, 400, 100, 0, 0)]  # 100 sites: 33 blocks and a third
    assert len(blk) == 134 and rows(blk)[-1][:3] == (399, 400, 1) and rows(blk)[33][:3] == (99, 102, 3)  # a block across the window's border
    items = bigbed.items_of_stream(data)
    offs = np.cumsum([0] + [12 + len(t) + 1 for _, _, _, t in items])
    assert [int(b["off"]) for b in blk] == [int(offs[3 * k]) for k in range(134)] and offs[-1] == len(data)


def test_each_room_one_short_and_bad_arguments():
    recs = random_records(np.random.default_rng(9400), 500, 77, wide=True)
    bbp = {"items_per_block": 16, "reduction": 32}
    want = bigbed.blocks_recs_host(recs, 3, None, bbp)
    exact = (len(want[0]), len(want[1]), len(want[2]))
    assert min(exact) > 10
    same(bigbed.blocks_recs_host(recs, 3, None, bbp, room=exact), want)
    for k in range(3):
        with pytest.raises(B.BscError):  # (that nothing was written into any room is checked inside)
            bigbed.blocks_recs_host(recs, 3, None, bbp, room=tuple(v - (1 if j == k else 0) for j, v in enumerate(exact)))
    for bad in ({"items_per_block": 0}, {"items_per_block": 65536}, {"reduction": 0}):
        with pytest.raises(B.BscError):
            bigbed.blocks_recs_host(recs, 3, None, bad)
    with pytest.raises(B.BscError):
        bigbed.blocks_recs_host(recs, 3, {"contexts": 2}, bbp)
    assert bigbed.blocks_recs_host(recs[:0], 3, None, bbp)[0] == b""
    with pytest.raises(ValueError):
        bigbed.items_of_stream(want[0][:-1])


def test_host_form_and_writer_under_sanitizers(tmp_path):
    """make bigbed-san: integration/bigbed_san.c + csrc/bigbed.c + csrc/methbed.c + libz under ASan + UBSan, a program of its own: the host
    form and the file's writer, plain and compressed."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "bigbed_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "bigbed_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "bigbed.c"), os.path.join(ROOT, "bs_call_amd", "csrc", "methbed.c"), "-lz", "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


# ---- the file: bsc_bigbed_open / _add / _add_z / _finish against tests/bigbed_ref.py, the reader, the refusals ---------------------------------
import zlib  # noqa: E402

import bigbed_ref as BR  # noqa: E402


def fake_item(tid, start, k):
    """An item of the rule's shape with a text whose length varies (46 .. 70 bytes)."""
    cov = 10 ** (k % 9)
    return start, struct.pack("<III", tid, start, start + 1) + b"CG\t%d\t+\t%d\t%d\t0,255,0\t%d\t0\t0\t%d\t9\tPASS\0" % (min(cov, 1000), start, start + 1, cov, cov)


def items_at(tid, starts, salt=0):
    return [fake_item(tid, s, k + salt) for k, s in enumerate(starts)]


def write_file(path, refs, adds, B, red, compress=False):
    """The C writer over the adds; the summaries are the Python rule's (blocks_of_items).  Compressed: Python zlib's streams at level 1."""
    with bigbed.Writer(str(path), refs, B, red, compress=compress) as w:
        for tid, items in adds:
            data, blk, zoom = bigbed.blocks_of_items(items, B, red)
            if not compress:
                w.add(tid, data, blk, zoom)
            else:
                offs = [int(b["off"]) for b in blk] + [len(data)]
                zs = [zlib.compress(data[a:b], 1) for a, b in zip(offs, offs[1:])]
                w.add_z(tid, b"".join(zs), [len(z) for z in zs], len(data), blk, zoom)
        w.finish()
    return open(path, "rb").read()


def refs_of(n):
    return [("c%d" % (k * 7919 % 1000) + "x" * (k % 5), 10**9) for k in range(n)]


FILE_CASES = {
    "no block": (1, [], 512, 1024),
    "an add without a site": (2, [(1, [])], 512, 1024),
    "one block": (1, [(0, items_at(0, range(100, 160)))], 512, 1024),
    "256 blocks, B = 1": (2, [(1, items_at(1, range(5, 5 + 256)))], 1, 1024),
    "257 blocks, B = 3, two levels": (2, [(0, items_at(0, range(0, 3 * 257 - 1)))], 3, 1),
    "65 537 blocks": (3, [(0, items_at(0, range(0, 40000))), (2, items_at(2, range(7, 7 + 25537)))], 1, 1024),
    "256 contigs": (256, [(k, items_at(k, range(k, k + 3), k)) for k in range(0, 256, 5)], 512, 1024),
    "257 contigs": (257, [(k, items_at(k, range(k, k + 3), k)) for k in range(0, 257, 4)], 3, 64),
    "300 contigs, every one with sites": (300, [(k, items_at(k, range(1000 * k, 1000 * k + 2), k)) for k in range(300)], 512, 1024),
    "seven levels": (1, [(0, items_at(0, range(0, 1024 * 257, 1024)))], 512, 1),
    "eight levels": (1, [(0, items_at(0, range(0, 4096 * 257, 4096)))], 512, 1),
    "a window two adds share": (2, [(0, items_at(0, [10, 20, 1030])), (0, items_at(0, [1040, 1050, 5000], 3)), (1, items_at(1, [1040]))], 512, 1024),
    "B = 512 with a short last block in every add": (1, [(0, items_at(0, range(0, 1300))), (0, items_at(0, range(2000, 2600), 1))], 512, 100),
}


@pytest.mark.parametrize("case", list(FILE_CASES))
@pytest.mark.parametrize("compress", [False, True])
def test_the_file_equals_the_independent_builder_s(tmp_path, case, compress):
    n_refs, adds, B, red = FILE_CASES[case]
    refs = refs_of(n_refs)
    got = write_file(tmp_path / "t.bb", refs, adds, B, red, compress)
    want = BR.build(refs, adds, B, red, (lambda raw: zlib.compress(raw, 1)) if compress else None)
    assert got == want
    f = bigbed.BigBed(got)
    n_items = sum(len(items) for _, items in adds)
    assert f.item_count == n_items and f.header["fieldCount"] == 15 and f.header["definedFieldCount"] == 9 and f.items_per_slot == B
    assert f.autosql.encode() + b"\n" == BR.AUTOSQL + b"\n" and f.autosql.startswith("table bedMethyl") and "bigint coverage" in f.autosql
    assert f.chrom_count == n_refs and all(f.chrom_lookup(n) == (k, 10**9) for k, (n, _) in enumerate(refs))
    assert f.summary == (dict(basesCovered=n_items, minVal=1.0, maxVal=1.0, sumData=float(n_items), sumSquares=float(n_items)) if n_items else
                         dict(basesCovered=0, minVal=0.0, maxVal=0.0, sumData=0.0, sumSquares=0.0))
    assert (f.header["uncompressBufSize"] != 0) == (compress and n_items > 0)
    if "levels" in case:
        assert len(f.zooms) == {"two": 2, "seven": 7, "eight": 8}[case.split(" levels")[0].split()[-1]]
    if case == "one block":
        assert len(f.zooms) == 1
    assert [(i[0], i[1], i[2]) for i in f.all_items()] == [(tid, s, s + 1) for tid, items in adds for s, _ in items]
    for level in range(len(f.zooms)):
        recs = f.zoom_records(level)
        assert sum(r["validCount"] for r in recs) == n_items and all(r["minVal"] == r["maxVal"] == 1.0 and r["sumData"] == r["validCount"] for r in recs)
    if case == "a window two adds share":
        assert [(r["chromId"], r["start"], r["end"], r["validCount"]) for r in f.zoom_records(0)] == [(0, 10, 21, 2), (0, 1030, 1051, 3), (0, 5000, 5001, 1),
                                                                                                    (1, 1040, 1041, 1)]


@pytest.mark.parametrize("compress", [False, True])
def test_lines_of_the_file_are_the_table(tmp_path, compress):
    rng = np.random.default_rng(9500)
    refs, par, table = [("chrA", 10**6), ("chrB", 10**6), ("chrC", 500)], {"contexts": 1, "min_cov": 2}, []
    path = str(tmp_path / "t.bb")
    with bigbed.Writer(path, refs, 64, 128, compress=compress) as w:
        for tid, x0, n in ((0, 1, 900), (0, 5000, 700), (2, 10, 300)):
            recs = random_records(rng, n, x0, wide=True)
            data, blk, zoom = bigbed.blocks_recs_host(recs, tid, par, {"items_per_block": 64, "reduction": 128})
            table.append(methbed.format_recs(recs, refs[tid][0], _lib.MethParams(**par)))
            if compress:
                offs = [int(b["off"]) for b in blk] + [len(data)]
                zs = [zlib.compress(data[a:b], 1) for a, b in zip(offs, offs[1:])]
                w.add_z(tid, b"".join(zs), [len(z) for z in zs], len(data), blk, zoom)
            else:
                w.add(tid, data, blk, zoom)
        w.finish()
    assert bigbed.lines(path) == b"".join(table) and len(table[0]) > 10000
    f = bigbed.read(path)
    assert f.entries("chrB") == [] and f.entries("nowhere") == [] and len(f.entries("chrC")) == table[2].count(b"\n")


def test_entries_equal_a_linear_scan_at_block_and_node_borders(tmp_path):
    # 600 blocks of 3 items: more than two leaf nodes of 256; starts 10 apart, so a block covers [30 k, 30 k + 21)
    items = items_at(1, range(0, 18000, 10))
    refs = refs_of(3)
    for compress in (False, True):
        f = bigbed.BigBed(write_file(tmp_path / ("e%d.bb" % compress), refs, [(1, items[:900]), (1, items[900:])], 3, 1000, compress))
        name = refs[1][0]
        flat = [(s, s + 1, it[12:-1]) for s, it in items]
        edges = [0, 1, 20, 21, 29, 30, 31, 256 * 30 - 10, 256 * 30 - 9, 256 * 30, 256 * 30 + 1, 512 * 30, 512 * 30 + 21, 8990, 8991, 9000, 17990, 17991, 18500]
        for s in edges:
            for e in (s, s + 1, s + 10, s + 11, s + 31, 256 * 30 + 5, 20000):
                assert f.entries(name, s, e) == [x for x in flat if x[0] < e and s < x[1]], (s, e)
        assert f.entries(name) == flat and f.entries(refs[0][0]) == [] and f.entries(refs[2][0]) == []


def test_every_refusal_leaves_the_file_as_it_was(tmp_path):
    refs = refs_of(3)
    path = str(tmp_path / "r.bb")
    good = items_at(1, range(100, 110))
    data, blk, zoom = bigbed.blocks_of_items(good, 3, 1000)
    with bigbed.Writer(path, refs, 3, 1000) as w:
        w.add(1, data, blk, zoom)
        size = os.path.getsize(path)
        assert size > len(data)

        def refused(tid, d, b, z, word):
            with pytest.raises(B.BscError, match=word):
                w.add(tid, d, b, z)
            assert os.path.getsize(path) == size

        def changed(arr, k, **kv):
            out = arr.copy()
            for f, v in kv.items():
                out[f][k] = v
            return out

        nxt = items_at(1, range(200, 210))
        d2, b2, z2 = bigbed.blocks_of_items(nxt, 3, 1000)
        refused(0, d2, b2, z2, "behind contig")
        refused(3, d2, b2, z2, "contig 3 of 3")
        refused(1, data, blk, zoom, "below the previous end")
        refused(1, d2, changed(b2, 1, count=2), z2, "is not one of 3 sites")
        refused(1, d2, changed(b2, 0, off=1), z2, "not 0")
        refused(1, d2, changed(b2, 2, off=int(b2["off"][1])), z2, "do not ascend")
        refused(1, d2, changed(b2, 1, off=int(b2["off"][0]) + 3 * bigbed.ITEM_MIN - 1), z2, "has .* bytes")  # block 0 below 3 items of the shortest
        refused(1, d2 + bytes(3 * 100), b2, z2, "has .* bytes")  # the last block above its items of the longest
        refused(1, d2[:-1], changed(b2, 3, off=len(d2) - 1), z2, "do not ascend")
        refused(1, d2, b2, changed(z2, 0, count=9), "windows do not hold")
        refused(1, d2, b2, z2[:0], "without a window")
        with pytest.raises(B.BscError, match="compressed|plain"):
            w.add_z(1, b"x" * 40, [10] * 4, len(d2), b2, z2)
        assert os.path.getsize(path) == size
        w.add(1, d2, b2, z2)
        w.add(2, b"", b2[:0], z2[:0])  # an add without a site is no error
        w.finish()
        with pytest.raises(B.BscError, match="finished"):
            w.add(2, d2, b2, z2)
    assert bigbed.BigBed(open(path, "rb").read()).item_count == 20
    # the compressed add's own checks
    pz = str(tmp_path / "z.bb")
    with bigbed.Writer(pz, refs, 3, 1000, compress=True) as w:
        offs = [int(b["off"]) for b in blk] + [len(data)]
        zs = [zlib.compress(data[a:b], 1) for a, b in zip(offs, offs[1:])]
        for sizes, blob, word in (([0] + [len(z) for z in zs[1:]], b"".join(zs[1:]), "stream of 0 bytes"),
                                  ([offs[1] - offs[0] + 12] + [len(z) for z in zs[1:]], bytes(offs[1] - offs[0] + 12) + b"".join(zs[1:]), "stream of"),
                                  ([len(z) for z in zs], b"".join(zs) + b"x", "add up")):
            with pytest.raises(B.BscError, match=word):
                w.add_z(1, blob, sizes, len(data), blk, zoom)
            assert os.path.getsize(pz) == 0
        w.add_z(1, b"".join(zs), [len(z) for z in zs], len(data), blk, zoom)
        with pytest.raises(B.BscError, match="compressed"):
            w.add(1, d2, b2, z2)
        w.finish()
    assert bigbed.lines(pz) == bigbed.lines_of_stream(data, {1: refs[1][0].encode()})
    with pytest.raises(B.BscError, match="at most 652"):
        with bigbed.Writer(str(tmp_path / "big.bb"), refs, 653, 1000, compress=True) as w:
            w.add_z(1, b"".join(zs), [len(z) for z in zs], len(data), blk, zoom)
    for bad in ((0, 1), (65536, 1), (1, 0)):
        with pytest.raises(B.BscError):
            bigbed.Writer(str(tmp_path / "bad.bb"), refs, *bad)
    with pytest.raises(ValueError):
        bigbed.BigBed(open(pz, "rb").read()[:-4] + b"\0\0\0\0")


def test_bam2bcf_refusals_that_need_no_device():
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    assert os.path.exists(exe), "run `make demo`"

    def refused(args, word, env=None):
        r = subprocess.run([exe, *args, "in.bam", "ref.fa", "out.bcf", "out.json"], capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, **(env or {})))
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr)

    refused(["--meth-bigbed-compress"], "needs --meth-bigbed")
    refused(["--meth-bigbed", "o.bb", "--meth-bigbed-items", "0"], "1 .. 65535")
    refused(["--meth-bigbed", "o.bb", "--meth-bigbed-items", "65536"], "1 .. 65535")
    refused(["--meth-bigbed", "o.bb", "--meth-bigbed-zoom", "0"], "1 or more")
    refused(["--meth-bigbed", "o.bb", "--meth-bigbed-zoom", "-3"], "1 or more")
    refused(["--meth-bigbed-items", "653", "--meth-bigbed-compress", "--meth-bigbed", "o.bb"], "652")
    refused(["--meth-bigbed", "o.bb", "--rank", "0", "--world", "2"], "--meth-bigbed writes a single run's file")
    refused(["--meth-bigbed", "o.bb", "--meth-bigbed-compress", "--merge", "2"], "--meth-bigbed writes a single run's file")
    for var in ("BAM2BCF_HOST_READER", "BAM2BCF_HOST_BCF", "BAM2BCF_HOST_PREP"):
        refused(["--meth-bigbed", "o.bb"], "not with BAM2BCF_HOST_READER", {var: "1"})
    assert not os.path.exists("o.bb")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert "--meth-bigbed-compress" in r.stderr and "--meth-bigbed-items" in r.stderr
