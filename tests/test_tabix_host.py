"""The index of the compressed methylation tables without a GPU: bsc_tbx_add / bsc_tbx_finish fed with entries computed in Python (the run
rule of tests/tabix_ref.py, cut at random line starts and across several adds, as the device scan's intervals and the blocks cut them)
against tests/tabix_ref.py's .tbi / .csi of the same table; every refusal; methbed.read_index / reg2bins / fetch against a linear scan; the
host form of the device scan (bsc_bed_entries_host) against the Python run rule over whole and damaged streams; writer and host scan as
a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer; the tool's refusals."""
import atexit
import ctypes as C
import gzip
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import tabix_ref as R
from bs_call_amd import _lib, methbed
from bs_call_amd.caller import BED_ENTRY, TBX_CSI, TBX_TBI, BscError, TabixIndex, bed_entries_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 0xFF00
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _text(name, spans, pad=None):
    """A contig's lines from (start, end) pairs; pad: {line number: bytes of the fourth column}."""
    return b"".join(b"%s\t%d\t%d\t%s\t7\n" % (name.encode(), a, b, (pad or {}).get(i, b"x")) for i, (a, b) in enumerate(spans))


def _spans(rng, length, n, widths, min_shift=14, straddle=(8, 64, 512, 4096, 32768)):
    """Sorted (start, end) pairs: random ones of the given widths, pairs around every window border of `straddle` multiples — one line
    that ends at the border, one across it (wl a multiple of 8, 64, ...), one that begins at it — and gaps of many empty windows."""
    out = []
    for s in rng.integers(0, max(length - max(widths), 1), n):
        w = int(rng.choice(widths))
        out.append((int(s), min(int(s) + w, length)))
    for m in straddle:
        b = m << min_shift
        if b + 2 <= length:
            out += [(b - 2, b), (b - 1, b + 1), (b, b + 2)] if 2 in widths or len(widths) > 1 else [(b - 1, b), (b, b + 1)]
    return sorted(out)


def _scenarios():
    rng = np.random.default_rng(20261020)
    S = {}
    S["none"] = ([], {})
    S["span1"] = ([("chr1", 1 << 29)], {"chr1": _spans(rng, 1 << 29, 400, [1])})
    S["span2"] = ([("a", 1 << 28), ("b", 1 << 20)], {"a": _spans(rng, 1 << 28, 300, [2]), "b": _spans(rng, 1 << 20, 200, [2])})
    many = [("c%03d" % i, 100_000 + 977 * i) for i in range(300)]
    lines = {}
    for i, (n, ln) in enumerate(many):
        if i not in (0, 150, 151, 299) and i % 7 != 3:  # a contig without lines first, in the middle (two in a row) and last
            lines[n] = _spans(rng, ln, 12, [1, 2, 500, 40_000])
    S["many"] = (many, lines)
    S["dense"] = ([("d", 200_000)], {"d": _spans(rng, 200_000, 3000, [1, 2])})  # long runs: cut by the intervals and by the adds
    # mixed spans up to 40 000 bases, a leaf bin cut in two by a straddler: lines in window 4, a long line across the border 5, then
    # a one-base line still in window 4 (the starts do not descend)
    B = 5 << 14
    cut = [(B - 300, B - 299), (B - 200, B - 198), (B - 100, B + 700), (B - 50, B - 49), (B - 1, B), (B, B + 1)]
    S["mixed"] = ([("m", 1 << 29), ("empty", 10), ("n", 3 << 20)],
                  {"m": sorted(_spans(rng, 1 << 29, 500, [1, 2, 17, 16_384, 40_000]) + cut), "n": _spans(rng, 3 << 20, 100, [1, 2, 40_000])})
    return S


SCN = _scenarios()
KINDS = [("tbi", 14), ("csi", 14), ("csi", 10)]


def _table(scn, kind_shift=14, pad_to=None, line_at=None):
    """(data, [(tid, contig text)]) of a scenario; line_at: pad the first line so that the SECOND begins at that offset; pad_to: pad the
    last line so that the table has that many bytes."""
    names, lines = SCN[scn]
    per = []
    for tid, (n, ln) in enumerate(names):
        sp = lines.get(n, [])
        if kind_shift != 14 and sp:  # the straddlers of this min_shift too
            sp = sorted(sp + [(b - 1, b + 1) for m in (8, 64, 512, 4096, 32768) for b in [m << kind_shift] if b + 1 <= ln])
        if sp:
            per.append((tid, n, sp))

    def render(last_pad):
        blocks = []
        for k, (tid, n, sp) in enumerate(per):
            pad = {}
            if k == 0 and line_at is not None:
                pad[0] = b"x" * (line_at - len(_text(n, sp[:1])) + 1)
            if k == len(per) - 1 and last_pad:
                pad[len(sp) - 1] = b"x" * (1 + last_pad)
            blocks.append((tid, _text(n, sp, pad)))
        return blocks

    blocks = render(0)
    if pad_to is not None:
        blocks = render(pad_to - sum(len(t) for _, t in blocks))
        assert sum(len(t) for _, t in blocks) == pad_to
    return b"".join(t for _, t in blocks), blocks


def _feed(ix, blocks, min_shift, rng, stats=None):
    """Every contig's table in one to three adds cut at line starts, each add's entries cut at random line starts."""
    for tid, t in blocks:
        starts = [l[3] for l in R.lines_of(t)]
        cuts = sorted(set(int(v) for v in rng.choice(starts, min(len(starts), 2), replace=False)) - {0})
        for a, b in zip([0] + cuts, cuts + [len(t)]):
            piece = t[a:b]
            ps = [l[3] for l in R.lines_of(piece)]
            sync = [int(v) for v in rng.choice(ps, min(len(ps), 9), replace=False)]
            whole = R.runs_of(piece, min_shift)
            inside = [ps[ps.index(e[4]) + 1] for e in whole if e[2] > 1]  # the second line of a run: a border there cuts the run
            ent = R.runs_of(piece, min_shift, sync=sync + inside[:3])
            if stats is not None:
                stats["pieces"] += len(ent) - len(R.runs_of(piece, min_shift))
                stats["adds"] += 1
            ix.add(tid, np.array(ent, dtype=BED_ENTRY), len(piece))


def _index(kind, min_shift, names, data, blocks, sizes, seed=3, stats=None):
    with TabixIndex(None, TBX_TBI if kind == "tbi" else TBX_CSI, names, min_shift, 0) as ix:
        _feed(ix, blocks, min_shift, np.random.default_rng(seed), stats)
        ix.members(sizes)
        return ix.finish()


def _fake_sizes(n_bytes, rng):
    return [int(v) for v in rng.integers(28, 0x10000, (n_bytes + M - 1) // M)]


@pytest.mark.parametrize("kind,min_shift", KINDS)
@pytest.mark.parametrize("scn", list(SCN))
def test_finish_equals_the_python_index(scn, kind, min_shift):
    names = SCN[scn][0]
    data, blocks = _table(scn, min_shift)
    assert b"".join(t for _, t in blocks) == data
    sizes = _fake_sizes(len(data), np.random.default_rng(5))
    stats = {"pieces": 0, "adds": 0}
    got = _index(kind, min_shift, names, data, blocks, sizes, stats=stats)
    assert got.endswith(EOF)
    want = R.build(kind, data, sizes, [n for n, _ in names], [l for _, l in names], min_shift)
    assert gzip.decompress(got) == want
    if data:
        assert stats["adds"] > len(blocks)  # contigs did come in several adds
    if scn in ("dense", "mixed", "many"):
        assert stats["pieces"] > 0  # runs did continue across intervals
    if len(want) > M:  # the index itself spans more than one member: stored members of 0xFF00 bytes
        assert struct.unpack_from("<H", got, 16)[0] + 1 == M + 31


def test_the_scenarios_hold_what_they_are_for():
    ix = methbed_index_of("mixed", "tbi")
    leaf4 = 4681 + 4
    assert len(ix["refs"][0]["bins"][leaf4]) >= 2  # a leaf bin cut in two by a straddler
    assert any(len(ch) > 1 for k, ch in ix["refs"][0]["bins"].items() if k < 4681)  # a parent bin with several chunks
    for m, level0 in ((8, 585), (64, 73), (512, 9), (4096, 1)):  # the straddler at wl = m lies in a bin of the level above m's
        sp = SCN["mixed"][1]["m"]
        assert ((m << 14) - 1, (m << 14) + 1) in sp
        assert R.bin_of(m - 1, m, 5) < level0
    io = ix["refs"][0]["ioff"]
    assert len(io) == 1 + max((e - 1) >> 14 for _, e in SCN["mixed"][1]["m"])
    assert any(io[w] == io[w + 1] == io[w + 2] for w in range(len(io) - 2))  # gaps of several windows: the backward fill
    assert ix["refs"][1] == {"bins": {}, "loff": {}, "ioff": [], "n_lines": 0}
    many = methbed_index_of("many", "csi")
    assert [i for i, r in enumerate(many["refs"]) if not r["n_lines"]][:1] == [0] and not many["refs"][150]["n_lines"] and not many["refs"][299]["n_lines"]
    assert len(many["names"]) == 300


_IX = {}


def methbed_index_of(scn, kind, min_shift=14):
    key = (scn, kind, min_shift)
    if key not in _IX:
        import tempfile

        names = SCN[scn][0]
        data, blocks = _table(scn, min_shift)
        blob, sizes = R.bgzf(data)
        d = tempfile.mkdtemp(prefix="tabix_host_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        p = os.path.join(d, "t.bed.gz")
        open(p, "wb").write(blob)
        open(p + "." + kind, "wb").write(_index(kind, min_shift, names, data, blocks, sizes))
        ix = methbed.read_index(p + "." + kind)
        ix["_path"], ix["_data"] = p, data
        _IX[key] = ix
    return _IX[key]


@pytest.mark.parametrize("edge", ["line_at_member", "size-1", "size", "size+1"])
@pytest.mark.parametrize("kind", ["tbi", "csi"])
def test_member_borders(kind, edge):
    names = SCN["span2"][0]
    if edge == "line_at_member":
        data, blocks = _table("span2", line_at=M)
        assert R.lines_of(data)[1][3] == M  # a line that begins exactly at a multiple of 0xFF00
    else:
        SCN["one"] = ([("a", 1 << 28)], {"a": SCN["span2"][1]["a"][:40]})
        names = SCN["one"][0]
        data, blocks = _table("one", pad_to=M + {"size-1": -1, "size": 0, "size+1": 1}[edge])
    blob, sizes = R.bgzf(data)
    got = _index(kind, 14, names, data, blocks, sizes)
    assert gzip.decompress(got) == R.build(kind, data, sizes, [n for n, _ in names], [l for _, l in names], 14)
    assert len(sizes) == (len(data) + M - 1) // M


def test_a_contig_of_2_29_plus_1_bases():
    names = [("big", (1 << 29) + 1)]
    with pytest.raises(BscError) as ei:
        TabixIndex(None, TBX_TBI, names, 14, 0)
    assert "csi" in str(ei.value)
    TabixIndex(None, TBX_TBI, [("ok", 1 << 29)], 14, 0).close()
    t = _text("big", [(5, 6), ((1 << 29) - 1, (1 << 29) + 1)])  # wl = 32768: a straddler at the top level's border
    sizes = [100]
    with TabixIndex(None, TBX_CSI, names, 14, 0) as ix:
        ix.add(0, np.array(R.runs_of(t, 14), dtype=BED_ENTRY), len(t))
        ix.members(sizes)
        raw = gzip.decompress(ix.finish())
    assert struct.unpack_from("<ii", raw, 4) == (14, 6)
    assert raw == R.build("csi", t, sizes, ["big"], [(1 << 29) + 1], 14)
    with pytest.raises(BscError):
        TabixIndex(None, TBX_TBI, [("ok", 100)], 10, 0)  # a .tbi is min_shift 14


def test_refusals_leave_the_index_as_it_was():
    L = _lib.load()
    names = [("a", 1 << 20), ("b", 1 << 20), ("c", 1 << 20)]
    good = [(0, [(0, 0, 2, 0, 0), (0, 1, 1, 0, 40), (1, 1, 3, 0, 60)], 100), (1, [(3, 3, 1, 0, 0)], 30), (1, [(3, 3, 2, 0, 0), (9, 9, 1, 0, 10)], 50)]
    bad = [(0, [(0, 0, 1, 0, 0)], 20),  # a descending tid
           (1, [(2, 2, 1, 0, 0)], 20),  # within a contig, a win_beg below the last one
           (1, [(9, 9, 1, 0, 5)], 20), (1, [(9, 9, 1, 0, 0), (9, 10, 1, 0, 0)], 20), (1, [(9, 9, 1, 0, 0), (10, 10, 1, 0, 20)], 20),  # u_beg
           (1, [(9, 9, 0, 0, 0)], 20),  # an entry without lines
           (1, [(10, 9, 1, 0, 0)], 20),  # win_last < win_beg
           (1, [(9, 1 << 15, 1, 0, 0)], 20), (1, [(1 << 15, 1 << 15, 1, 0, 0)], 20),  # a bin out of range
           (1, [], 20), (1, [(9, 9, 1, 0, 0)], 0), (3, [(9, 9, 1, 0, 0)], 20), (-1, [(9, 9, 1, 0, 0)], 20)]

    def run(with_bad):
        with TabixIndex(None, TBX_TBI, names, 14, 0) as ix:
            for g in good:
                ix.add(g[0], np.array(g[1], dtype=BED_ENTRY), g[2])
            for b in bad if with_bad else []:
                with pytest.raises(BscError) as ei:
                    ix.add(b[0], np.array(b[1], dtype=BED_ENTRY).reshape(-1), b[2])
                assert ei.value.code == -1, b
            with pytest.raises(BscError) as ei:
                ix.finish()
            assert "not closed yet" in str(ei.value)
            ix.members([77])
            with pytest.raises(BscError):
                ix.add(2, np.array([(0, 0, 1, 0, 0)], dtype=BED_ENTRY), 10)
            return ix.finish()

    plain = run(False)
    assert run(True) == plain
    raw = gzip.decompress(plain)
    want = (b"TBI\x01" + struct.pack("<8i", 3, 0x10000, 1, 2, 3, ord("#"), 0, 6) + b"a\0b\0c\0"
            + struct.pack("<i", 4) + struct.pack("<IiQQ", 585, 1, 40, 60) + struct.pack("<IiQQ", 4681, 1, 0, 40) + struct.pack("<IiQQ", 4682, 1, 60, 100)
            + struct.pack("<IiQQQQ", 37450, 2, 0, 100, 6, 0) + struct.pack("<iQQ", 2, 0, 40)
            + struct.pack("<i", 3) + struct.pack("<IiQQ", 4684, 1, 100, 140) + struct.pack("<IiQQ", 4690, 1, 140, 180) + struct.pack("<IiQQQQ", 37450, 2, 100, 180, 4, 0)
            + struct.pack("<i", 10) + struct.pack("<10Q", *([100] * 4 + [140] * 6)) + struct.pack("<ii", 0, 0) + struct.pack("<Q", 0))
    assert raw == want
    h = C.c_void_p()
    nm, ln = (C.c_char_p * 1)(b"a"), (C.c_uint32 * 1)(100)
    assert L.bsc_tbx_open(None, 0, 14, 1, nm, ln, C.byref(h)) == -1 and b"not an open BGZF writer" in L.bsc_last_error()
    assert L.bsc_tbx_open_detached(2, 14, 1, nm, ln, 0, C.byref(h)) == -1 and L.bsc_tbx_open_detached(1, 0, 1, nm, ln, 0, C.byref(h)) == -1
    assert L.bsc_tbx_open_detached(1, 14, 1, None, ln, 0, C.byref(h)) == -1 and L.bsc_tbx_open_detached(1, 14, 1, nm, ln, 0, None) == -1
    assert L.bsc_tbx_add(None, 0, None, 0, 0) == -1 and L.bsc_tbx_finish(None, None, 0) == -1 and L.bsc_tbx_members(None, None, 0) == -1
    L.bsc_tbx_close(None)
    assert L.bsc_tbx_open_detached(1, 14, 1, nm, ln, 0, C.byref(h)) == 0
    assert L.bsc_tbx_members(h, None, 0) == 0
    need = L.bsc_tbx_finish(h, None, 0)
    buf = np.full(need + 8, 0xEE, np.uint8)
    assert L.bsc_tbx_finish(h, None, 5) == -1
    assert L.bsc_tbx_finish(h, buf.ctypes.data_as(C.c_void_p), need - 1) == need and (buf == 0xEE).all()  # too small: nothing written
    assert L.bsc_tbx_finish(h, buf.ctypes.data_as(C.c_void_p), need) == need and (buf[need:] == 0xEE).all()
    L.bsc_tbx_close(h)
    assert L.bsc_tbx_finish(h, None, 0) == -1  # a closed index


# ---- region queries ---------------------------------------------------------------------------------------------------------------------
def test_reg2bins():
    assert methbed.reg2bins(0, 1) == [0, 1, 9, 73, 585, 4681] and methbed.reg2bins(5, 5) == []
    assert methbed.reg2bins((1 << 14) - 1, (1 << 14) + 1, 14, 1) == [0, 1, 2]
    assert methbed.reg2bins(0, 1 << 20, 14, 2) == [0] + list(range(1, 9)) + list(range(9, 73))


@pytest.mark.parametrize("kind,min_shift", KINDS)
def test_fetch_equals_the_linear_scan(kind, min_shift):
    ix = methbed_index_of("mixed", kind, min_shift)
    path, data = ix["_path"], ix["_data"]
    rng = np.random.default_rng(11)
    names = SCN["mixed"][0]
    B, G = 5 << 14, None
    io = methbed_index_of("mixed", "tbi")["refs"][0]["ioff"]
    G = next(w for w in range(len(io) - 2) if io[w] == io[w + 1] == io[w + 2]) + 1  # a window inside a gap
    qs = [("m", B - 1, B), ("m", B, B + 1), ("m", B - 1, B + 1), ("m", G << 14, (G << 14) + 100), ("m", 0, 1 << 29), ("n", 0, 3 << 20), ("empty", 0, 10),
          ("nope", 0, 10), ("m", 7, 7), ("m", 9, 3), ("m", (1 << 29) - 1, 1 << 29), ("m", 1 << 29, (1 << 29) + 5)]
    for _ in range(220):
        n, ln = names[int(rng.choice([0, 0, 2]))]
        a = int(rng.integers(0, ln + 10))
        qs.append((n, a, a + int(rng.choice([1, 2, 50, 1000, 1 << 14, 1 << 20, ln]))))
    for m in (8, 64, 512, 4096):
        b = m << min_shift
        qs += [("m", b - 1, b), ("m", b, b + 1)]
    ls = R.lines_of(data)
    for k in rng.choice(len(ls), 60, replace=False):  # single bases at both ends of a line, and the base before it
        c, st, en = ls[int(k)][0].decode(), ls[int(k)][1], ls[int(k)][2]
        qs += [(c, st, st + 1), (c, en - 1, en), (c, max(st - 1, 0), st), (c, en, en + 1)]
    hits = 0
    for n, a, b in qs:
        got = methbed.fetch(path, n, a, b, index_path=ix)
        assert got == R.linear(data, n, a, b), (n, a, b)
        hits += bool(got)
    assert hits > 100
    assert methbed.fetch(path, 2, 0, 3 << 20) == R.linear(data, "n", 0, 3 << 20)  # by contig number, the index found beside the table
    # a query reads its chunks, not the file
    ch = methbed.index_chunks(ix, 0, B, B + 10)
    with open(path, "rb") as f:
        assert ch and sum(len(methbed._read_chunk(f, b, e)) for b, e in ch) < len(data) // 4


# ---- the host form of the scan -----------------------------------------------------------------------------------------------------------
def _as_tuples(ent):
    return [tuple(int(v) for v in e) for e in ent]


def test_host_scan_equals_the_run_rule():
    rng = np.random.default_rng(8)
    for scn, tid in (("mixed", 0), ("span2", 0), ("span1", 0)):
        t = _table(scn)[1][tid][1]
        starts = [l[3] for l in R.lines_of(t)]
        for ms in (0, 4, 10, 14, 31):
            want = R.runs_of(t, ms)
            ent, n, lines, err = bed_entries_host(t, None, ms)
            assert (_as_tuples(ent), n, lines, err) == (want, len(want), len(starts), 0)
            every = starts + [len(t)]
            want = R.runs_of(t, ms, sync=every)
            ent, n, lines, err = bed_entries_host(t, every, ms)
            assert (_as_tuples(ent), n, lines, err) == (want, len(starts), len(starts), 0)
            cuts = sorted(int(v) for v in rng.choice(starts[1:], 20, replace=False))
            sync = [0, 0, 0] + cuts[:10] + cuts[9:10] * 2 + cuts[10:] + [len(t)] * 3  # empty intervals first, in the middle and last
            want = R.runs_of(t, ms, sync=sync)
            ent, n, lines, err = bed_entries_host(t, sync, ms)
            assert (_as_tuples(ent), n, lines, err) == (want, len(want), len(starts), 0)
        want = R.runs_of(t, 14)
        ent, n, lines, err = bed_entries_host(t, None, 14, cap_entries=len(want) - 1)  # one short: the count still comes back
        assert (_as_tuples(ent), n, lines, err) == (want[:-1], len(want), len(starts), 0)
    assert bed_entries_host(b"", None, 14)[1:] == (0, 0, 0) and bed_entries_host(b"", [0, 0], 14)[1:] == (0, 0, 0)
    # the limits of the columns
    ok = b"c\t0\t1\n" + b"c\t4294967295\t4294967296\tx\n"
    assert _as_tuples(bed_entries_host(ok, None, 14)[0]) == [(0, 0, 1, 0, 0), (262143, 262143, 1, 0, 6)] and bed_entries_host(ok, None, 14)[3] == 0
    wide = b"c\t0\t4294967296\n"
    assert _as_tuples(bed_entries_host(wide, None, 31)[0]) == [(0, 1, 1, 0, 0)]


def test_host_scan_of_damaged_streams():
    good = _text("c", [(10, 12), (20, 22), (16_383, 16_385), (16_390, 16_392)])
    second = len(_text("c", [(10, 12)]))
    whole, less = R.runs_of(good, 14), R.runs_of(good[: good.rindex(b"\n", 0, -1) + 1], 14)
    for bad, err, want in ((good[:-1], 1, less), (good + b"c\t30", 1, whole), (good + b"c", 1, whole), (good + b"c\t16400\t164", 1, whole),  # ends inside a line
                           (good + b"c\t5\t7\n", 2, whole),  # a start below the one before it
                           (good + b"c 16400 16402\n", 4, whole), (good + b"c\tx\t9\n", 4, whole), (good + b"c\t16400\n", 4, whole),
                           (good + b"c\t16400\t16400\n" + good, 4, whole), (good + b"c\t16400\t16399\n", 4, whole),
                           (good + b"c\t16400\t4294967297\n", 4, whole), (good + b"c\t00000016400\t16402\n", 4, whole),
                           (good + b"c\t16400\t-1\n", 4, whole), (good + b"\n", 4, whole), (good + b"c\t16400\t16402x\n", 4, whole)):
        ent, n, lines, e = bed_entries_host(bad, None, 14)
        assert e == err, (bad[-30:], e)
        assert _as_tuples(ent) == want and n == len(want) and lines == sum(w[2] for w in want), bad[-30:]
    assert bed_entries_host(good, [0, second + 3, len(good)], 14)[3] & 1  # a line that leaves its interval (the next one then begins inside a line)
    assert bed_entries_host(good, [0, len(good), second, len(good)], 14)[3] & 8 and bed_entries_host(good, [0, len(good) + 1], 14)[3] == 8
    ent, n, lines, e = bed_entries_host(good + b"c\t5\t7\n" + good, [0, len(good) + 6, 2 * len(good) + 6], 14)
    assert e == 2 and lines == 8  # the walk of THAT interval stops; the next one is walked
    with pytest.raises(BscError):
        bed_entries_host(good, None, 32)


def test_writer_and_host_scan_under_sanitizers(tmp_path):
    """make tabix-san: integration/tabix_san.c + csrc/tabix.c under ASan + UBSan, a program of its own (no sanitizer runs inside Python)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "tabix_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "tabix_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "tabix.c"), "-lpthread", "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


def test_bam2bcf_refuses_meth_index_without_a_compressed_single_run(tmp_path):
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    assert os.path.exists(exe), "run `make demo`"
    args = ["in.bam", "ref.fa", str(tmp_path / "o.bcf"), str(tmp_path / "o.json")]
    mp = str(tmp_path / "t.bed.gz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("BAM2BCF_HOST")}
    for opts, extra, word in ((["--meth-index", "tbi"], {}, "--meth "), (["--meth", mp, "--meth-index", "tbi"], {}, "-O b or --meth-bgzf"),
                              (["--meth", mp, "-O", "u", "--meth-index", "csi"], {}, "--meth-bgzf"), (["--meth", mp, "--meth-bgzf", "--meth-index", "bai"], {}, "tbi or csi"),
                              (["--meth-bgzf"], {}, "--meth "), (["--meth", mp, "--meth-bgzf", "--meth-index", "tbi", "--rank", "0", "--world", "2"], {}, "--rank"),
                              (["--meth", mp, "-O", "b", "--meth-index", "tbi", "--merge", "2"], {}, "--merge"),
                              (["--meth", mp, "--meth-bgzf", "--meth-index", "csi"], {"BAM2BCF_HOST_READER": "1"}, "BAM2BCF_HOST_READER"),
                              (["--meth", mp, "--meth-bgzf", "--meth-index", "csi"], {"BAM2BCF_HOST_BCF": "1"}, "BAM2BCF_HOST")):
        p = subprocess.run([exe] + opts + args, capture_output=True, text=True, timeout=60, env=dict(env, **extra))
        assert p.returncode == 2 and word in p.stderr and p.stderr.count("\n") == 1, (opts, p.stderr)
        assert not os.path.exists(tmp_path / "o.bcf") and not os.path.exists(mp + ".tbi") and not os.path.exists(mp + ".csi")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert "[--meth-bgzf] [--meth-index tbi|csi]" in p.stderr
