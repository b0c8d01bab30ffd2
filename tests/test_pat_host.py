"""The per-read CpG pattern table (PAT) on the host: csrc/pat.c (bsc_pat_recs_host, bsc_pat_format, bsc_pat_count_sites) against the Python form
of the rule (bs_call_amd/pat.py) and the hand tallies of tests/pat_cases.py, record for record, total for total and byte for byte; the
formatter at its extremes; the site count; the per-CpG counts the table implies against the read-level CpG table of the same block; and the
host form under the address and undefined-behaviour sanitizers as a stand-alone program (integration/pat_san.c).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pat_cases as P
from bs_call_amd import _lib, pat
from bs_call_amd.caller import BscError, cpg_reads_sites_host, pat_count_sites, pat_format_host, pat_recs_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()


def both(b, cap=None, index_base=0):
    """The block through the Python rule and the host form; asserts they agree on records, totals and bytes; returns (records, totals)."""
    want, wtot = pat.patterns(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    got, n, tot = pat_recs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"], cap=cap)
    assert n == len(want) and tot == wtot, (b["name"], n, len(want), tot, wtot)
    assert got.tobytes() == pat.pack(want)[: len(got)].tobytes() and pat.unpack(got) == want[: len(got)], b["name"]
    if cap is None:
        assert pat_format_host("chrP", index_base, got, b["params"]) == pat.format("chrP", index_base, want, b["params"]), b["name"]
    return want, wtot


def test_the_header_states_the_rule():
    for word in ("ORDINAL", "PATTERN(t)", "PIECES", "BSC_PAT_MAX_SITES", "WGBSTOOLS-UNPINNED", "bsc_pat_rec", "bsc_pat_params", "bsc_pat_count_sites",
                 "bsc_pat_recs_host", "bsc_pat_format", "bsc_pat_device", "bsc_pat_text_device", "bsc_block_pat_kept", "bsc_pat_stream_read",
                 "bsc_pat_stream_detach"):
        assert word in HEADER, word
    assert C.sizeof(_lib.PatParams) == 8 and pat.REC.itemsize == 24 and pat.MAX_SITES == 64
    p = _lib.PatParams(9, 9)
    _lib.load().bsc_pat_params_default(C.byref(p))
    assert (p.min_sites, p.reserved) == (1, 0)


def test_a_block_worked_by_hand():
    """tests/pat_cases.py: hand_block's docstring has the tally, template by template."""
    b = P.hand_block()
    assert tuple(pat.site_positions(b["x"], b["y"], b["ref"])) == P.HAND_SITES
    recs, tot = both(b, index_base=P.HAND_INDEX_BASE)
    assert recs == P.HAND_RECORDS and tot == P.HAND_TOTALS
    assert pat.format("chrP", P.HAND_INDEX_BASE, recs) == (P.HAND_TABLE, 8) == pat_format_host("chrP", P.HAND_INDEX_BASE, pat.pack(recs))
    recs3, tot3 = both(dict(b, params={"min_sites": 3}), index_base=P.HAND_INDEX_BASE)
    assert recs3 == P.HAND_RECORDS_3 and tot3 == P.HAND_TOTALS_3
    assert pat.format("chrP", P.HAND_INDEX_BASE, recs3) == (P.HAND_TABLE_3, 4) == pat_format_host("chrP", P.HAND_INDEX_BASE, pat.pack(recs3))
    assert both(dict(b, params={"min_sites": 0})) == (recs, tot)  # max(1, min_sites)
    assert both(dict(b, params={"min_sites": 8}))[1] == (0, 0, 0, 0, 0, 0, 0, 7)
    # the order is that of `LC_ALL=C sort -k2,2n -k3,3` on the lines
    lines = pat.read_pat(P.HAND_TABLE)
    assert lines == sorted(lines, key=lambda r: (r[1], r[2].encode())) and [(i - 101, s, n) for _, i, s, n in lines] == recs
    # the record's bits: site j in bits 127 - 2 j and 126 - 2 j of hi:lo, codes 1 '.', 2 'C', 3 'T'
    r = pat.pack([(0, "C.T", 1)])[0]
    assert (int(r["hi"]), int(r["lo"])) == (0b100111 << 58, 0)


@pytest.mark.parametrize("b,want", P.cut_blocks(), ids=lambda v: v["name"] if isinstance(v, dict) else "")
def test_templates_cut_at_64_sites(b, want):
    recs, tot = both(b)
    assert recs == want, b["name"]
    if b["name"].startswith("spans"):
        assert tot[:3] == (11, 11, 6) and tot[5] == 0 and tot[6] == 4  # 64 -> 1 piece, 65 -> 2, 128 -> 2, 129 -> 3, 64 -> 1, 65 -> 2; four are cut
    if b["name"].startswith("a piece of dots"):
        assert tot[:3] == (5, 5, 2) and tot[6] == 2
    if b["name"] == "seams":
        assert tot[6] == 2 and tot[0] == len(want) == 11 and tot[1] == 12


@pytest.mark.parametrize("b", P.placement_blocks() + P.long_read_blocks() + [P.identical_block(), P.sixteen_block(), P.distinct_block(300)],
                         ids=lambda b: "%s, min_sites %d" % (b["name"], b["params"]["min_sites"]))
def test_host_form_equals_the_python_rule_on_the_targeted_blocks(b):
    recs, tot = both(b)
    assert tot[0] == len(recs) and tot[1] == sum(n for _, _, n in recs)
    name = b["name"]
    if name == "contention, one code":
        assert recs == [(0, "CTCT", 5000)] and tot == (1, 5000, 5000, 10000, 10000, 0, 0, 4)
    if name == "contention, 16 codes":
        assert len(recs) == 16 and {i for i, _, _ in recs} == {0} and sorted(n for _, _, n in recs) == [312] * 8 + [313] * 8
    if name == "300 distinct":
        assert len(recs) == 300 and all(n == 1 for _, _, n in recs)
    if name == "long read" and tot[7] == 2500:
        if b["params"]["min_sites"] == 1:
            assert tot[2] == 3 and tot[6] == 3 and tot[1] == 120  # three reads of 40 pieces
        else:
            assert tot[2] < 3  # min_sites is judged on the template: 2 490 states of 2 500 sites
    if name == "mates" and tot[7] == 4:  # the epiallele table's
        assert (0, "CTCC", 1) in recs and (0, "C.CC", 1) in recs  # read 0 decides in the overlap; 1020 lies in a gap


@pytest.mark.parametrize("n_pos,seed", P.TILE_EDGE_BLOCKS)
def test_host_form_equals_the_python_rule_around_a_tile(n_pos, seed):
    b = P.dense_block(seed, n_pos, 60)
    _, tot = both(b)
    assert tot[1] > 0, "the seed must give a pattern by the host form alone"
    both(dict(b, params={"min_sites": 4}))


@pytest.fixture(scope="module")
def big():
    b = P.big_block()
    recs, n, tot = pat_recs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, b["params"])
    assert n >= 1000, "the seed must give 1 000 records by the host form alone"
    return b, recs, tot


def test_host_form_equals_the_python_rule_on_20003_positions(big):
    b, recs, tot = big
    want, wtot = both(b)
    assert pat.pack(want).tobytes() == recs.tobytes() and wtot == tot
    assert all(v > 0 for v in tot[:6]) and tot[2] < len(b["tpl"])
    both(dict(b, params={"min_sites": 5}))
    # the room rule: records beyond cap are counted, not stored
    both(b, cap=len(recs) - 1)
    both(b, cap=0)
    # a read outside the buffer is absent
    t2 = b["tpl"].copy()
    k = int(np.flatnonzero(t2["len"][:, 0] > 0)[5])
    t2["off"][k][0] = len(b["seq"])
    both(dict(b, tpl=t2))
    with pytest.raises(BscError):
        pat_recs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, {"reserved": 1})
    with pytest.raises(ValueError):
        pat.patterns(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, {"reserved": 1})
    with pytest.raises(ValueError):
        pat.patterns(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, {"min_cov": 3})


def test_formatter_at_its_extremes():
    one, full = "T", "CT" * 16 + "T." * 15 + "TC"
    recs = [(0, one, 1), (0, full, 0xFFFFFFFF), (7, one, 0xFFFFFFFF), (0xFFFFFFFE, full, 1), (12345, "C.T", 1234567890)]
    packed = pat.pack(recs)
    assert pat.unpack(packed) == recs
    for base in (0, 9, 2 ** 32 - 1, 2 ** 63 - 2 ** 32, 2 ** 63):
        for name in ("c", "chr1", "x" * 255):
            want, lines = pat.format(name, base, recs)
            assert lines == 5 and pat_format_host(name, base, packed) == (want, 5)
            assert pat_format_host(name, base, packed, cap=len(want) - 1) == (None, len(want))  # a room one short: the need, nothing written
            assert [(c, i - base - 1, s, n) for c, i, s, n in pat.read_pat(want)] == [(name.encode(), i, s, n) for i, s, n in recs]
    assert pat.format("chr1", 9, recs[:2])[0] == b"chr1\t10\tT\t1\n" + b"chr1\t10\t" + full.encode() + b"\t4294967295\n"
    assert pat.format("chr1", 2 ** 63 - 2 ** 32, recs[3:4])[0] == b"chr1\t9223372036854775807\t" + full.encode() + b"\t1\n"
    assert len(pat.format("x" * 255, 2 ** 63, [(0xFFFFFFFE, full, 0xFFFFFFFF)])[0]) == 255 + 97  # the longest line: nineteen digits of twenty
    assert pat.format("chr1", 0, []) == (b"", 0) == pat_format_host("chr1", 0, packed[:0])
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(ValueError):
            pat.format(bad, 0, recs)
        with pytest.raises(BscError):
            pat_format_host(bad, 0, packed)
    with pytest.raises(BscError):
        pat_format_host("chr1", 0, packed, {"min_sites": 1, "reserved": 2})
    with pytest.raises(ValueError):
        pat.format("chr1", 0, recs, {"reserved": 2})
    with pytest.raises(BscError):
        pat_format_host("chr1", 2 ** 63 + 1, packed)
    with pytest.raises(ValueError):
        pat.format("chr1", 2 ** 63 + 1, recs)
    for bad in (b"chr1\t1\tCT\n", b"chr1\t1\t.C\t1\n", b"chr1\t1\tCA\t1\n"):
        with pytest.raises(ValueError):
            pat.read_pat(bad)


def test_count_sites_against_the_python_count():
    rng = np.random.default_rng(63)
    for n in (1, 2, 3, 64, 300):
        codes = rng.choice([1, 2, 2, 3, 3, 4, 0], n).astype(np.uint8)
        codes[-1] = 2  # a C at the contig's last position is no site
        if n >= 3:
            codes[-3:-1] = (2, 3)  # ... and the one in front of it is
        sites = [p for p in range(1, n) if codes[p - 1] == 2 and codes[p] == 3]
        count = lambda a, b: sum(a <= p < b for p in sites)  # noqa: E731
        assert pat_count_sites(codes, 1, n + 1) == len(sites) == pat_count_sites(codes, 1, n + 100)
        edges = sorted({1, n - 1, n, n + 1} | {p + d for p in sites[:4] + sites[-2:] for d in (-1, 0, 1, 2)})
        for a in edges:
            for b in edges:
                if a >= 1:
                    assert pat_count_sites(codes, a, b) == count(a, b), (n, a, b)
                    if a <= b:  # two halves are the whole
                        mid = (a + b) // 2
                        assert pat_count_sites(codes, a, mid) + pat_count_sites(codes, mid, b) == count(a, b)
        assert pat_count_sites(codes, n, n + 1) == 0
    with pytest.raises(BscError):
        pat_count_sites(codes, 0, 5)
    assert pat_count_sites(np.zeros(0, np.uint8), 1, 10) == 0


def test_contig_offsets_and_shift(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">chr1 first\nACGTC\nGACG\n>chr2\nCGCG\nNNC\n>chr3\nG\n")  # chr1: CG at 2, 5|6, 8: three; chr2: two; the C G across contigs is none
    off = pat.contig_offsets(str(fa))
    assert off == {b"chr1": 0, b"chr2": 3, b"chr3": 5}
    lines = [(b"chr1", 1, "CT", 2), (b"chr2", 2, "T", 1)]
    assert pat.shift(lines, off) == [(b"chr1", 1, "CT", 2), (b"chr2", 5, "T", 1)] and pat.shift(lines, 10)[1] == (b"chr2", 12, "T", 1)


def test_site_counts_against_the_read_level_table(big):
    """At min_sites 1 every state of every template is in exactly one piece: the table implies the read-level table's m and u per site, and its
    totals [3] and [4] are their sums."""
    n_states = 0
    for b in [P.hand_block(), big[0]] + P.placement_blocks() + P.long_read_blocks()[:2] + [c for c, _ in P.cut_blocks()]:
        recs, _, tot = pat_recs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], P.PAR)
        sites, ns, _ = cpg_reads_sites_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], {"min_sites": 1, "min_cov": 1})
        assert ns == tot[7]
        lines = pat.read_pat(pat.format("c", 0, pat.unpack(recs))[0])
        got = pat.site_counts(lines)
        for i, s in enumerate(sites):
            assert tuple(got.get((b"c", i + 1), (0, 0))) == (int(s["m"]), int(s["u"])), (b["name"], i)
        assert set(k[1] for k in got) <= set(range(1, ns + 1))
        assert tot[3] == int(sites["m"].astype(np.int64).sum()) and tot[4] == int(sites["u"].astype(np.int64).sum())
        n_states += tot[3] + tot[4]
    assert n_states > 50_000


def test_host_form_under_sanitizers(tmp_path):
    """make pat-san: integration/pat_san.c + csrc/pat.c under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "pat_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "pat_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "pat.c"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
