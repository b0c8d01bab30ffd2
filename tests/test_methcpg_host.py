"""The host form of the combined-strand CpG table (bsc_meth_cpg_format_recs, csrc/methcpg.c) on the CPU: tables worked out by hand — which
halves pair, where the line is placed, what it sums —, every one of them also against the independent Python rule (tests/methcpg_ref.py),
random records laid out as runs of consecutive positions against that rule, a buffer too small, the refused arguments, and bam2bcf
--meth-merge's refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import methcpg_ref as R
from bs_call_amd import _lib, methbed
from bs_call_amd.abi import VCF_REC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
R_ALL = 1  # BSC_METH_ALL


def rec(pos, strand, a=3, b=1, phred=50, flt=0, emit=1, cg=b"C"):
    """A written record of a CC ("+") or GG ("-") call — or of a heterozygous one (anything else) — whose strand counts are a (not
    converted) and b (converted); the other counts hold values that must not show."""
    r = np.zeros(1, dtype=VCF_REC)[0]
    c = r["core"]
    c["pos"], c["emit"], c["gt"], c["cg"], c["phred"], c["flt"] = pos, emit, {"+": 4, "-": 7}.get(strand, 5), cg, phred, flt
    r["counts"] = [901, 902, 903, 904, 905, 906, 907, 908]
    if strand == "-":
        r["counts"][6], r["counts"][4] = a, b
    else:
        r["counts"][5], r["counts"][7] = a, b
    return r


def tab(recs, contig=b"chr1", **par):
    """The host form's table and totals — checked against the Python rule on the way."""
    arr = np.array(recs, dtype=VCF_REC) if len(recs) else np.zeros(0, dtype=VCF_REC)
    got, tot = methbed.format_cpg_recs(arr, contig, methbed.params(**par), totals=True)
    want, wtot = R.of_rec_bytes(arr.tobytes(), contig, {k: int(v) for k, v in par.items()})
    assert got == want and tot == wtot
    return got, tot


def L1(start, strand, A, B, gq=50, ft="PASS", rgb=None, pct=None, contig="chr1"):
    cov = A + B
    pct = (200 * A + cov) // (2 * cov) if pct is None else pct
    rgb = R.RGB[pct // 10] if rgb is None else rgb
    return ("%s\t%d\t%d\tCG\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (contig, start, start + 2, min(cov, 1000), strand, start, start + 2, rgb, cov, pct, A,
                                                                             B, gq, ft)).encode()


# ---- tables worked out by hand ----------------------------------------------------------------------------------------------------------------
def test_a_pair_is_one_line_at_its_plus_half():
    got, tot = tab([rec(1000, "+", 3, 1), rec(1001, "-", 2, 4)])
    assert got == b"chr1\t999\t1001\tCG\t10\t.\t999\t1001\t255,255,0\t10\t50\t5\t5\t50\tPASS\n"
    assert tot == [len(got), 1, 5, 5, 1]


def test_single_halves_keep_their_strand_and_the_dinucleotide_s_start():
    got, tot = tab([rec(1000, "+", 3, 1)])
    assert got == b"chr1\t999\t1001\tCG\t4\t+\t999\t1001\t255,155,0\t4\t75\t3\t1\t50\tPASS\n" and tot == [len(got), 1, 3, 1, 0]
    got, tot = tab([rec(1001, "-", 0, 7, phred=7)])
    assert got == b"chr1\t999\t1001\tCG\t7\t-\t999\t1001\t0,255,0\t7\t0\t0\t7\t7\tPASS\n" and tot == [len(got), 1, 0, 7, 0]


def test_which_halves_pair():
    P, M = L1(999, "+", 3, 1), L1(999, "-", 2, 4)
    # positions two apart: two singles
    assert tab([rec(1000, "+"), rec(1002, "-", 2, 4)])[0] == P + L1(1000, "-", 2, 4)
    # a record between them that is no half: "the next record" is not the minus half
    assert tab([rec(1000, "+"), rec(1000, "x"), rec(1001, "-", 2, 4)])[0] == P + M
    # minus at p, plus at p + 1: two singles
    assert tab([rec(1000, "-", 2, 4), rec(1001, "+")])[0] == L1(998, "-", 2, 4) + L1(1000, "+", 3, 1)
    # plus, minus, minus: a pair and a single
    got, tot = tab([rec(1000, "+"), rec(1001, "-", 2, 4), rec(1002, "-", 1, 1)])
    assert got == L1(999, ".", 5, 5) + L1(1000, "-", 1, 1) and tot[1:] == [2, 6, 6, 1]
    # plus, plus, minus: a single and a pair
    got, tot = tab([rec(1000, "+", 9, 0), rec(1001, "+"), rec(1002, "-", 2, 4)])
    assert got == L1(999, "+", 9, 0) + L1(1000, ".", 5, 5) and tot[1:] == [2, 14, 5, 1]
    # plus, minus, plus, minus: two pairs
    got, tot = tab([rec(1000, "+"), rec(1001, "-", 2, 4), rec(1002, "+", 1, 0), rec(1003, "-", 0, 1)])
    assert got == L1(999, ".", 5, 5) + L1(1001, ".", 1, 1) and tot[1:] == [2, 6, 6, 2]
    # same position twice is no pair; nor is the plus half BEHIND the minus half at p + 1 - 2
    assert tab([rec(1000, "+"), rec(1000, "-", 2, 4)])[0] == P + L1(998, "-", 2, 4)


def test_a_gated_half_leaves_its_partner_single():
    plus, minus = rec(1000, "+", 3, 1, phred=50), rec(1001, "-", 2, 4, phred=19)
    assert tab([plus, minus])[0] == L1(999, ".", 5, 5, gq=19)
    assert tab([plus, minus], min_phred=20)[0] == L1(999, "+", 3, 1)
    assert tab([rec(1000, "+", 3, 1, phred=19), rec(1001, "-", 2, 4)], min_phred=20)[0] == L1(999, "-", 2, 4)
    failed = rec(1001, "-", 2, 4, flt=8)
    assert tab([plus, failed])[0] == L1(999, ".", 5, 5, ft="fail") and tab([plus, failed], pass_only=True)[0] == L1(999, "+", 3, 1)
    assert tab([rec(1000, "+", 3, 1, flt=1), rec(1001, "-", 2, 4)], pass_only=True)[0] == L1(999, "-", 2, 4)
    # not written, another call, another context: no half
    for other in (rec(1001, "-", 2, 4, emit=0), rec(1001, "x", 2, 4), rec(1001, "-", 2, 4, cg=b"H"), rec(1001, "-", 2, 4, cg=b"c")):
        assert tab([plus, other])[0] == L1(999, "+", 3, 1)
    # a partner without a read on its strand is no half
    assert tab([plus, rec(1001, "-", 0, 0)])[0] == L1(999, "+", 3, 1)
    assert tab([rec(1000, "+", 0, 0), rec(1001, "-", 2, 4)])[0] == L1(999, "-", 2, 4)
    assert tab([rec(1000, "+", 0, 0), rec(1001, "-", 0, 0)]) == (b"", [0, 0, 0, 0, 0])


def test_the_coverage_threshold_is_on_the_sum():
    pair = [rec(1000, "+", 1, 1), rec(1001, "-", 2, 0)]
    got, tot = tab(pair, min_cov=4)
    assert got == L1(999, ".", 3, 1) and tot[1:] == [1, 3, 1, 1]
    assert tab(pair[:1], min_cov=4)[0] == b"" and tab(pair[1:], min_cov=4)[0] == b""
    # one above the sum: no line at all — the minus half stays the pair's, it does not come back as a single
    assert tab(pair, min_cov=5) == (b"", [0, 0, 0, 0, 0])
    assert tab([rec(1000, "+", 1, 1), rec(1001, "-", 5, 0)], min_cov=7)[0] == L1(999, ".", 6, 1)
    assert tab([rec(1000, "+", 1, 1), rec(1001, "-", 5, 0)], min_cov=8)[0] == b""
    assert tab(pair, min_cov=0)[0] == L1(999, ".", 3, 1)


def test_gq_is_the_minimum_and_filter_the_or():
    assert tab([rec(1000, "+", phred=30), rec(1001, "-", 2, 4, phred=200)])[0] == L1(999, ".", 5, 5, gq=30)
    assert tab([rec(1000, "+", phred=255), rec(1001, "-", 2, 4, phred=0)])[0] == L1(999, ".", 5, 5, gq=0)
    for f0, f1, text in [(0, 0, "PASS"), (0, 128, "mac1"), (128, 0, "mac1"), (128, 1, "fail"), (8, 128, "fail"), (2, 4, "fail"), (128, 128, "mac1")]:
        assert tab([rec(1000, "+", flt=f0), rec(1001, "-", 2, 4, flt=f1)])[0] == L1(999, ".", 5, 5, ft=text), (f0, f1)
    for f, text in [(0, "PASS"), (128, "mac1"), (129, "fail"), (64, "fail"), (15, "fail")]:
        assert tab([rec(1000, "+", flt=f)])[0] == L1(999, "+", 3, 1, ft=text), f


def test_sums_beyond_32_bits_and_the_score_s_clamp():
    m = 2**32 - 1
    got, tot = tab([rec(1000, "+", m, m), rec(1001, "-", m, m)])
    assert got == b"chr1\t999\t1001\tCG\t1000\t.\t999\t1001\t255,255,0\t17179869180\t50\t8589934590\t8589934590\t50\tPASS\n"
    assert tot == [len(got), 1, 2 * m, 2 * m, 1]
    assert tab([rec(1000, "+", m, 0), rec(1001, "-", 1, 0)])[0] == L1(999, ".", 2**32, 0)
    assert tab([rec(1000, "+", 400, 100), rec(1001, "-", 0, 500)])[0] == b"chr1\t999\t1001\tCG\t1000\t.\t999\t1001\t205,255,0\t1000\t40\t400\t600\t50\tPASS\n"
    assert tab([rec(1000, "+", 400, 100), rec(1001, "-", 0, 499)])[0].split(b"\t")[4] == b"999"
    assert tab([rec(1000, "+", m, m), rec(1001, "-", m, m)], min_cov=m)[0] == got


def test_first_and_last_positions():
    m = 2**32 - 1
    assert tab([rec(1, "+"), rec(2, "-", 2, 4)])[0] == L1(0, ".", 5, 5)
    assert tab([rec(1, "+")])[0] == L1(0, "+", 3, 1) and tab([rec(2, "-", 2, 4)])[0] == L1(0, "-", 2, 4)
    # a minus half at 1 has no dinucleotide in the contig: q - 2 modulo 2^32, end in 64 bits
    assert tab([rec(1, "-", 2, 4)])[0] == b"chr1\t4294967295\t4294967297\tCG\t6\t-\t4294967295\t4294967297\t155,255,0\t6\t33\t2\t4\t50\tPASS\n"
    assert tab([rec(m - 1, "+"), rec(m, "-", 2, 4)])[0] == L1(m - 2, ".", 5, 5)
    # 2^32 - 1 has no partner: its successor is compared in 64 bits, position 0 is not it
    assert tab([rec(m, "+"), rec(0, "-", 2, 4)])[0] == L1(m - 1, "+", 3, 1) + L1(m - 1, "-", 2, 4)


def test_longest_contig_and_longest_line():
    name = bytes(range(33, 127)) * 2 + b"x" * 67
    assert len(name) == 255
    assert tab([rec(1000, "+"), rec(1001, "-", 2, 4)], name)[0] == name + L1(999, ".", 5, 5)[4:]
    m = 2**32 - 1
    longest, _ = tab([rec(0, "+", m - 5, m, phred=255, flt=128), rec(1, "-", m, m - 5, phred=255)], name)
    assert longest == name + b"\t4294967295\t4294967297\tCG\t1000\t.\t4294967295\t4294967297\t255,255,0\t17179869170\t50\t8589934585\t8589934585\t255\tmac1\n"
    assert len(longest) == 255 + 111  # the bound the device encoder's image is sized by: no other choice of the columns is longer
    # (rgb + pct is 11 bytes wide at pct 20 .. 89 and 10 at 100, which a coverage of 11 digits — 10^10 or more, A below 2^33 — never reaches)


def test_buffer_too_small_returns_the_length_and_writes_nothing():
    L = _lib.load()
    arr = np.array([rec(1000, "+"), rec(1001, "-", 2, 4), rec(1005, "+", 9, 9)], dtype=VCF_REC)
    want = L1(999, ".", 5, 5) + L1(1004, "+", 9, 9)
    p = _lib.MethParams()
    for cap in [0, 1, len(want) - 1, len(want), len(want) + 1]:
        buf = (C.c_char * 256)(*([b"\xa5"] * 256))
        tot = (C.c_uint64 * 5)()
        n = L.bsc_meth_cpg_format_recs(arr.ctypes.data, 3, b"chr1", C.byref(p), buf, cap, tot)
        assert n == len(want) and list(tot) == [len(want), 2, 14, 14, 1]
        if cap >= len(want):
            assert buf.raw[: len(want)] == want and buf.raw[len(want) :] == b"\xa5" * (256 - len(want))
        else:
            assert buf.raw == b"\xa5" * 256
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 3, b"chr1", C.byref(p), None, 0, None) == len(want)
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 2, b"chr1", C.byref(p), None, 0, None) == len(L1(999, ".", 5, 5))  # records at or beyond n do not exist
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 1, b"chr1", C.byref(p), None, 0, None) == len(L1(999, "+", 3, 1))
    assert L.bsc_meth_cpg_format_recs(None, 0, b"chr1", C.byref(p), None, 0, None) == 0


def test_bad_arguments_are_refused():
    L = _lib.load()
    arr = np.array([rec(1000, "+")], dtype=VCF_REC)
    buf, ok = C.create_string_buffer(512), _lib.MethParams()
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 1, b"chr1", C.byref(ok), buf, 512, None) > 0
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 1, b"chr1", C.byref(_lib.MethParams(contexts=R_ALL)), buf, 512, None) < 0
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 1, b"chr1", C.byref(_lib.MethParams(contexts=2)), buf, 512, None) < 0
    for contig in [b"", b"a\tb", b"a\nb", b"x" * 256, None]:
        assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 1, contig, C.byref(ok), buf, 512, None) < 0, contig
    assert L.bsc_meth_cpg_format_recs(None, 1, b"chr1", C.byref(ok), buf, 512, None) < 0
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 1, b"chr1", None, buf, 512, None) < 0
    assert L.bsc_meth_cpg_format_recs(arr.ctypes.data, 1, b"chr1", C.byref(ok), None, 512, None) < 0
    with pytest.raises(ValueError):
        methbed.format_cpg_recs(arr, b"chr1", methbed.params(contexts=R_ALL))


# ---- random records against the Python rule -------------------------------------------------------------------------------------------------
def random_runs(rng, n, shaped=True):
    """n records of random bytes at positions that run consecutively for a while and then jump; shaped: emit, gt, cg, the filter, GQ and
    the counts are then drawn so that most records are halves and many pair."""
    raw = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    step = np.where(rng.random(n) < 0.85, 1, rng.choice([2, 3, 50], n))
    raw[:, 0:4] = (1 + np.cumsum(step)).astype("<u4").view(np.uint8).reshape(n, 4)
    if shaped:
        raw[:, 4] = rng.choice([0, 1, 1, 1, 1, 1, 1, 255], n)
        raw[:, 5] = rng.choice([4, 7, 4, 7, 4, 7, 4, 7, 0, 5], n)
        raw[:, 8] = rng.choice([0, 0, 0, 0, 1, 8, 128, 143], n)
        raw[:, 9] = rng.choice([0, 19, 20, 50, 99, 100, 255], n)
        raw[:, 11] = rng.choice(list(b"CCCCCCCCHN"), n)
        counts = raw[:, 64:96].view("<u4")
        scale = rng.choice([0, 1, 3, 30, 1000, 70000, 2**32 - 1], (n, 8))
        counts[:] = (rng.random((n, 8)) * (scale + 1)).astype(np.uint64).clip(0, 2**32 - 1).astype(np.uint32)
        counts[rng.random(n) < 0.05] = 2**32 - 1
    return raw


@pytest.mark.parametrize("shaped", [False, True])
def test_random_runs_equal_the_python_rule(shaped):
    rng = np.random.default_rng(20261020 + shaped)
    raw = random_runs(rng, 20_000, shaped)
    seen = set()
    for par in [{}, {"min_cov": 5}, {"min_cov": 40, "min_phred": 20, "pass_only": 1}]:
        got, tot = methbed.format_cpg_recs(raw, b"chrR", _lib.MethParams(**par), totals=True)
        want, wtot = R.of_rec_bytes(raw.tobytes(), b"chrR", par)
        assert got == want and tot == wtot, par
        seen |= set(ln.split(b"\t")[5] for ln in got.split(b"\n") if ln)
        starts = [int(ln.split(b"\t")[1]) for ln in got.split(b"\n") if ln]
        assert all(s0 < s1 for s0, s1 in zip(starts, starts[1:]))  # positions increase: so do the lines' starts, strictly
        assert not shaped or (tot[1] > 1_000 and tot[4] > (1_000 if not par else 100)), tot
    assert not shaped or seen == {b"+", b"-", b"."}


def test_read_bed_takes_the_combined_strand(tmp_path):
    text, _ = tab([rec(1000, "+"), rec(1001, "-", 2, 4), rec(2000, "-", 0, 9, flt=128)])
    (tmp_path / "t.bed").write_bytes(text)
    t = methbed.read_bed(str(tmp_path / "t.bed"))
    assert list(t["strand"]) == [".", "-"] and list(t["start"]) == [999, 1998] and list(t["end"]) == [1001, 2000] and list(t["name"]) == ["CG", "CG"]
    assert list(t["a"]) == [5, 0] and list(t["b"]) == [5, 9] and list(t["coverage"]) == [10, 9] and list(t["filter"]) == ["PASS", "mac1"]


# ---- bam2bcf --meth-merge: refused before a context is created ------------------------------------------------------------------------------
def _run(tmp_path, *args):
    assert os.path.exists(EXE), "run `make demo`"
    out = str(tmp_path / "out.bcf")
    r = subprocess.run([EXE, *args, str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), out, str(tmp_path / "rep.json")], capture_output=True, text=True, timeout=60)
    return r, out


def test_meth_merge_without_meth_is_refused(tmp_path):
    for args in (("--meth-merge",), ("-O", "b", "--meth-merge"), ("--meth-merge", "--meth-min-cov", "4")):
        r, out = _run(tmp_path, *args)
        assert r.returncode == 2 and "--meth-merge" in r.stderr and "needs --meth" in r.stderr, r.stderr
        assert not os.path.exists(out)


def test_meth_merge_with_meth_all_is_refused(tmp_path):
    bed = str(tmp_path / "out.bed")
    for args in (("--meth", bed, "--meth-merge", "--meth-all"), ("--meth-all", "--meth-merge", "--meth", bed)):
        r, out = _run(tmp_path, *args)
        assert r.returncode == 2 and "--meth-merge" in r.stderr and "--meth-all" in r.stderr and "partner strand" in r.stderr, r.stderr
        assert not os.path.exists(out) and not os.path.exists(bed)


def test_usage_names_the_option():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--meth-merge" in r.stderr
