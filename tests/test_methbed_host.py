"""The host form of the methylation table's line (bsc_meth_format_rec, csrc/methbed.c) and bam2bcf --meth's refusals, on the CPU: lines
written out by hand, the cases that give no line, a buffer too small, 40 000 random records against the independent Python formatter
(tests/methbed_ref.py), and the option combinations that are refused before a context is created."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import methbed_ref as R
from bs_call_amd import _lib, methbed
from bs_call_amd.abi import VCF_REC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")


def rec(pos=1000, gt=4, cg=b"C", a=3, b=1, phred=50, flt=0, emit=1, cx_gt=b"ACGTA"):
    """A written record of a CC (gt 4) or GG (gt 7) call whose strand counts are a (not converted) and b (converted); the other counts hold
    values that must not show."""
    r = np.zeros(1, dtype=VCF_REC)[0]
    c = r["core"]
    c["pos"], c["emit"], c["gt"], c["cg"], c["phred"], c["flt"], c["cx_gt"] = pos, emit, gt, cg, phred, flt, cx_gt
    r["counts"] = [901, 902, 903, 904, 905, 906, 907, 908]
    if gt == 7:
        r["counts"][6], r["counts"][4] = a, b
    else:
        r["counts"][5], r["counts"][7] = a, b
    return r


def fmt(r, contig=b"chr1", **par):
    return methbed.format_rec(r, contig, methbed.params(**par))


# ---- lines written by hand ---------------------------------------------------------------------------------------------------------------
def test_plus_strand_three_of_four():
    assert fmt(rec(pos=1000, gt=4, a=3, b=1, phred=50)) == b"chr1\t999\t1000\tCG\t4\t+\t999\t1000\t255,155,0\t4\t75\t3\t1\t50\tPASS\n"


def test_minus_strand_none_of_seven():
    assert fmt(rec(pos=31, gt=7, a=0, b=7, phred=7)) == b"chr1\t30\t31\tCG\t7\t-\t30\t31\t0,255,0\t7\t0\t0\t7\t7\tPASS\n"


@pytest.mark.parametrize("a, b, pct, rgb", [(1, 1, 50, "255,255,0"), (1, 2, 33, "155,255,0"), (2, 1, 67, "255,205,0"), (7, 0, 100, "255,0,0"), (1, 199, 1, "0,255,0"),
                                            (1, 200, 0, "0,255,0"), (199, 1, 100, "255,0,0"), (99, 1, 99, "255,55,0"), (1, 9, 10, "55,255,0")])
def test_percentage_rounds_half_up(a, b, pct, rgb):
    want = "chr1\t999\t1000\tCG\t%d\t+\t999\t1000\t%s\t%d\t%d\t%d\t%d\t50\tPASS\n" % (min(a + b, 1000), rgb, a + b, pct, a, b)
    assert fmt(rec(a=a, b=b)) == want.encode()


def test_score_clamps_at_a_thousand():
    assert fmt(rec(a=400, b=600)) == b"chr1\t999\t1000\tCG\t1000\t+\t999\t1000\t205,255,0\t1000\t40\t400\t600\t50\tPASS\n"
    assert fmt(rec(a=400, b=601)) == b"chr1\t999\t1000\tCG\t1000\t+\t999\t1000\t205,255,0\t1001\t40\t400\t601\t50\tPASS\n"
    assert fmt(rec(a=999, b=0)) == b"chr1\t999\t1000\tCG\t999\t+\t999\t1000\t255,0,0\t999\t100\t999\t0\t50\tPASS\n"


def test_counts_at_the_top_of_32_bits():
    m = 2**32 - 1
    assert fmt(rec(a=m, b=m, gt=7)) == b"chr1\t999\t1000\tCG\t1000\t-\t999\t1000\t255,255,0\t8589934590\t50\t4294967295\t4294967295\t50\tPASS\n"
    assert fmt(rec(a=m, b=0)) == b"chr1\t999\t1000\tCG\t1000\t+\t999\t1000\t255,0,0\t4294967295\t100\t4294967295\t0\t50\tPASS\n"
    assert fmt(rec(a=m, b=1)) == b"chr1\t999\t1000\tCG\t1000\t+\t999\t1000\t255,0,0\t4294967296\t100\t4294967295\t1\t50\tPASS\n"


def test_first_and_last_position():
    assert fmt(rec(pos=1)) == b"chr1\t0\t1\tCG\t4\t+\t0\t1\t255,155,0\t4\t75\t3\t1\t50\tPASS\n"
    assert fmt(rec(pos=2**32 - 1)) == b"chr1\t4294967294\t4294967295\tCG\t4\t+\t4294967294\t4294967295\t255,155,0\t4\t75\t3\t1\t50\tPASS\n"


def test_longest_contig_and_longest_line():
    name = bytes(range(33, 127)) * 2 + b"x" * 67
    assert len(name) == 255
    assert fmt(rec(), name) == name + b"\t999\t1000\tCG\t4\t+\t999\t1000\t255,155,0\t4\t75\t3\t1\t50\tPASS\n"
    m = 2**32 - 1
    longest = fmt(rec(pos=m, gt=7, cg=b"H", cx_gt=b"NNNNN", a=m - 5, b=m, phred=255, flt=128), name, contexts=R.ALL)
    assert longest == name + b"\t4294967294\t4294967295\tCHN\t1000\t-\t4294967294\t4294967295\t255,255,0\t8589934585\t50\t4294967290\t4294967295\t255\tmac1\n"
    assert len(longest) == 255 + 111  # the bound the device encoder's image is sized by


@pytest.mark.parametrize("flt, text", [(0, "PASS"), (1, "fail"), (2, "fail"), (4, "fail"), (8, "fail"), (15, "fail"), (128, "mac1"), (129, "mac1"), (143, "mac1"), (64, "fail")])
def test_filter_text(flt, text):
    assert fmt(rec(flt=flt)) == ("chr1\t999\t1000\tCG\t4\t+\t999\t1000\t255,155,0\t4\t75\t3\t1\t50\t%s\n" % text).encode()


@pytest.mark.parametrize("gt, cg, cx, name", [(4, b"C", b"ACGTA", "CG"), (7, b"C", b"ACGTA", "CG"), (4, b"H", b"AACAG", "CHG"), (7, b"H", b"CAGAA", "CHG"),
                                              (4, b"H", b"GGCAA", "CHH"), (4, b"H", b"GGCAC", "CHH"), (4, b"H", b"GGCAT", "CHH"), (7, b"H", b"ATGCC", "CHH"),
                                              (7, b"H", b"GTGCC", "CHH"), (7, b"H", b"TTGCC", "CHH"), (4, b"H", b"AACA\0", "CHN"), (7, b"H", b"\0AGAA", "CHN"),
                                              (4, b"H", b"AACAR", "CHN"), (7, b"H", b"YAGAA", "CHN"), (4, b"H", b"AACAN", "CHN"), (7, b"H", b"gAGAA", "CHN"),
                                              (4, b"H", b"GACAg", "CHN"), (7, b"H", b"GAGAC", "CHH"), (4, b"H", b"CACAG", "CHG")])
def test_context_label(gt, cg, cx, name):
    r = rec(gt=gt, cg=cg, cx_gt=cx)
    raw = bytearray(r.tobytes())
    raw[19:24] = cx  # (numpy's S5 drops trailing NULs on the way in; the bytes as they are)
    want = ("chr1\t999\t1000\t%s\t4\t%s\t999\t1000\t255,155,0\t4\t75\t3\t1\t50\tPASS\n" % (name, "+" if gt == 4 else "-")).encode()
    assert methbed.format_rec(bytes(raw), b"chr1", methbed.params(contexts=R.ALL)) == want
    assert methbed.format_rec(bytes(raw), b"chr1", methbed.params(contexts=R.CPG)) == (want if cg == b"C" else b"")


# ---- no line ---------------------------------------------------------------------------------------------------------------------------------
def test_records_that_give_no_line():
    assert fmt(rec(emit=0)) == b""
    assert fmt(rec(emit=2)) != b""  # any non-zero flag
    for gt in [0, 1, 2, 3, 5, 6, 8, 9, 10, 36, 255]:
        assert fmt(rec(gt=gt), contexts=R.ALL) == b"", gt
    for cg in [b"N", b"?", b".", b"c", b"h", b"G", b"\0", b"\xc3"]:
        assert fmt(rec(cg=cg), contexts=R.ALL) == b"", cg
    assert fmt(rec(cg=b"H")) == b"" and fmt(rec(cg=b"H"), contexts=R.ALL) != b""
    assert fmt(rec(a=0, b=0)) == b"" and fmt(rec(a=0, b=0, gt=7), min_cov=0) == b""
    assert fmt(rec(a=0, b=1), min_cov=0) != b""


def test_thresholds_one_below_and_at():
    assert fmt(rec(a=3, b=1), min_cov=5) == b"" and fmt(rec(a=3, b=2), min_cov=5) != b"" and fmt(rec(a=3, b=1), min_cov=4) != b""
    assert fmt(rec(a=2**32 - 1, b=2**32 - 1), min_cov=2**32 - 1) != b""
    assert fmt(rec(phred=19), min_phred=20) == b"" and fmt(rec(phred=20), min_phred=20) != b""
    assert fmt(rec(phred=255), min_phred=256) == b"" and fmt(rec(phred=255), min_phred=255) != b""
    assert fmt(rec(flt=1), pass_only=True) == b"" and fmt(rec(flt=128), pass_only=True) == b"" and fmt(rec(flt=0), pass_only=True) != b""
    assert fmt(rec(flt=1), pass_only=False) != b""


def test_defaults_and_bad_arguments():
    L = _lib.load()
    p = _lib.MethParams(9, 9, 9, 9)
    L.bsc_meth_params_default(C.byref(p))
    assert (p.contexts, p.min_cov, p.min_phred, p.pass_only) == (0, 1, 0, 0)
    raw, buf = rec().tobytes(), C.create_string_buffer(512)
    ok = _lib.MethParams()
    assert L.bsc_meth_format_rec(raw, b"chr1", C.byref(ok), buf, 512) > 0
    for contig in [b"", b"a\tb", b"a\nb", b"x" * 256, None]:
        assert L.bsc_meth_format_rec(raw, contig, C.byref(ok), buf, 512) < 0, contig
    assert L.bsc_meth_format_rec(None, b"chr1", C.byref(ok), buf, 512) < 0
    assert L.bsc_meth_format_rec(raw, b"chr1", None, buf, 512) < 0
    assert L.bsc_meth_format_rec(raw, b"chr1", C.byref(ok), None, 512) < 0
    assert L.bsc_meth_format_rec(raw, b"chr1", C.byref(_lib.MethParams(contexts=2)), buf, 512) < 0


def test_buffer_too_small_returns_the_length_and_writes_nothing_behind_it():
    L = _lib.load()
    raw, p = rec().tobytes(), _lib.MethParams()
    want = fmt(rec())
    for cap in [0, 1, len(want) - 1, len(want), len(want) + 1]:
        buf = (C.c_char * 128)(*([b"\xa5"] * 128))
        n = L.bsc_meth_format_rec(raw, b"chr1", C.byref(p), buf, cap)
        assert n == len(want)
        assert buf.raw[cap:] == b"\xa5" * (128 - cap)
        if cap >= len(want):
            assert buf.raw[: len(want)] == want and buf.raw[len(want) : cap] == b"\xa5" * (cap - len(want))
    assert L.bsc_meth_format_rec(raw, b"chr1", C.byref(p), None, 0) == len(want)


# ---- random records against the Python formatter -------------------------------------------------------------------------------------
def random_records(rng, n, shaped):
    """n records of random bytes; shaped: emit, gt, cg, the filter and the counts are then drawn so that most records give a line."""
    raw = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    if shaped:
        raw[:, 4] = rng.choice([0, 1, 1, 1, 1, 1, 1, 255], n)
        raw[:, 5] = rng.choice([4, 7, 4, 7, 4, 7, 0, 5, 9, 36], n)
        raw[:, 8] = rng.choice([0, 0, 0, 1, 8, 128, 143], n)
        raw[:, 11] = rng.choice(list(b"CCCHHHN?c"), n)
        raw[:, 19] = rng.choice(list(b"ACGTNRc\0"), n)
        raw[:, 23] = rng.choice(list(b"ACGTNYg\0"), n)
        counts = raw[:, 64:96].view("<u4")
        scale = rng.choice([0, 1, 3, 30, 1000, 70000, 2**32 - 1], (n, 8))
        counts[:] = (rng.random((n, 8)) * (scale + 1)).astype(np.uint64).clip(0, 2**32 - 1).astype(np.uint32)
        edge = rng.random(n) < 0.05
        counts[edge] = 2**32 - 1
    return raw


@pytest.mark.parametrize("shaped", [False, True])
def test_random_records_equal_the_python_formatter(shaped):
    rng = np.random.default_rng(20261019 + shaped)
    raw = random_records(rng, 20_000, shaped)
    n_lines = 0
    for par in [{}, {"contexts": R.ALL}, {"contexts": R.ALL, "min_cov": 5, "min_phred": 100, "pass_only": 1}]:
        p = _lib.MethParams(**par)
        got = methbed.format_recs(raw, b"chrR", p)
        want = [R.of_rec_bytes(raw[i].tobytes(), b"chrR", par) for i in range(len(raw))]
        assert got == b"".join(want), par
        n_lines += sum(1 for w in want if w)
    assert not shaped or n_lines > 8_000  # (random bytes alone give a line about once in 20 000 records)
    labels = set(ln.split(b"\t")[3] for ln in got.split(b"\n") if ln)
    assert not shaped or labels == {b"CG", b"CHG", b"CHH", b"CHN"}


def test_read_bed_plain_and_bgzf(tmp_path):
    from bs_call_amd import vcf

    text = fmt(rec()) + fmt(rec(pos=2000, gt=7, a=0, b=9, flt=128))
    (tmp_path / "t.bed").write_bytes(text)
    vcf.write_vcf_blobs(str(tmp_path / "t.bed.gz"), "", [text], True)
    for name in ("t.bed", "t.bed.gz"):
        t = methbed.read_bed(str(tmp_path / name))
        assert len(t) == 2 and list(t["chrom"]) == ["chr1", "chr1"] and list(t["end"]) == [1000, 2000] and list(t["strand"]) == ["+", "-"]
        assert list(t["pct"]) == [75, 0] and list(t["a"]) == [3, 0] and list(t["b"]) == [1, 9] and list(t["filter"]) == ["PASS", "mac1"]


# ---- bam2bcf --meth: refused before a context is created ----------------------------------------------------------------------------------
def _run(tmp_path, *args, env=None):
    assert os.path.exists(EXE), "run `make demo`"
    out = str(tmp_path / "out.bcf")
    r = subprocess.run([EXE, *args, str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), out, str(tmp_path / "rep.json")], capture_output=True,
                       text=True, timeout=60, env=dict(os.environ, **(env or {})))
    return r, out


def _refused(tmp_path, r, out, *words):
    assert r.returncode == 2, r.stderr + r.stdout
    assert "--meth" in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "out.bed"))


@pytest.mark.parametrize("args", [("--rank", "0", "--world", "2"), ("--world", "2"), ("--merge", "2"), ("-O", "u", "--merge", "3"), ("--format", "bcf", "--rank", "1", "--world", "4")])
def test_meth_of_a_sharded_run_is_refused(tmp_path, args):
    m = ("--meth", str(tmp_path / "out.bed"))
    for order in (m + args, args + m, m + ("--meth-all",) + args):
        r, out = _run(tmp_path, *order)
        _refused(tmp_path, r, out, "sharded run", "--rank / --world / --merge")


@pytest.mark.parametrize("var", ["BAM2BCF_HOST_READER", "BAM2BCF_HOST_BCF", "BAM2BCF_HOST_PREP"])
def test_meth_with_a_host_variant_is_refused(tmp_path, var):
    r, out = _run(tmp_path, "--meth", str(tmp_path / "out.bed"), env={var: "1"})
    _refused(tmp_path, r, out, "BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP")


def test_meth_without_a_value_is_refused():
    for args in (["--meth"], ["-O", "b", "--meth"], ["--index", "--meth"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--meth takes the path" in r.stderr, r.stderr


@pytest.mark.parametrize("opt", ["--meth-min-cov", "--meth-min-gq"])
@pytest.mark.parametrize("value", ["x", "-1", "", "4294967296", "3x"])
def test_meth_thresholds_take_counts(tmp_path, opt, value):
    r, out = _run(tmp_path, "--meth", str(tmp_path / "out.bed"), opt, value)
    _refused(tmp_path, r, out, opt, "takes a count")


def test_usage_names_the_option():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--meth out.bed" in r.stderr
