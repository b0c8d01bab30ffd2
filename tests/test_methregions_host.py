"""The host forms of the per-region methylation summary (csrc/methregions.c) on the CPU: the sum over packed records against the
independent Python rule (tests/methregions_ref.py) with region sets of every relation, the formatter's bytes against Python's, the BED
reader on well-formed and malformed text, the package's numpy form (methbed.region_summary over table rows) against the same rule, the
stand-alone sanitizer program of the reader and formatter (integration/methregions_san.c), and bam2bcf's refusals."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import methregions_ref as R
from bs_call_amd import _lib, methbed
from methregions_ref import random_records, region_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")


PARS = [{}, {"min_cov": 5}, {"min_phred": 100}, {"pass_only": 1}, {"contexts": 1}, {"contexts": 1, "min_cov": 3, "min_phred": 20, "pass_only": 1}]


@pytest.mark.parametrize("par", PARS)
def test_host_sum_equals_the_python_rule(par):
    rng = np.random.default_rng(8100 + len(par))
    for x0, n in ((1, 300), (5000, 257), (2**32 - 200, 200)):
        recs = random_records(rng, n, x0, wide=True)
        regs = region_sets(x0, n)
        want = R.summary(R.sites_of_rec_bytes(recs.tobytes(), par), regs)
        got = methbed.region_summary(recs, regs, methbed.params(**par))
        assert got.tolist() == want, (par, x0)
        whole = [k for k, r in enumerate(regs) if r == (max(x0 - 51, 0), min(x0 - 1 + n + 50, 2**32 - 1))]
        assert len(whole) == 2 and want[whole[0]][0] > 5 and want[whole[0]] == want[whole[1]]
        assert all(want[k] == [0, 0, 0, 0] for k, (s, e) in enumerate(regs) if s == e or e <= x0 - 1 or s >= x0 - 1 + n)
    # the thresholds each take sites away; the other contexts add some
    recs, regs = random_records(rng, 2000), [(0, 2000)]
    plain = methbed.region_summary(recs, regs)[0]
    one = methbed.region_summary(recs, regs, methbed.params(**par))[0]
    if par:
        assert (one[0] > plain[0]) if par == {"contexts": 1} else (0 < one[0] < plain[0] or "contexts" in par)


def test_host_sum_adds_into_acc_and_skips_pos_zero():
    recs = random_records(np.random.default_rng(8200), 64, 0)  # the first record has pos = 0
    c = recs["core"]
    c["emit"], c["gt"], c["cg"], c["flt"] = 1, 4, b"C", 0
    recs["core"] = c
    recs["counts"] = 2
    regs = [(0, 64)]
    L = _lib.load()
    acc = np.array([[10, 20, 30, 40]], dtype=np.uint64)
    r = np.array(regs, dtype=np.uint32)
    p = methbed.params()
    import ctypes as C

    assert L.bsc_meth_regions_sum_recs(recs.ctypes.data, 64, C.byref(p), r.ctypes.data, 1, acc.ctypes.data) == 0
    assert acc.tolist() == [[10 + 63, 20 + 2 * 63, 30 + 2 * 63, 40 + 50 * 63]] == R.summary(R.sites_of_rec_bytes(recs.tobytes()), regs, [[10, 20, 30, 40]])
    bad = np.array([[5, 4]], dtype=np.uint32)
    assert L.bsc_meth_regions_sum_recs(recs.ctypes.data, 64, C.byref(p), bad.ctypes.data, 1, acc.ctypes.data) == -1 and b"start 5 > end 4" in L.bsc_last_error()
    assert L.bsc_meth_regions_sum_recs(recs.ctypes.data, 64, C.byref(methbed.params(contexts=2)), r.ctypes.data, 1, acc.ctypes.data) == -1


def test_formatter_bytes_equal_python_s():
    regs = [(0, 2**32 - 1), (100, 150), (100, 200), (100, 200), (7, 7)]
    names = ["whole", None, "a name with spaces", "x" * 255, "."]
    acc = [[0, 0, 0, 0], [1, 1, 0, 100], [3, 3 * (2**32 - 1), 5, 250], [70, 2**40, 2**41, 2310], [2, 0, 9, 0]]
    want = R.lines("chr1", regs, names, acc)
    got = methbed.format_regions("chr1", regs, [n or "." for n in names], acc)
    assert got == want
    assert b"chr1\t0\t4294967295\twhole\t0\t0\t0\t0\t.\t.\n" in got  # sites == 0
    assert b"chr1\t100\t200\ta name with spaces\t3\t12884901890\t12884901885\t5\t100\t83\n" in got  # A + B above 2^32
    assert methbed.format_regions(b"c", regs, None, acc) == R.lines("c", regs, None, acc)
    assert methbed.format_regions("chr1", [], None, np.zeros((0, 4))) == b""
    rng = np.random.default_rng(8300)
    regs = sorted((int(s), int(s + w)) for s, w in zip(rng.integers(0, 2**31, 200), rng.integers(0, 2**31, 200)))
    acc = [[int(n), int(a), int(b), int(p)] for n, a, b, p in zip(rng.integers(1, 10**6, 200), rng.integers(0, 2**45, 200), rng.integers(1, 2**45, 200), rng.integers(0, 10**8, 200))]
    acc[17] = [0, 0, 0, 0]
    assert methbed.format_regions("chrUn_KI270742v1", regs, None, acc) == R.lines("chrUn_KI270742v1", regs, None, acc)
    for bad in ("", "a\tb", "a\nb", "y" * 256):
        with pytest.raises(ValueError):
            methbed.format_regions(bad, regs, None, acc)
        with pytest.raises(ValueError):
            methbed.format_regions("c", regs[:1], [bad], acc[:1])
    # too little room: the length needed, nothing written
    import ctypes as C

    L = _lib.load()
    r, a = np.array(regs[:3], dtype=np.uint32), np.array(acc[:3], dtype=np.uint64)
    full = methbed.format_regions("c", regs[:3], None, acc[:3])
    buf = C.create_string_buffer(b"\xee" * len(full), len(full))
    assert L.bsc_meth_regions_format(b"c", r.ctypes.data, None, a.ctypes.data, 3, buf, len(full) - 1) == len(full) and buf.raw == b"\xee" * len(full)


GOOD = (b"# a comment\ntrack name=x\nbrowser position chr1:1-100\r\n\n\r\nchr1\t100\t200\tsecond\t0\t+\nchr2 5 9 spaced\nchr1\t100\t200\tthird\r\n"
        b"chr1\t0\t4294967295\nchr1\t100\t150\t\nchr2\t7\t7\tempty region\textra\tcolumns\there\nchr1\t100\t200\tfourth\ntrackless\t1\t2\n")


def test_parser_on_well_formed_text(tmp_path):
    got = methbed.parse_regions(GOOD)
    assert list(got) == ["chr1", "chr2", "trackless"]  # in order of first appearance; a contig whose name begins with "track" is a contig
    regs, names = got["chr1"]
    assert [tuple(r) for r in regs.tolist()] == [(0, 4294967295), (100, 150), (100, 200), (100, 200), (100, 200)]
    assert names == [".", ".", "second", "third", "fourth"]  # a missing and an empty name; duplicates keep the file's order
    regs, names = got["chr2"]
    assert [tuple(r) for r in regs.tolist()] == [(5, 9), (7, 7)] and names == ["spaced", "empty region"]  # spaces; more than four columns
    assert methbed.parse_regions(b"") == {} and methbed.parse_regions(b"#only\n\n") == {}
    p = tmp_path / "r.bed"
    p.write_bytes(GOOD)
    assert list(methbed.read_regions(str(p))) == ["chr1", "chr2", "trackless"]
    import gzip

    (tmp_path / "r.bed.gz").write_bytes(gzip.compress(GOOD))
    assert methbed.read_regions(str(tmp_path / "r.bed.gz"))["chr2"][1] == ["spaced", "empty region"]


@pytest.mark.parametrize("text, line, what", [
    (b"chr1\t1\t2\nchr1\t5\n", 2, "columns"),
    (b"chr1\n", 1, "columns"),
    (b"#c\nchr1\t1x\t2\n", 2, "coordinate"),
    (b"chr1\t-1\t2\n", 1, "coordinate"),
    (b"chr1\t1\t\n", 1, "coordinate"),
    (b"chr1\t1\t2\n\nchr1\t1\t4294967296\n", 3, "coordinate"),
    (b"chr1\t4294967296\t4294967297\n", 1, "coordinate"),
    (b"chr1\t9\t8\n", 1, "start 9 > end 8"),
    (b"\t1\t2\n", 1, "name is empty"),
    (b" 1 2\n", 1, "name is empty"),
    (b"chr1\t1\t2\nchr1\t3\t4", 2, "no newline"),
    (b"chr1\t1\t2\r\n" + b"c" * 256 + b"\t1\t2\n", 2, "255"),
])
def test_parser_refuses_with_the_line_number(text, line, what):
    with pytest.raises(ValueError) as ei:
        methbed.parse_regions(text)
    assert ("line %d:" % line) in str(ei.value) and what in str(ei.value)


def test_region_summary_over_table_rows_equals_the_rule():
    """methbed.region_summary over the rows of a per-cytosine table (what the file-to-file tests compare bam2bcf with): prefix sums over the
    sorted starts — against the plain double loop of the Python rule."""
    rng = np.random.default_rng(8400)
    n = 500
    rows = np.zeros(n, dtype=methbed.BED)
    pos = np.sort(rng.choice(np.arange(1, 3000), n, replace=False))
    rows["start"], rows["a"], rows["b"] = pos - 1, rng.integers(0, 2**32, n), rng.integers(1, 2**32, n)
    regs = region_sets(1, 3000) + [(2**32 - 2, 2**32 - 1)]
    want = R.summary([(int(p), int(a), int(b)) for p, a, b in zip(pos, rows["a"], rows["b"])], regs)
    whole = want[regs.index((0, 3050))]
    assert methbed.region_summary(rows, regs).tolist() == want and whole[0] == n and whole[1] > 2**32
    assert methbed.region_summary(rows[::-1], regs).tolist() == want  # rows in any order
    assert methbed.region_summary(rows[:0], regs).tolist() == [[0, 0, 0, 0]] * len(regs)
    w = methbed.window_regions(3000, 7)
    assert w["start"].tolist() == list(range(0, 3000, 7)) and w["end"][-1] == 3000 and (w["end"][:-1] == w["start"][1:]).all()
    assert methbed.region_summary(rows, w).sum(axis=0).tolist() == whole  # windows partition the contig
    with pytest.raises(ValueError):
        methbed.window_regions(100, 0)


def test_reader_and_formatter_under_the_sanitizers(tmp_path):
    """The stand-alone program of csrc/methregions.c (integration/methregions_san.c: the malformed and well-formed cases above, each text in
    a heap block of exactly its length), compiled with -fsanitize=address,undefined and run as a process of its own."""
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "methregions_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "methregions_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "methregions.c"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr


def test_bam2bcf_refusals():
    assert os.path.exists(EXE), "run `make demo`"

    def refused(args, word, env=None):
        r = subprocess.run([EXE, *args, "in.bam", "ref.fa", "out.bcf", "out.json"], capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))
        assert r.returncode == 2 and word in r.stderr, (args, r.stderr)

    R2 = ["--meth-regions", "r.bed", "--meth-regions-out", "o.tsv"]
    refused(["--meth-regions", "r.bed"], "--meth-regions-out")
    refused(["--meth-regions-out", "o.tsv"], "--meth-regions regions.bed or --meth-window")
    refused(R2 + ["--meth-window", "1000"], "exclude each other")
    refused(["--meth-window", "0", "--meth-regions-out", "o.tsv"], "--meth-window takes")
    refused(["--meth-window", "12x", "--meth-regions-out", "o.tsv"], "--meth-window takes")
    refused(R2 + ["--rank", "0", "--world", "2"], "--meth-regions sums a single run")
    refused(R2 + ["--merge", "2"], "--meth-regions sums a single run")
    refused(["--meth-window", "100", "--meth-regions-out", "o.tsv", "--world", "2"], "--meth-regions sums a single run")
    for var in ("BAM2BCF_HOST_READER", "BAM2BCF_HOST_BCF", "BAM2BCF_HOST_PREP"):
        refused(R2, "not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP", env={var: "1"})
