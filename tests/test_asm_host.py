"""The allele-specific methylation table on the host: csrc/asm.c (bsc_asm_pairs_host, bsc_asm_format, bsc_asm_fisher_p) against the Python form
of the rule (bs_call_amd/asm.py, with the oracle's pure-Python Fisher test) on the hand-made blocks of tests/asm_cases.py and on seeded random
ones, record for record and total for total; a block worked by hand; the 48 entries of ALLELE; Fisher's p against the reference's own binary
(directly where oracle/_ref is built, and always against the values recorded from it in tests/golden/asm_fisher.json); the special tables;
the formatter; and the host form under the address and undefined-behaviour sanitizers as a stand-alone program (integration/asm_san.c).
No GPU."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import asm_cases as A
from bs_call_amd import _lib, asm
from bs_call_amd.caller import BscError, asm_fisher_p_host, asm_format_host, asm_pairs_host
from oracle import py_model, ref_loader as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()
LFACT = asm.lfact_table()


def python_rule(b, cap=None):
    return asm.pairs(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["core"], b["emit"], b["min_qual"], py_model.fisher, LFACT, b["params"], cap=cap)


def both(b, cap=None):
    """The block through the Python rule and the host form; asserts they agree and returns (records, totals)."""
    want, wtot = python_rule(b, cap)
    got, n, tot = asm_pairs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["core"], b["emit"], LFACT, b["min_qual"], b["params"], cap=cap)
    assert n == wtot[1] and tot == wtot, (b["name"], n, tot, wtot)
    assert got.tobytes() == want.tobytes(), (b["name"], got, want)
    return want, wtot


def test_the_header_states_the_rule():
    for word in ("SNP ", "ALLELE(t, h)", "WINDOW", "OVERLAPPED", "DEEP", "AQ ", "46340", "-700.0", "1e-100", "bsc_asm_pair", "bsc_asm_params",
                 "bsc_asm_pairs_host", "bsc_asm_format", "bsc_asm_device", "bsc_asm_text_device", "bsc_block_asm_kept", "bsc_asm_stream_read",
                 "bsc_asm_stream_detach", "NOT by start", "Not built: sharded runs"):
        assert word in HEADER, word
    assert C.sizeof(_lib.AsmParams) == 16 and asm.PAIR.itemsize == 32
    p = _lib.AsmParams(9, 9, 9, 9)
    _lib.load().bsc_asm_params_default(C.byref(p))
    assert (p.min_phred, p.pass_only, p.max_dist, p.min_cov) == (20, 0, 500, 2)


def test_the_lfact_table_is_the_oracle_s():
    """ln k! as the context fills it: the oracle's store (lgamma(k + 1)) to the last few bits — the running sum and lgamma round differently —
    and the very numbers where the reference's binary is at hand."""
    for k in range(256):
        assert abs(LFACT[k] - py_model._libm.lgamma(float(k + 1))) <= 1e-12 * max(1.0, LFACT[k])
    if R.available():
        assert R.tables()[0].tobytes() == LFACT.tobytes()


def test_a_block_worked_by_hand():
    """Positions 201 .. 240, sites 205, 212, 220, 230, W = 8.  SNPs: 210 AT (window 202 .. 218: sites 205, 212), 221 CG (213 .. 229: site 220,
    whose G it is: OVERLAPPED), 230 CT (222 .. 238: site 230, whose C it is: OVERLAPPED).  Seven templates:
      T1 C2T 203 .. 222: A at 210 -> allele 1; 205 M, 212 U.  G at 221 -> allele 2 of CG; nothing to count
      T2 C2T 203 .. 222: T at 210 -> C or T -> allele 2; 205 U, 212 U.  G at 221 -> allele 2
      T3 G2A 203 .. 222: A at 210 -> G or A -> allele 1; G at 206 -> 205 M, A at 213 -> 212 U.  T at 221 -> neither C nor G
      T4 C2T 208 .. 215: quality 10 at 210 -> no byte, no allele
      T5 C2T 203 .. 207 + 209 .. 214: read 1 has T at 210 -> allele 2; read 0 has 205 M, read 1 has 212 M
      T6 C2T 225 .. 236: CT on C2T -> no allele
      T7 G2A 225 .. 236: C at 230 -> allele 1 of CT; the window's only site is overlapped
    (210, 205): m1 2 (T1 T3) u1 0 m2 1 (T5) u2 1 (T2).  (210, 212): m1 0 u1 2 (T1 T3) m2 1 (T5) u2 1 (T2).  Both: p = 1, aq 0.
    totals: 3 SNPs, 4 records, 7 observations (210: T1 T2 T3 T5; 221: T1 T2; 230: T7), 3 with allele 1 (T1, T3, T7), 8 adds, 0 DEEP."""
    b = A.hand_block()
    recs, tot = both(b)
    assert [tuple(int(v) for v in r) for r in recs] == A.HAND_RECORDS
    assert tot == A.HAND_TOTALS
    assert asm.format_pairs("chrT", recs, b["params"]) == (A.HAND_TABLE, 2)
    assert asm_format_host("chrT", recs, b["params"]) == (A.HAND_TABLE, 2)
    names, back = asm.read_table(A.HAND_TABLE)
    assert names == [b"chrT"] * 2 and back.tobytes() == recs[:2].tobytes()


@pytest.mark.parametrize("b,al", A.allele_blocks(), ids=lambda v: v["name"] if isinstance(v, dict) else None)
def test_the_48_entries_of_allele(b, al):
    recs, tot = both(b)
    counts = {0: (0, 0, 0, 0), 1: (1, 0, 0, 0), 2: (0, 0, 1, 0)}[al]
    assert len(recs) == 1 and tuple(int(recs[0][f]) for f in ("m1", "u1", "m2", "u2")) == counts, b["name"]
    assert tot[:5] == (1, 1, int(al != 0), int(al == 1), int(al != 0))
    bs, gt, base = int(b["tpl"]["bs_strand"][0]), int(b["core"]["gt"][10]), "ACGT".index(b["name"][-1])
    assert asm.allele(bs, gt, base) == al


def test_allele_table_is_complete():
    assert len(A.ALLELE_TABLE) == 12 and len(A.allele_blocks()) == 48
    assert set(A.ALLELE_TABLE) == {(bs, gt) for bs in (1, 2) for gt in asm.HET}


@pytest.mark.parametrize("b", A.targeted_blocks() + A.tile_blocks(), ids=lambda b: b["name"])
def test_targeted_blocks(b):
    recs, tot = both(b)
    name = b["name"]
    if name == "snps at x and y, W 1":
        assert tot[0] == 3 and [int(v) for v in recs["cpg_pos"]] == [3]  # the windows of 1 and of 200 hold no site
    if name == "snps at x and y, W 65535":
        assert tot[:2] == (3, 15) and recs["m1"].sum() + recs["u1"].sum() > 0 and recs["m2"].sum() + recs["u2"].sum() > 0
    if name == "overlapped sites":
        flags = {(int(r["snp_pos"]), int(r["cpg_pos"])): int(r["info"]) >> 8 for r in recs}
        assert flags[(1020, 1020)] == 1 and flags[(1031, 1030)] == 1 and flags[(1020, 1010)] == 0 and flags[(1031, 1020)] == 0
        assert all(int(r["m1"]) + int(r["u1"]) + int(r["m2"]) + int(r["u2"]) == 0 for r in recs if int(r["info"]) >> 8)
        assert tot[4] > 0
    if name == "mates and quality":
        assert tot[2] == 4 and tot[3] == 2  # templates 1 and 3: allele 1, 2 and 5: allele 2, 4: no byte at the SNP
        assert [tuple(int(r[f]) for f in ("m1", "u1", "m2", "u2")) for r in recs] == [(2, 0, 1, 1), (1, 1, 2, 0)]
    if name.startswith("thresholds") or name == "emit bytes":
        want = {"defaults": [1015, 1030], "min_phred 19": [1005, 1015, 1030], "min_phred 0": [1005, 1015, 1030], "pass_only": [1030], "min_phred 41": []}
        snps = want.get(name.split(": ")[-1], [1015])  # the emit bytes take 1030 away
        assert sorted(set(int(v) for v in recs["snp_pos"])) == snps and tot[0] == len(snps)
    if name in ("no snp", "no site"):
        assert len(recs) == 0 and tot[1] == 0 and tot[4] == 0
    if name == "no template":
        assert len(recs) == 2 and tot == (2, 2, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("seed,n_pos,nr,n_snps", [(1, 63, 40, 4), (2, 64, 40, 4), (3, 65, 40, 4), (4, 127, 60, 6), (5, 128, 60, 6), (6, 129, 60, 6), (7, 1500, 300, 12)])
def test_random_blocks(seed, n_pos, nr, n_snps):
    b = A.random_block(seed, n_pos, nr, n_snps)
    recs, tot = both(b)
    assert tot[0] > 0 and tot[1] == len(recs)
    if n_pos >= 127:
        assert tot[4] > 0
    # a room: counted, not stored; the stored records and totals [0 .. 4] do not depend on it
    for cap in (0, 1, len(recs) - 1):
        part, ptot = both(b, cap=cap)
        assert part.tobytes() == recs[:cap].tobytes() and ptot[:5] == tot[:5]
    both(dict(b, emit=None))
    both(dict(b, params=dict(b["params"], pass_only=1)))


def test_long_read():
    recs, tot = both(A.long_read_block())
    assert tot[0] == 2 and tot[2] == 4 and tot[3] == 2 and tot[4] > 20


def test_refusals():
    b = A.hand_block()
    for bad in ({"max_dist": 0}, {"max_dist": 65536}):
        with pytest.raises(BscError):
            asm_pairs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["core"], None, LFACT, 20, dict(b["params"], **bad))
        with pytest.raises(ValueError):
            python_rule(dict(b, params=dict(b["params"], **bad)))


# ---- Fisher's p ------------------------------------------------------------------------------------------------------------------------------
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "asm_fisher.json")))


def test_fisher_p_equals_the_recorded_reference_values():
    """Bits equal on every recorded table with z >= 1e-100; below it the rule asks only that the host form stays below, too."""
    c = np.array(GOLDEN["tables"], dtype=np.int32)
    want = np.array([float.fromhex(h) for h in GOLDEN["p_hex"]])
    assert len(c) >= 3000 and c.max() == 300 and (want >= 1e-100).sum() > 2500 and (want < 1e-100).sum() > 50
    got = asm_fisher_p_host(c, LFACT)
    big = want >= 1e-100
    bad = np.flatnonzero(got[big].view(np.uint64) != want[big].view(np.uint64))
    assert not len(bad), (c[big][bad[:3]], got[big][bad[:3]], want[big][bad[:3]])
    assert (got[~big] < 1e-100).all()


def test_fisher_p_equals_the_reference_binary():
    if not R.available():
        pytest.skip("oracle/_ref is not built here (%s)" % R.RECIPE)
    rng = np.random.default_rng(99)
    c = np.concatenate([rng.integers(0, 301, (2000, 4)), rng.integers(0, 9, (1000, 4)), np.array(GOLDEN["tables"])]).astype(np.int32)
    want = R.fisher_array(c)
    assert [float(v).hex() for v in want[3000:]] == GOLDEN["p_hex"]  # the fixture is this binary's
    got = asm_fisher_p_host(c, LFACT)
    big = want >= 1e-100
    assert (got[big].view(np.uint64) == want[big].view(np.uint64)).all() and (got[~big] < 1e-100).all()


def test_python_rule_s_fisher_gives_the_same_aq():
    """The Python rule takes p from the oracle's pure-Python model, which has no clamp: aq is the same on every recorded table."""
    c = np.array(GOLDEN["tables"], dtype=np.int32)[::7]
    recs = np.zeros(len(c), asm.PAIR)
    for k, row in enumerate(c):
        z = float(asm_fisher_p_host(row, LFACT)[0])
        want = int(-(math.log(z) / asm.LN10) * 10.0 + 0.5) if z >= 1e-100 else 1000
        assert asm.aq_of(row, LFACT, py_model.fisher) == want, row
        recs[k] = (1, 2, *row, want, 3)
    assert 0 in recs["aq"] and 1000 in recs["aq"] and ((recs["aq"] > 0) & (recs["aq"] < 1000)).any()


def _one_pair(n1m, n1u, n2m, n2u):
    """A block whose one record has the given counts: groups of identical three-base templates."""
    import cpg_reads_cases as K

    x = 50
    rows = []
    reps = []
    for base, st, n in (("A", "C", n1m), ("A", "T", n1u), ("T", "C", n2m), ("T", "T", n2u)):
        if n:
            rows.append((1, K.read(x + 10, 3, "G", at={x + 10: base, x + 11: st}), None))
            reps.append(n)
    b = A.block("one pair", rows, x, x + 19, K.ref_with_sites(x, 20, [x + 11]), {x + 10: 3}, params={"min_cov": 1})
    b["tpl"] = np.repeat(b["tpl"], reps)
    return b


def test_special_tables():
    def host(b):
        got, n, tot = asm_pairs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["core"], None, LFACT, 20, b["params"])
        assert n == 1
        return tuple(int(v) for v in got[0]), tot

    r, tot = host(_one_pair(20000, 0, 0, 20000))
    assert r == (60, 61, 20000, 0, 0, 20000, 1000, 3) and tot == (1, 1, 40000, 20000, 40000, 0, 0, 0)
    r, tot = host(_one_pair(46340, 0, 0, 0))  # not DEEP: p = 1
    assert r == (60, 61, 46340, 0, 0, 0, 0, 3) and tot[5] == 0
    r, tot = host(_one_pair(23170, 0, 0, 23170))
    assert r[6:] == (1000, 3) and tot[5] == 0
    r, tot = host(_one_pair(46341, 0, 0, 0))
    assert r == (60, 61, 46341, 0, 0, 0, 0, 3 | 2 << 8) and tot[5] == 1
    r, tot = host(_one_pair(23170, 1, 0, 23170))
    assert r[6:] == (0, 3 | 2 << 8) and tot[5] == 1
    b = _one_pair(1, 0, 0, 0)
    r, tot = host(dict(b, tpl=b["tpl"][:0]))  # an all-zero record: p = 1
    assert r == (60, 61, 0, 0, 0, 0, 0, 3) and tot == (1, 1, 0, 0, 0, 0, 0, 0)
    both(_one_pair(30, 2, 3, 40))  # a small table through the Python rule as well
    recs, _ = both(_one_pair(300, 0, 0, 300))
    assert int(recs[0]["aq"]) == 1000


# ---- the formatter ---------------------------------------------------------------------------------------------------------------------------
def test_the_formatter():
    recs = np.array([
        (4000000000, 3999999990, 1, 1, 1, 1, 7, 3),  # ten-digit positions, a negative dist
        (100, 165635, 12, 0, 0, 12, 1000, 8),
        (100, 90, 2, 0, 0, 0, 0, 1),  # allele 2 uncovered: no line
        (100, 99, 0, 0, 0, 0, 0, 2 | 1 << 8),  # OVERLAPPED: no line
        (100, 120, 40000, 0, 0, 40000, 0, 5 | 2 << 8),  # DEEP: no line
        (7, 9, 1, 0, 0, 1, 3, 6),
    ], dtype=asm.PAIR)
    want = (b"c\t3999999989\t3999999991\t4000000000\tAT\t1\t1\t1\t1\t7\t-10\n"
            b"c\t165634\t165636\t100\tGT\t12\t0\t0\t12\t1000\t165535\n"
            b"c\t8\t10\t7\tCT\t1\t0\t0\t1\t3\t2\n")
    for mc in (0, 1):  # min_cov 0 and 1 give the same lines
        par = {"min_cov": mc}
        assert asm_format_host("c", recs, par) == (want, 3) and asm.format_pairs("c", recs, par) == (want, 3)
    two = b"".join(l + b"\n" for l in want.split(b"\n")[:2])  # 1 + 0 < 2: the last line goes
    assert asm_format_host("c", recs, {"min_cov": 2}) == (two, 2) == asm.format_pairs("c", recs, {"min_cov": 2})
    assert asm_format_host("c", recs, {"min_cov": 1}, cap=len(want) - 1) == (None, len(want))  # one short: the need, nothing written
    assert asm_format_host("c", recs[:0], {}) == (b"", 0)
    assert asm_format_host("x" * 255, recs[:1], {"min_cov": 1})[0].startswith(b"x" * 255 + b"\t")
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(BscError):
            asm_format_host(bad, recs, {})
        with pytest.raises(ValueError):
            asm.format_pairs(bad, recs, {})
    rng = np.random.default_rng(5)
    rnd = np.zeros(500, asm.PAIR)
    for f in asm.PAIR.names:
        rnd[f] = (10 ** rng.integers(0, 10, 500) * rng.integers(1, 10, 500)).clip(1, 0xFFFFFFFF)
    rnd["info"] = rng.choice([1, 2, 3, 5, 6, 8, 0, 9, 3 | 1 << 8, 3 | 2 << 8], 500)
    for mc in (0, 2, 5000):
        assert asm_format_host("chr1", rnd, {"min_cov": mc}) == asm.format_pairs("chr1", rnd, {"min_cov": mc})


def test_host_form_under_sanitizers(tmp_path):
    """make asm-san: integration/asm_san.c + csrc/asm.c under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "asm_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "asm_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "asm.c"), "-lm", "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
    assert "asm-san:" in open(os.path.join(ROOT, "Makefile")).read()
