"""The per-region fragment methylation summary on the host: csrc/frag.c (bsc_frag_regions_host, bsc_frag_format) against the Python form of
the rule (bs_call_amd/frag.py) and the hand tallies of tests/frag_cases.py, accumulator for accumulator and total for total; the formatter
and the table's reader; the one-region sums against the read-level CpG table of the same block; the same sums from the PAT table's records.
No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import frag_cases as F
from bs_call_amd import _lib, frag, pat
from bs_call_amd.caller import BscError, cpg_reads_sites_host, frag_format_host, frag_regions_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()


def both(b, regions=None, params=None):
    """The block through the Python rule and the host form; asserts they agree and returns (accumulators, totals)."""
    regions = b["regions"] if regions is None else regions
    params = b["params"] if params is None else params
    want, wtot = frag.region_frags(b, regions, params)
    got, tot = frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], regions, b["min_qual"], params)
    assert tot == wtot, (b["name"], tot, wtot)
    assert got.tolist() == want.tolist(), b["name"]
    assert tot[1:] == tuple(int(v) for v in want[:, :7].sum(axis=0)) if len(want) else tot[1:] == (0,) * 7
    assert (want[:, 0] == want[:, 1] + want[:, 2] + want[:, 3]).all() and (want[:, 5] <= want[:, 4]).all() and (want[:, 6] <= want[:, 0]).all()
    return want, wtot


def test_the_header_states_the_rule():
    for word in ("IN(s, R)", "SHORT", "FRAGMENT", "DISCORDANT", "LIMITS", "No template spans two blocks", "bsc_frag_params", "bsc_frag_regions_host",
                 "bsc_frag_format", "bsc_frag_attach", "bsc_frag_device", "bsc_block_frag_kept", "bsc_frag_read", "bsc_frag_reset"):
        assert word in HEADER, word
    assert C.sizeof(_lib.FragParams) == 16 and frag.N_SUMS == 8 == frag.N_TOTALS
    p = _lib.FragParams(9, 9, 99, 9)
    _lib.load().bsc_frag_params_default(C.byref(p))
    assert (p.min_sites, p.u_max_pct, p.m_min_pct, p.reserved) == (3, 25, 75, 0)


def test_a_block_worked_by_hand():
    """tests/frag_cases.py: hand_block's docstring has the tally, template by template and region by region."""
    b = F.hand_block()
    assert tuple(frag.site_positions(b["x"], b["y"], b["ref"])) == F.HAND_SITES and b["regions"] == F.HAND_REGIONS
    acc, tot = both(b)
    assert [tuple(int(v) for v in r) for r in acc] == F.HAND_ACC and tot == F.HAND_TOTALS
    assert frag.format_regions("chrF", b["regions"], F.HAND_NAMES, acc) == F.HAND_TABLE == frag_format_host("chrF", b["regions"], F.HAND_NAMES, acc)
    rows = frag.read_table(F.HAND_TABLE)
    assert [tuple(int(r[n]) for n in frag.SUM_NAMES) for r in rows] == F.HAND_ACC and [r["name"] for r in rows] == [b"all", b".", b"island", b"empty", b"tail"]
    f = frag.fractions(rows[0])
    assert (f["U"], f["X"], f["M"], f["disc"]) == (0.25, 0.5, 0.25, 0.75) and f["level"] == 16 / 30
    assert all(math.isnan(v) for v in frag.fractions(rows[3]).values())
    # k = min_sites - 1 against k = min_sites: at min_sites 4 T4's three sites of B are short, at 2 its two of C a fragment
    acc4, _ = both(b, params=dict(F.PAR, min_sites=4))
    assert tuple(int(v) for v in acc4[1]) == (2, 0, 1, 1, 8, 5, 2, 2) and int(acc4[2][0]) == 0 and int(acc4[2][7]) == 4
    acc2, _ = both(b, params=dict(F.PAR, min_sites=2))
    assert tuple(int(v) for v in acc2[2]) == (4, 1, 1, 2, 11, 6, 1, 0)  # + T4: k 2, m 2: M
    # regions need not be sorted on the host, and each is summed alone: the reversed list gives the reversed rows
    back, btot = both(b, regions=b["regions"][::-1])
    assert back.tolist() == acc.tolist()[::-1] and btot == tot


def test_the_class_borders():
    """(k, m) of F.BORDER_KM: (4, 1) U, (4, 3) M, (3, 1) X, (8, 2) U, (8, 6) M, (8, 3) X, and (1, 0) U / (1, 1) M where min_sites is 1."""
    p = frag._params(None)
    assert [frag.classify(k, m, p) for k, m in F.BORDER_KM] == [frag.CU, frag.CM, frag.CX, frag.CU, frag.CM, frag.CX, frag.CU, frag.CM]
    acc, tot = both(F.borders_block())
    assert tuple(int(v) for v in acc[0]) == (6, 2, 2, 2, 35, 16, 6, 2) and tot == (8, 6, 2, 2, 2, 35, 16, 6)
    acc, _ = both(F.borders_block(dict(F.PAR, min_sites=1)))
    assert tuple(int(v) for v in acc[0]) == (8, 3, 2, 3, 37, 17, 6, 0)
    acc, _ = both(F.borders_block({"min_sites": 1, "u_max_pct": 0, "m_min_pct": 100}))  # U iff m == 0, M iff m == k
    assert tuple(int(v) for v in acc[0]) == (8, 1, 6, 1, 37, 17, 6, 0)


SMALL = F.small_blocks()


@pytest.mark.parametrize("b", SMALL, ids=lambda b: b["name"])
def test_host_form_equals_the_python_rule(b):
    acc, tot = both(b)
    if b["name"].startswith("contention, one"):
        assert tuple(int(v) for v in acc[0]) == (5000, 0, 5000, 0, 20000, 10000, 5000, 0)  # M U M U: 200 of 4: X
    if b["name"].startswith("contention, 16"):
        assert int(acc[0][1]) > 0 and int(acc[0][2]) > 0 and int(acc[0][3]) > 0 and int(acc[0][0]) == 5000
    if "candidates" in b["name"]:
        assert (acc[:, 0] + acc[:, 7] >= 2).all()  # every region holds sites of the two full reads


@pytest.mark.parametrize("nr", F.COUNTS)
def test_host_form_equals_the_python_rule_on_the_count_series(nr):
    acc, tot = both(F.count_block(nr))
    if nr == 0:
        assert tot == (0,) * 8 and not acc.any()
    if nr >= 63:
        assert tot[0] > nr // 2 and tot[1] > 0


def test_host_form_equals_the_python_rule_on_the_big_block():
    acc, tot = both(F.big_block())
    assert tot[1] > 1000 and tot[2] > 0 and tot[3] > 0 and tot[4] > 0 and int((acc[:, 0] > 0).sum()) > 500


def test_accumulators_add_and_totals_may_be_null():
    b = F.hand_block()
    once, tot = both(b)
    twice, _ = frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], b["params"], acc=once)
    assert twice.tolist() == (2 * once).tolist()
    half = len(b["tpl"]) // 2
    a1, t1 = frag_regions_host(b["tpl"][:half], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], b["params"])
    a2, t2 = frag_regions_host(b["tpl"][half:], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], b["params"], acc=a1)
    assert a2.tolist() == once.tolist() and tuple(u + v for u, v in zip(t1, t2)) == tot
    quiet, zero = frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], b["params"], with_totals=False)
    assert quiet.tolist() == once.tolist() and zero == (0,) * 8


@pytest.mark.parametrize("bad", [{"min_sites": 0}, {"u_max_pct": 101, "m_min_pct": 102}, {"m_min_pct": 101}, {"u_max_pct": 75}, {"u_max_pct": 80},
                                 {"reserved": 1}], ids=str)
def test_the_refusals(bad):
    b = F.hand_block()
    before = np.full((len(b["regions"]), 8), 7, np.uint64)
    with pytest.raises(BscError):
        frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], dict(F.PAR, **bad), acc=before)
    with pytest.raises(ValueError):
        frag.region_frags(b, b["regions"], dict(F.PAR, **bad))


def test_other_refusals_of_the_host_form():
    b = F.hand_block()
    with pytest.raises(BscError):
        frag_regions_host(b["tpl"], b["seq"], b["y"], b["x"], b["ref"], b["regions"], b["min_qual"], F.PAR)  # y < x
    with pytest.raises(BscError):
        frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], [(5, 4)], b["min_qual"], F.PAR)  # start > end


def test_the_formatter_s_lines_and_refusals():
    regs = [(0, 10), (5, 4000000000), (7, 7)]
    acc = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [2**64 - 1] * 8, [0] * 8], np.uint64)
    want = (b"c\t0\t10\t.\t1\t2\t3\t4\t5\t6\t7\t8\n" + b"c\t5\t4000000000\tn 1\t" + b"\t".join([b"18446744073709551615"] * 8) + b"\n"
            + b"c\t7\t7\t.\t0\t0\t0\t0\t0\t0\t0\t0\n")
    assert frag_format_host("c", regs, [None, "n 1", None], acc) == want == frag.format_regions("c", regs, [None, "n 1", None], acc)
    assert frag_format_host("c", regs, None, acc) == want.replace(b"n 1", b".") == frag.format_regions("c", regs, None, acc)
    assert frag_format_host("c", regs, [None, "n 1", None], acc, cap=len(want) - 1) == (None, len(want))  # too small: the need, nothing written
    assert frag_format_host("c", [], None, np.zeros((0, 8), np.uint64)) == b""
    for contig, names in (("", None), ("a\tb", None), ("x" * 256, None), ("c", ["", "a", "b"]), ("c", ["a", "b\nc", "d"]), ("c", ["a", "b", "y" * 256])):
        with pytest.raises(ValueError):
            frag_format_host(contig, regs, names, acc)
        with pytest.raises(ValueError):
            frag.format_regions(contig, regs, names, acc)
    assert len(frag_format_host("x" * 255, regs[:1], ["y" * 255], acc[:1])) == 255 * 2 + len(b"\t0\t10\t\t1\t2\t3\t4\t5\t6\t7\t8\n")
    with pytest.raises(ValueError):
        frag.read_table(b"c\t0\t10\t.\t1\t2\t3\n")
    with pytest.raises(ValueError):
        frag.read_table(b"c\t0\t10\t.\t3\t1\t1\t0\t9\t4\t1\t0\n")  # the classes do not add up


@pytest.mark.parametrize("b", [F.hand_block(), F.first_long_block(), F.count_block(65), F.candidates_block(1)], ids=lambda b: b["name"])
@pytest.mark.parametrize("s", (1, 2, 3, 5))
def test_one_region_over_the_block_meets_the_read_level_table(b, s):
    """frags = the read-level table's eligible templates and disc = its discordant ones at its min_sites = s; at s = 1 Mm = its sum of m,
    K = its sum of m + u and frags = its templates with a state."""
    whole = [(max(b["x"] - 1, 0), b["y"])]
    acc, tot = both(b, regions=whole, params=dict(F.PAR, min_sites=s))
    _, _, rt = cpg_reads_sites_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], {"min_sites": s, "min_cov": 1})
    assert (int(acc[0][0]), int(acc[0][6])) == (rt[5], rt[6]) and tot[0] == rt[4] and int(acc[0][0]) + int(acc[0][7]) == rt[4]
    if s == 1:
        assert (int(acc[0][5]), int(acc[0][4]), int(acc[0][0])) == (rt[1], rt[1] + rt[2], rt[4])


@pytest.mark.parametrize("b", [F.hand_block(), F.borders_block(dict(F.PAR, min_sites=1)), F.first_long_block(), F.count_block(4113), F.candidates_block(65)]
                         + F.edge_blocks()[:4], ids=lambda b: b["name"])
def test_from_pat_over_the_pat_rule_s_records_equals_the_rule(b):
    """No template of these blocks covers more than 64 sites, so a PAT line is a template whole."""
    recs, _ = pat.patterns(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], {"min_sites": 1})
    assert all(len(s) <= pat.MAX_SITES for _, s, _ in recs)
    sp = frag.site_positions(b["x"], b["y"], b["ref"])
    lines = pat.read_pat(pat.format("chrP", 0, recs)[0])
    want, wtot = both(b)
    got, tot = frag.from_pat(lines, sp, b["regions"], b["params"])
    assert got.tolist() == want.tolist() and tot == wtot
