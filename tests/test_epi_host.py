"""The epiallele table on the host: csrc/epi.c (bsc_epi_windows_host, bsc_epi_format) against the Python form of the rule
(bs_call_amd/epialleles.py) and the hand tallies of tests/epi_cases.py, record for record and total for total; the formatter and the table
reader; the window counts against the read-level CpG table of the same block; and the host form under the address and undefined-behaviour
sanitizers as a stand-alone program (integration/epi_san.c).  No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpg_reads_cases as K
import epi_cases as E
from bs_call_amd import _lib, epialleles
from bs_call_amd.caller import BscError, cpg_reads_sites_host, epi_format_host, epi_windows_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()


def both(b, cap=None):
    """The block through the Python rule and the host form; asserts they agree and returns (records, totals)."""
    want, wtot = epialleles.windows(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    got, n, tot = epi_windows_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"], cap=cap)
    assert n == len(want) and tot == wtot, (b["name"], n, len(want), tot, wtot)
    assert got.tobytes() == want[: len(got)].tobytes(), b["name"]
    return want, wtot


def test_the_header_states_the_rule():
    for word in ("WINDOW", "PATTERN(t, i)", "BSC_EPI_K", "bsc_epi_window", "bsc_epi_params", "bsc_epi_windows_host", "bsc_epi_format", "bsc_epi_device",
                 "bsc_epi_text_device", "bsc_block_epi_kept", "bsc_epi_stream_read", "bsc_epi_stream_detach"):
        assert word in HEADER, word
    assert C.sizeof(_lib.EpiParams) == 8 and epialleles.WINDOW.itemsize == 72 and epialleles.K == 4
    p = _lib.EpiParams(9, 9)
    _lib.load().bsc_epi_params_default(C.byref(p))
    assert (p.min_cov, p.reserved) == (10, 0)


def test_a_block_worked_by_hand():
    """tests/epi_cases.py: hand_block's docstring has the tally, template by template and window by window."""
    b = E.hand_block()
    assert tuple(epialleles.site_positions(b["x"], b["y"], b["ref"])) == E.HAND_SITES
    recs, tot = both(b)
    assert E.as_tuples(recs) == E.HAND_RECORDS and tot == E.HAND_TOTALS
    assert epialleles.format("chrE", recs, E.PAR) == (E.HAND_TABLE, 4)
    assert epi_format_host("chrE", recs, E.PAR) == (E.HAND_TABLE, 4)
    first_two = b"".join(E.HAND_TABLE.splitlines(True)[:2])
    assert epialleles.format("chrE", recs, {"min_cov": 3}) == (first_two, 2) == epi_format_host("chrE", recs, {"min_cov": 3})  # n >= 3
    assert epialleles.format("chrE", recs) == (b"", 0) == epi_format_host("chrE", recs)  # the default asks for ten
    names, back = epialleles.read_table(E.HAND_TABLE)
    assert names == [b"chrE"] * 4 and back.tobytes() == recs.tobytes()


def test_the_anchor_on_the_read_level_table_s_hand_block():
    """K.hand_block (sites 103, 107, 110, 120, 125): T1 alone has four states in a row, M U M M U: w0 = (103 .. 120) MUMM = 13,
    w1 = (107 .. 125) UMMU = 6."""
    b = dict(K.hand_block(), params=E.PAR)
    recs, tot = both(b)
    assert E.as_tuples(recs) == E.ANCHOR_RECORDS and tot == E.ANCHOR_TOTALS
    assert epialleles.format("chrT", recs, E.PAR) == (E.ANCHOR_TABLE, 2) == epi_format_host("chrT", recs, E.PAR)
    assert E.ANCHOR_TABLE.startswith(b"chrT\t102\t121\t1\t1\t") and b"\nchrT\t106\t126\t1\t1\t" in E.ANCHOR_TABLE


@pytest.mark.parametrize("b", E.targeted_blocks() + [E.long_read_block(), E.contention_block(), E.contention_block(spread=True)], ids=lambda b: b["name"])
def test_host_form_equals_the_python_rule_on_the_targeted_blocks(b):
    recs, tot = both(b)
    assert tot[0] == len(recs) and tot[5:] == (0, 0, 0) and tot[1] == int(recs["c"].sum())
    name, x = b["name"], b["x"]
    if name.startswith("S = "):
        S = int(name[4:])
        assert len(recs) == max(S - 3, 0)
        if S == 4:
            assert E.as_tuples(recs) == [E.rec(x + 10, 36, c11=1, c6=1)]  # MMUM and UMMU; the short read holds three sites
        if S == 5:
            assert E.as_tuples(recs) == [E.rec(x + 10, 36, c11=1, c6=1), E.rec(x + 22, 36, c5=1, c11=1, c15=1)]  # ... and here sites 1 .. 4
    if "tile" in name:
        s = [int(recs[0]["pos"]), int(recs[1]["pos"])]
        assert len(recs) == 2 and s[0] + int(recs[0]["span"]) < s[1] + int(recs[1]["span"])
        # w0: the three full reads, the two reads that span exactly it, and the back-to-back mates where they hold all four
        assert int(recs[0]["c"][13]) == 1 and int(recs[0]["c"][4]) == 1 and int(recs[0]["c"][0]) == 1 and int(recs[0]["c"].sum()) >= 5
        assert int(recs[1]["c"][15]) >= 2  # the all-M read and the read over the second window alone
    if name == "lanes 0, 62, 63":
        assert [int(r["pos"]) for r in recs] == [x, x + 62] and [int(r["span"]) for r in recs] == [190, 193]
        assert [int(v) for v in recs[1]["c"]] == E.rec(0, 0, c10=1, c3=1, c15=1, c0=1)[2]  # UMUM = 2+8, MMUU = 1+2, the C2T and the G2A read over it alone
        assert [int(v) for v in recs[0]["c"]] == E.rec(0, 0, c5=1, c6=1, c15=1)[2]  # MUMU, UMMU, the G2A read that ends on lane 62's G
    if name == "a site at y":
        assert E.as_tuples(recs) == [E.rec(x + 5, 45, c3=1, c15=1), E.rec(x + 10, 89, c9=1)]  # the G2A reads have no state at y
    if name.startswith("a stateless site"):
        # the template whose site j has no state leaves window 0 for j < 4 ... and fills window 1 only for j = 0
        assert E.as_tuples(recs) == [E.rec(x + 10, 30), E.rec(x + 20, 30, c10=1, c3=1)] and tot[4] == 8
    if name == "mates":
        assert E.as_tuples(recs) == E.MATES_RECORDS and tot == (1, 4, 4, 12, 4, 0, 0, 0)
    if name == "long read":
        assert len(recs) == 2497 and (recs["span"] == 6).all() and tot[2] == 3 and tot[1] > 6000
    if name == "contention, one code":
        assert E.as_tuples(recs) == [E.rec(53, 18, c5=5000)] and tot == (1, 5000, 5000, 10000, 5000, 0, 0, 0)
    if name == "contention, 16 codes":
        assert E.as_tuples(recs) == [(53, 18, [313] * 8 + [312] * 8)] and tot[:3] == (1, 5000, 5000)


@pytest.mark.parametrize("n_pos,seed", E.TILE_EDGE_BLOCKS)
def test_host_form_equals_the_python_rule_around_a_tile(n_pos, seed):
    b = E.dense_block(seed, n_pos, 60)
    _, _, tot = epi_windows_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, b["params"])
    assert tot[1] > 0, "the seed must give a pattern by the host form alone"
    both(b)


@pytest.fixture(scope="module")
def big():
    b = E.big_block()
    recs, n, tot = epi_windows_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, b["params"])
    assert int((recs["c"].sum(axis=1) > 0).sum()) >= 1000, "the seed must give patterns in 1 000 windows by the host form alone"
    return b, recs, tot


def test_host_form_equals_the_python_rule_on_20003_positions(big):
    b, recs, tot = big
    want, wtot = both(b)
    assert want.tobytes() == recs.tobytes() and wtot == tot
    assert all(v > 0 for v in tot[:5]) and tot[2] <= tot[4] < len(b["tpl"]) and (recs["c"].sum(axis=0) > 0).all()  # every code occurs
    thin, _ = both(E.dense_block(8, 2003, 20))
    assert (thin["c"].sum(axis=1) == 0).any() and (thin["c"].sum(axis=1) > 0).any()  # a window no template reads is still a window
    # the room rule: records beyond cap are counted, not stored
    both(b, cap=len(recs) - 1)
    both(b, cap=0)
    # a read outside the buffer is absent
    t2 = b["tpl"].copy()
    k = int(np.flatnonzero(t2["len"][:, 0] > 0)[5])
    t2["off"][k][0] = len(b["seq"])
    both(dict(b, tpl=t2))
    with pytest.raises(BscError):
        epi_windows_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, {"reserved": 1})
    with pytest.raises(ValueError):
        epialleles.windows(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, {"reserved": 1})
    with pytest.raises(ValueError):
        epialleles.windows(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, {"min_sites": 3})


def extreme_records():
    """Records made by hand: c = 2^32 - 1 in one code and in all sixteen (n = 16 (2^32 - 1), eleven digits), pos at 1 and at 2^32 - 2 - span."""
    top = 0xFFFFFFFF
    recs = np.zeros(6, epialleles.WINDOW)
    recs[0] = (1, 6, [0] * 16)
    recs[1] = (1, 6, [0] * 9 + [top] + [0] * 6)
    recs[2] = (1, 60, [top] * 16)
    recs[3] = (top - 1 - 6, 6, [top] * 16)
    recs[4] = (top - 1 - 4000, 4000, [1] + [0] * 15)
    recs[5] = (12345, 100, list(range(16)))
    return recs


def test_formatter_equals_the_python_formatter():
    rng = np.random.default_rng(16)
    recs = np.zeros(400, epialleles.WINDOW)
    recs["pos"] = (10 ** rng.integers(0, 9, len(recs)) * rng.integers(1, 10, len(recs))).clip(1, 0x7FFFFFFF)
    recs["span"] = rng.integers(6, 5000, len(recs))
    recs["c"] = np.where(rng.random((len(recs), 16)) < 0.6, 0, 10 ** rng.integers(0, 10, (len(recs), 16)) * rng.integers(1, 10, (len(recs), 16))).clip(0, 0xFFFFFFFF)
    recs["c"][::7] = 0  # no line whatever min_cov
    recs["c"][3::7] = 0
    recs["c"][3::7, 11] = 1  # a line at min_cov 1 only
    recs[:6] = extreme_records()
    for name in ("c", "chr1", "x" * 255):
        for mc in (0, 1, 2, 10, 0xFFFFFFFF):
            par = {"min_cov": mc}
            want, lines = epialleles.format(name, recs, par)
            assert epi_format_host(name, recs, par) == (want, lines)
            assert epi_format_host(name, recs, par, cap=len(want) - 1) == (None, len(want))  # the need, nothing written
            names, back = epialleles.read_table(want)
            keep = recs[recs["c"].astype(np.int64).sum(axis=1) >= max(1, mc)]
            assert len(back) == lines == len(keep) > 0 and set(names) == {name.encode()} and back.tobytes() == keep.tobytes()
    assert epialleles.format("chr1", recs, {"min_cov": 0})[0] == epialleles.format("chr1", recs, {"min_cov": 1})[0]
    top = b"4294967295"
    assert epialleles.format("chr1", recs[2:4], E.PAR)[0] == (b"chr1\t0\t62\t68719476720\t16" + (b"\t" + top) * 16 + b"\n"
                                                              b"chr1\t4294967287\t4294967295\t68719476720\t16" + (b"\t" + top) * 16 + b"\n")
    assert epialleles.format("chr1", recs[1:2], E.PAR)[0] == b"chr1\t0\t8\t4294967295\t1" + b"\t0" * 9 + b"\t" + top + b"\t0" * 6 + b"\n"
    assert len(epialleles.format("x" * 255, recs[3:4], E.PAR)[0]) == 255 + 214  # the longest line
    assert epialleles.format("chr1", recs[:0]) == (b"", 0) and epi_format_host("chr1", recs[:0]) == (b"", 0)
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(ValueError):
            epialleles.format(bad, recs)
        with pytest.raises(BscError):
            epi_format_host(bad, recs)
    with pytest.raises(BscError):
        epi_format_host("chr1", recs, {"min_cov": 1, "reserved": 2})
    with pytest.raises(ValueError):
        epialleles.format("chr1", recs, {"reserved": 2})
    with pytest.raises(ValueError):
        epialleles.read_table(b"chr1\t1\t2\n")
    with pytest.raises(ValueError):
        epialleles.read_table(b"chr1\t0\t8\t2\t1" + b"\t0" * 15 + b"\t1\n")  # n does not fit


def test_the_derived_statistics():
    c = [0] * 16
    assert math.isnan(epialleles.epipolymorphism(c)) and math.isnan(epialleles.entropy(c))
    c[5] = 7
    assert epialleles.epipolymorphism(c) == 0.0 and epialleles.entropy(c) == 0.0
    assert epialleles.epipolymorphism([3] * 16) == pytest.approx(1 - 1 / 16) and epialleles.entropy([3] * 16) == pytest.approx(4.0)
    assert epialleles.epipolymorphism([1, 1] + [0] * 14) == pytest.approx(0.5) and epialleles.entropy([1, 1] + [0] * 14) == pytest.approx(1.0)
    assert epialleles.entropy([2, 1, 1] + [0] * 13) == pytest.approx(1.5)


def pair_sums(c):
    """For j = 0, 1, 2: the counts grouped by bits (j, j + 1) as (mm, mu, um, uu) of sites i + j and i + j + 1."""
    out = []
    for j in range(3):
        g = {"mm": 0, "mu": 0, "um": 0, "uu": 0}
        for code in range(16):
            a, b = (code >> j) & 1, (code >> (j + 1)) & 1
            g[("m" if a else "u") + ("m" if b else "u")] += int(c[code])
        out.append(g)
    return out


def check_against_the_read_level_table(b, equal=False):
    recs, n, tot = epi_windows_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], E.PAR)
    sites, ns, stot = cpg_reads_sites_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], {"min_sites": 4, "min_cov": 1})
    assert n == max(ns - 3, 0) and tot[4] == stot[5]  # k_t >= 4 is the read-level table's ELIGIBLE at min_sites 4
    for i, w in enumerate(recs):
        assert int(w["pos"]) == int(sites[i]["pos"]) and int(w["pos"]) + int(w["span"]) == int(sites[i + 3]["pos"])
        nobs = int(w["c"].astype(np.int64).sum())
        for j in range(4):
            cov = int(sites[i + j]["m"]) + int(sites[i + j]["u"])
            assert nobs <= cov if not equal else nobs == cov, (b["name"], i, j)
        for j, g in enumerate(pair_sums(w["c"])):
            for f in ("mm", "mu", "um", "uu"):
                assert g[f] <= int(sites[i + j][f]) if not equal else g[f] == int(sites[i + j][f]), (b["name"], i, j, f)
    return recs


def test_window_counts_against_the_read_level_table(big):
    n_obs = 0
    for b in [E.hand_block(), dict(K.hand_block(), params=E.PAR), E.long_read_block(), big[0]] + E.targeted_blocks():
        n_obs += int(check_against_the_read_level_table(b)["c"].sum())
    assert n_obs > 30_000
    # a block where every template covers every site: the two tables say the same
    x, s = 300, [310, 322, 341, 350, 377, 391]
    rng = np.random.default_rng(6)
    rows = []
    for k in range(40):
        st = {p: "MU"[int(v)] for p, v in zip(s, rng.integers(0, 2, len(s)))}
        rows.append((1, K._c2t(x, 100, st), None) if k % 2 else (2, K._g2a(x, 100, st), None))
    recs = check_against_the_read_level_table(E.block("every template covers every site", rows, x, x + 99, K.ref_with_sites(x, 100, s)), equal=True)
    assert len(recs) == 3 and (recs["c"].sum(axis=1) == 40).all()


def test_host_form_under_sanitizers(tmp_path):
    """make epi-san: integration/epi_san.c + csrc/epi.c under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "epi_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "epi_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "epi.c"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
