"""The read-level CpG concordance table on the host: csrc/cpgreads.c (bsc_cpg_reads_sites_host, bsc_cpg_reads_format) against the Python form
of the rule (bs_call_amd/cpgreads.py) on the hand-made blocks of tests/cpg_reads_cases.py and on seeded random templates, with the count,
the totals and the room rule; a block worked by hand; the formatter and the table reader; and the host form under the address and
undefined-behaviour sanitizers as a stand-alone program (integration/cpg_reads_san.c).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpg_reads_cases as K
from bs_call_amd import _lib, cpgreads
from bs_call_amd.caller import BscError, cpg_reads_format_host, cpg_reads_sites_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()


def both(b, cap=None):
    """The block through the Python rule and the host form; asserts they agree and returns (records, totals)."""
    want, wtot = cpgreads.sites(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    got, n, tot = cpg_reads_sites_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"], cap=cap)
    assert n == len(want) and tot == wtot, (b["name"], n, len(want), tot, wtot)
    assert got.tobytes() == want[: len(got)].tobytes(), b["name"]
    return want, wtot


def test_the_header_states_the_rule():
    for word in ("COUNTS", "SITE", "BYTE(t, q)", "STATE(t, s)", "RECORD", "TOTALS", "LINE", "bsc_cpg_reads_site", "bsc_cpg_reads_params",
                 "bsc_cpg_reads_sites_host", "bsc_cpg_reads_format", "bsc_cpg_reads_device", "bsc_cpg_reads_text_device", "bsc_block_cpg_reads_kept",
                 "bsc_cpg_reads_stream_read", "bsc_cpg_reads_stream_detach"):
        assert word in HEADER, word
    assert C.sizeof(_lib.CpgReadsParams) == 8 and cpgreads.SITE.itemsize == 40
    p = _lib.CpgReadsParams(9, 9)
    _lib.load().bsc_cpg_reads_params_default(C.byref(p))
    assert (p.min_sites, p.min_cov) == (4, 1)


def test_a_block_worked_by_hand():
    """Positions 101 .. 130, sites 103, 107, 110, 120, 125 (dist 4, 3, 10, 5, 0), min_sites 3, seven templates:
      T1 C2T over all:            M U M M U   eligible, discordant   pairs MU UM MM MU
      T2 C2T 103 .. 110:          M M M       eligible               pairs MM MM, none behind 110 (120 lies behind its end)
      T3 G2A 104 .. 111:          M U M       eligible, discordant   pairs MU UM
      T4 C2T 101 .. 105 + 118 .. 127: U . . U M  eligible, discordant  no pair at 103 (107 is in the gap), UM at 120
      T5 C2T, quality 19 at 107:  no state
      T6 G2A 119 .. 126:          . . . U M   two states: not eligible; pair UM at 120
      T7 not converted:           ignored
    103: m 3 (T1 T2 T3) u 1 (T4) e 4 d 3 (T1 T3 T4) mm 1 (T2) mu 2 (T1 T3)
    107: m 1 (T2) u 2 (T1 T3) e 3 d 2 mm 1 (T2) um 2 (T1 T3)
    110: m 3 u 0 e 3 d 2 mm 1 (T1)
    120: m 1 (T1) u 2 (T4 T6) e 2 (T1 T4) d 2 mu 1 (T1) um 2 (T4 T6)
    125: m 2 (T4 T6) u 1 (T1) e 2 d 2
    totals: 5 sites, 10 M, 6 U, 10 pairs, 5 templates with a state, 4 eligible, 3 discordant."""
    b = K.hand_block()
    assert tuple(cpgreads.site_positions(b["x"], b["y"], b["ref"])) == K.HAND_SITES
    recs, tot = both(b)
    assert [tuple(int(v) for v in r) for r in recs] == K.HAND_RECORDS
    assert tot == K.HAND_TOTALS
    assert cpgreads.format("chrT", recs, b["params"]) == (K.HAND_TABLE, 5)
    assert cpg_reads_format_host("chrT", recs, b["params"]) == (K.HAND_TABLE, 5)
    assert cpgreads.format("chrT", recs, {"min_sites": 3, "min_cov": 4}) == (K.HAND_TABLE.splitlines(True)[0], 1)  # m + u >= 4: 103 alone
    assert cpgreads.double_covered(b["tpl"], b["seq"], b["x"], b["y"], 20) == 0


@pytest.mark.parametrize("b", K.targeted_blocks() + [K.long_read_block(), K.contention_block(300)], ids=lambda b: b["name"])
def test_host_form_equals_the_python_rule_on_the_targeted_blocks(b):
    recs, tot = both(b)
    assert tot[0] == len(recs) and tot[7] == 0
    name = b["name"]
    by_pos = {int(r["pos"]): r for r in recs}
    x = b["x"]
    if name == "lanes 0, 62, 63":
        assert sorted(by_pos) == [x, x + 62, x + 127]
        assert (int(by_pos[x + 127]["m"]), int(by_pos[x + 127]["u"])) == (3, 3)  # the C2T reads: M M U, the G2A reads: U M U
        assert (int(by_pos[x + 62]["m"]), int(by_pos[x + 62]["u"])) == (3, 1)
    if name.startswith("next"):
        r = by_pos[x + 70]  # its NEXT is two tiles on
        assert int(r["dist"]) == 130 and int(r["mm"]) + int(r["mu"]) + int(r["um"]) + int(r["uu"]) == 4
        assert int(by_pos[x + 5]["mm"] + by_pos[x + 5]["mu"] + by_pos[x + 5]["um"] + by_pos[x + 5]["uu"]) == 2  # the third template has none
        five = "five" in name
        assert int(by_pos[x + 280]["m"] + by_pos[x + 280]["u"]) == (3 if five else 0)  # beyond the shorter reads' end
    if name == "mates":
        assert int(by_pos[x + 30]["m"]) == 1 and int(by_pos[x + 30]["u"]) == 3  # gap: none; read 0's G: none; read 1 where read 0 fails: U
        assert cpgreads.double_covered(b["tpl"], b["seq"], b["x"], b["y"], 20) == 3  # the last three pairs overlap
    if name.startswith("qualities"):
        assert [int(r["m"]) for r in recs] == [0, 0, 1, 1, 0] and [int(r["u"]) for r in recs] == [1, 1, 2, 2, 1]
    if name == "edges":
        assert sorted(by_pos) == [1, 33, 70] and int(by_pos[70]["m"]) == 1 and int(by_pos[70]["u"]) == 1 and int(by_pos[1]["u"]) == 1
    if name.startswith("min_sites"):
        ms = b["params"]["min_sites"]
        assert tot[5] == 3 and tot[4] == (6 if ms > 1 else 3) and tot[6] == (1 if ms > 1 else 0)
    if name == "long read":
        n_a, n_b = int((recs["pos"] < x + 100).sum()), int((recs["pos"] >= x + 4800).sum())  # the sites under the two mates of the pair
        assert tot[0] == 80 and tot[1] + tot[2] == 160 + n_a + n_b and tot[3] == 2 * 79 + max(n_a - 1, 0) + max(n_b - 1, 0) and n_a + n_b > 2
    if name == "contention":
        assert [tuple(int(v) for v in r) for r in recs] == [(x + 3, 6, 300, 0, 300, 300, 0, 300, 0, 0), (x + 9, 0, 0, 300, 300, 300, 0, 0, 0, 0)]


@pytest.mark.parametrize("seed,n_pos,nr", [(1, 63, 40), (2, 64, 40), (3, 65, 40), (4, 127, 60), (5, 128, 60), (6, 129, 60), (7, 2003, 700)])
def test_host_form_equals_the_python_rule_on_random_templates(seed, n_pos, nr):
    b = K.random_block(seed, n_pos, nr)
    recs, tot = both(b)
    if n_pos == 2003:
        assert all(v > 0 for v in tot[:7]) and tot[6] < tot[5] < tot[4] < nr, tot
        for f in ("m", "u", "e", "d", "mm", "mu", "um", "uu"):
            assert recs[f].max() > 0, f
        thin, _ = both(K.random_block(8, 2003, 20))
        assert (thin["m"] + thin["u"] == 0).any() and (thin["m"] + thin["u"] > 0).any()  # a site no template covers is still a record
        # the room rule: records beyond cap are counted, not stored
        both(b, cap=len(recs) - 1)
        both(b, cap=0)
        # a read outside the buffer is absent
        t2 = b["tpl"].copy()
        t2["off"][5][0] = len(b["seq"])
        both(dict(b, tpl=t2))
        for bad in ({"min_sites": 0},):
            with pytest.raises(BscError):
                cpg_reads_sites_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, bad)
            with pytest.raises(ValueError):
                cpgreads.sites(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, bad)
        with pytest.raises(ValueError):
            cpgreads.sites(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], 20, {"min_site": 3})


def test_formatter_equals_the_python_formatter():
    rng = np.random.default_rng(12)
    recs = np.zeros(400, cpgreads.SITE)
    for f in cpgreads.SITE.names:  # numbers of 1 .. 10 digits
        recs[f] = (10 ** rng.integers(0, 10, len(recs)) * rng.integers(1, 10, len(recs))).clip(1, 0xFFFFFFFF)
    recs["m"][::7] = 0
    recs["u"][::7] = 0  # no line whatever min_cov
    recs["u"][3::7] = 0
    recs["m"][3::7] = 1  # a line at min_cov 1 only
    recs[5] = (0xFFFFFFFF,) * 10
    recs[6] = (1, 0, 1, 0, 0, 0, 0, 0, 0, 0)
    for name in ("c", "chr1", "x" * 255):
        for mc in (0, 1, 2, 0xFFFFFFFF):
            par = {"min_sites": 4, "min_cov": mc}
            want, lines = cpgreads.format(name, recs, par)
            assert cpg_reads_format_host(name, recs, par) == (want, lines)
            assert cpg_reads_format_host(name, recs, par, cap=len(want) - 1) == (None, len(want)) or not want
            names, back = cpgreads.read_table(want)
            keep = recs[(recs["m"].astype(np.int64) + recs["u"]) >= max(1, mc)]
            assert len(back) == lines == len(keep) and set(names) <= {name.encode()}
            if mc != 0xFFFFFFFF:
                ok = keep["pos"] != 0xFFFFFFFF  # (end = 2^32 does not fit the record's pos on the way back)
                assert back[ok].tobytes() == keep[ok].tobytes()
    assert cpgreads.format("chr1", recs, {"min_cov": 0})[0] == cpgreads.format("chr1", recs, {"min_cov": 1})[0]
    assert cpgreads.format("chr1", recs[5:6])[0] == b"chr1\t4294967294\t4294967296" + b"\t4294967295" * 9 + b"\n"
    assert cpgreads.format("chr1", recs[:0]) == (b"", 0) and cpg_reads_format_host("chr1", recs[:0]) == (b"", 0)
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(ValueError):
            cpgreads.format(bad, recs)
        with pytest.raises(BscError):
            cpg_reads_format_host(bad, recs)
    with pytest.raises(ValueError):
        cpgreads.read_table(b"chr1\t1\t2\n")


def test_host_form_under_sanitizers(tmp_path):
    """make cpg-reads-san: integration/cpg_reads_san.c + csrc/cpgreads.c under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "cpg_reads_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "cpg_reads_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "cpgreads.c"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
