"""The M-bias table on the host: csrc/mbias.c (bsc_mbias_host, bsc_mbias_format) against the Python form of the rule (bs_call_amd/mbias.py), cell
for cell and total for total, on the hand-made blocks of tests/mbias_cases.py and on seeded random ones; a block worked by hand; G(j) against
the pre-processing (bsc_prepare_templates) byte for byte; the CpG cells against the read-level CpG table's sums; the formatter and its reader;
the binding's signatures against the header; and the host form under the address and undefined-behaviour sanitizers as a stand-alone program
(integration/mbias_san.c).  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mbias_cases as K
from bs_call_amd import _lib, mbias
from bs_call_amd.abi import MISMS_INS
from bs_call_amd.caller import BscError, cpg_reads_sites_host, mbias_format_host, mbias_host, prepare_templates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()


def both(b, n_cycles=512):
    """The block through the Python rule and the host form; asserts they agree and returns (counts, totals)."""
    want, wtot = mbias.table(b["raw"], b["seq"], b["misms"], b["x"], b["y"], b["ref"], b["min_qual"], n_cycles)
    got, tot = mbias_host(b["raw"], b["seq"], b["misms"], b["x"], b["y"], b["ref"], b["min_qual"], n_cycles)
    assert tuple(tot) == tuple(wtot), (b["name"], n_cycles, tot, wtot)
    assert got.tobytes() == want.tobytes(), (b["name"], n_cycles, np.argwhere(got != want)[:4])
    assert int(got.sum()) == int(tot[2]) and int(got[:, :, 0, :, 0].sum()) == int(tot[4]) and int(got[:, :, 0, :, 1].sum()) == int(tot[5]) and tot[7] == 0
    return got, tuple(int(v) for v in tot)


def test_the_header_states_the_rule():
    for word in ("READ ", "END ", "CYCLE ", "G(j) ", "COUNTS ", "CONTEXT ", "TABLE ", "TOTALS ", "LINE ", "Hard-clipped", "Mate overlap is NOT removed",
                 "bsc_prep_params is NOT an input", "malformed", "bsc_mbias_params_default", "bsc_mbias_host", "bsc_mbias_format", "bsc_mbias_device",
                 "bsc_block_mbias_rawdev", "bsc_mbias_read", "bsc_mbias_reset", "NOT built: suggested trim bounds"):
        assert word in HEADER, word
    assert C.sizeof(_lib.MbiasParams) == 4
    p = _lib.MbiasParams(9)
    _lib.load().bsc_mbias_params_default(C.byref(p))
    assert p.n_cycles == 512 and mbias.n_cycles_of(None) == 512 and mbias.MAX_CYCLES == 1024
    assert "#define BSC_ABI_VERSION 2" in HEADER


CTYPES_OF = {"bsc_context *": C.c_void_p, "const void *": C.c_void_p, "void *": C.c_void_p, "const bsc_raw_template *": C.c_void_p,
             "const uint8_t *": C.c_void_p, "const bsc_misms *": C.c_void_p, "uint64_t *": C.c_void_p, "const uint64_t *": C.c_void_p,
             "char *": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "size_t": C.c_size_t,
             "const bsc_mbias_params *": C.POINTER(_lib.MbiasParams), "bsc_mbias_params *": C.POINTER(_lib.MbiasParams),
             "uint64_t [8]": C.POINTER(C.c_uint64)}
RESTYPE_OF = {"int": C.c_int32, "long": C.c_long, "void": None}


def test_the_binding_s_signatures_are_the_header_s():
    """Every bsc_mbias_* / bsc_block_mbias_* declaration of the header, argument by argument, against _lib.py's argtypes and restype."""
    L = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decls = re.findall(r"\b(int|long|void)\s+(bsc_(?:block_)?mbias_[a-z_]+)\s*\(([^;{]*?)\)\s*;", code)
    assert sorted(d[1] for d in decls) == sorted(s for s in _lib.EXPORTS if "mbias" in s) and len(decls) == 7
    for ret, name, args in decls:
        f = getattr(L, name)
        want = []
        for a in args.split(","):
            a = " ".join(a.split())
            m = re.match(r"^(.*?)(\w+)(\[8\])?$", a)
            kind = m.group(1).strip() + (" [8]" if m.group(3) else "")
            kind = kind.replace(" *", " *").strip()
            assert kind in CTYPES_OF, (name, a, kind)
            want.append(CTYPES_OF[kind])
        assert f.restype == RESTYPE_OF[ret], name
        got = [C.c_void_p if t is C.c_char_p else t for t in f.argtypes]
        assert got == want, (name, got, want)


def test_a_block_worked_by_hand():
    b = K.hand_worked()
    got, tot = both(b, 8)
    want = np.zeros_like(got)
    for cell, v in K.HAND_CELLS.items():
        want[cell] = v
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)
    assert tot == K.HAND_TOTALS
    # the same block with n_cycles 5: the cell at cycle 5 overflows
    got, tot = both(b, 5)
    assert tot[2:4] == (5, 1) and int(got.sum()) == 5


TARGETED = K.targeted()


@pytest.mark.parametrize("b", TARGETED, ids=[b["name"] for b in TARGETED])
def test_targeted_blocks(b):
    for n_cycles in (1, 64, 512):
        got, tot = both(b, n_cycles)
    if b["name"].startswith("malformed"):
        # 12 malformed lists, each once alone and once as the mate of a walked read; the four reads beyond their buffers but one
        assert tot[6] == 24 + 4 and tot[0] == 12 + 7 + 1
    elif b["name"].startswith("read[1] alone"):
        # three reads per (bs_strand, orientation): bs_strand 0 is not counted; bs_strand 3 (three orientations) and orientation 2 of the
        # strands 1 and 2 are skipped and counted
        assert tot[6] == 3 * 3 + 2 * 3 and tot[0] == 2 * 2 * 3
    else:
        assert tot[6] == 0
    assert tot[2] > 0 or b["name"].startswith("one read")


def test_targeted_blocks_do_what_they_are_for():
    by = {b["name"].split(",")[0].split(" and ")[0]: b for b in TARGETED}
    got, tot = both(by["one read of length 1"], 4)
    # the C at G = y is CHG through y + 1, y + 2; the G at G = x has no context base inside the block
    assert tot[:3] == (2, 2, 1) and got[0, 0, 1, 0, 0] == 1
    q = by["qualities around the window"]
    _, tq = both(q, 128)
    quals = q["seq"] >> 2
    assert tq[1] == 160 and set(np.unique(quals)) >= {19, 20, 62, 63}
    # only the bytes of quality 20, 62 and 40 can count: raising the 19s to 20 adds counts, lowering the 63s to 62 adds counts
    for frm, to in ((19, 20), (63, 62)):
        q2 = dict(q, seq=np.where(quals == frm, (q["seq"] & 3) | (to << 2), q["seq"]).astype(np.uint8))
        assert both(q2, 128)[1][2] > tq[2]
    for frm, to in ((20, 19), (62, 63)):
        q2 = dict(q, seq=np.where(quals == frm, (q["seq"] & 3) | (to << 2), q["seq"]).astype(np.uint8))
        assert both(q2, 128)[1][2] < tq[2]


@pytest.mark.parametrize("n_cycles", [1, 64, 512, 1024])
def test_long_reads_overflow(n_cycles):
    b = K.long_reads()
    got, tot = both(b, n_cycles)
    full, ftot = both(b, 1024)
    assert tot[3] > 0 and tot[2] + tot[3] == ftot[2] + ftot[3] and tot[0] == 8
    assert got.tobytes() == full[:, :, :, :n_cycles].tobytes()


def test_lengths_contention_and_end_swap():
    both(K.lengths_block())
    got, tot = both(K.contention(300), 64)
    assert tot == (300, 300 * 64, 300 * 32, 0, 300 * 32, 0, 0, 0) and (got[0, 0, 0, 0:64:2, 0] == 300).all()
    # END: orientation swaps the two ends and nothing else; CYCLE: read[1] runs backwards
    b = K.random_block(5, 200, strands=(1, 2), orients=(0,))
    c0, t0 = both(b)
    r = b["raw"].copy()
    r["orientation"] = 1
    c1, t1 = both(dict(b, raw=r))
    assert t0 == t1 and c1[0].tobytes() == c0[1].tobytes() and c1[1].tobytes() == c0[0].tobytes() and c0[0].sum() and c0[1].sum()


@pytest.mark.parametrize("seed,nr", [(1, 1), (2, 63), (3, 400), (4, 1500)])
def test_random_blocks(seed, nr):
    b = K.random_block(seed, nr)
    got, tot = both(b)
    if nr >= 400:
        assert tot[0] > nr and tot[6] > nr // 8 and tot[2] > 100 and got[0].sum() and got[1].sum()
    # adding: a second call into the same arrays doubles them
    again, atot = mbias_host(b["raw"], b["seq"], b["misms"], b["x"], b["y"], b["ref"], b["min_qual"], 512, counts=got.copy(), totals=np.array(tot, np.uint64))
    assert (again == 2 * got).all() and tuple(atot) == tuple(2 * v for v in tot)
    # totals may be NULL
    L = _lib.load()
    c2 = np.zeros_like(got)
    mp = _lib.MbiasParams(512)
    assert L.bsc_mbias_host(b["raw"].ctypes.data, len(b["raw"]), b["seq"].ctypes.data, len(b["seq"]), b["misms"].ctypes.data, len(b["misms"]), b["x"], b["y"],
                            b["ref"].ctypes.data, b["min_qual"], C.byref(mp), c2.ctypes.data, None) == 0
    assert c2.tobytes() == got.tobytes()


def test_refusals():
    b = K.hand_worked()
    for n in (0, 1025, 0xFFFFFFFF):
        counts, totals = np.full((2, 2, 3, 1, 2), 7, np.uint64), np.full(8, 7, np.uint64)
        with pytest.raises(BscError):
            mbias_host(b["raw"], b["seq"], b["misms"], b["x"], b["y"], b["ref"], 20, _lib.MbiasParams(n), counts=counts, totals=totals)
        assert (counts == 7).all() and (totals == 7).all()
        with pytest.raises(ValueError):
            mbias.n_cycles_of(n)
    with pytest.raises(BscError):
        mbias_host(b["raw"], b["seq"], b["misms"], b["y"] + 1, b["y"], b["ref"], 20, 8)


def _clean(seed, nr):
    return K.random_block(seed, nr, strands=(1, 2), orients=(0, 1))


@pytest.mark.parametrize("seed", [11, 12])
def test_g_of_j_against_the_pre_processing(seed):
    """Trims 0, mates that do not overlap: every byte with a G lies in the prepared read at G - pos'[k], and the prepared bytes that are not
    padded deletions are exactly the raw bytes with a G."""
    b = _clean(seed, 400)
    tpl, pseq, _ = prepare_templates(b["raw"], b["seq"], b["misms"])
    n_bytes = n_indel = n_clip = 0
    for t, p in zip(b["raw"], tpl):
        for k in range(2):
            ln = int(t["len"][k])
            if not ln:
                assert int(p["len"][k]) == 0
                continue
            entries = b["misms"][int(t["misms_off"][k]) : int(t["misms_off"][k]) + int(t["n_misms"][k])]
            g = mbias.genome_map(t["pos"][k], ln, entries)
            assert g is not None
            raw_bytes = b["seq"][int(t["off"][k]) : int(t["off"][k]) + ln]
            prepared = pseq[int(p["off"][k]) : int(p["off"][k]) + int(p["len"][k])]
            j = np.flatnonzero(g >= 0)
            at = g[j] - int(p["pos"][k])
            assert (at >= 0).all() and (at < len(prepared)).all() and len(set(at.tolist())) == len(at)
            assert (prepared[at] == raw_bytes[j]).all()
            pads = int(entries["size"][entries["type"] == MISMS_INS].sum())
            assert len(j) == len(prepared) - pads
            rest = np.ones(len(prepared), bool)
            rest[at] = False
            assert (prepared[rest] == 0).all()
            n_bytes += len(j)
            n_indel += pads > 0 or len(j) < ln
            n_clip += int((entries["type"] == 3).any())
    assert n_bytes > 10_000 and n_indel > 50 and n_clip > 50


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_cpg_cells_are_the_read_level_table_s_sums(seed):
    """The same COUNTS, site p <= y, nothing left of x: the sum of the CpG cells over ends, strands and cycles is (sum of m, sum of u) of
    bsc_cpg_reads_sites_host over the prepared templates of the same block."""
    b = _clean(seed, 600)
    tpl, pseq, _ = prepare_templates(b["raw"], b["seq"], b["misms"])
    _, _, rtot = cpg_reads_sites_host(tpl, pseq, b["x"], b["y"], b["ref"], b["min_qual"], {"min_sites": 1, "min_cov": 1})
    got, tot = both(b, 1024)
    assert tot[3] == 0 and (tot[4], tot[5]) == (rtot[1], rtot[2]) and tot[4] > 50 and tot[5] > 50
    assert (int(got[:, :, 0, :, 0].sum()), int(got[:, :, 0, :, 1].sum())) == (rtot[1], rtot[2])


def test_formatter_and_reader():
    counts, _ = both(K.random_block(31, 300), 64)
    text, n = mbias_format_host(counts)
    assert text == mbias.format_table(counts) and text.startswith(mbias.HEADER) and n == len(text)
    assert mbias.read_table(text, 64).tobytes() == counts.tobytes()
    # L(e) with a zero line inside the range, an end with no count, no count at all
    c = np.zeros((2, 2, 3, 16, 2), np.uint64)
    assert mbias_format_host(c) == (mbias.HEADER, len(mbias.HEADER)) and mbias.HEADER == mbias.format_table(c)
    c[1, 0, 2, 4, 1] = 12345678901234567890
    c[1, 1, 0, 0, 0] = 3
    text = mbias_format_host(c)[0]
    assert text == mbias.format_table(c)
    lines = text.split(b"\n")[1:-1]
    assert len(lines) == 6 * 5 and all(ln.startswith(b"2\t") for ln in lines) and b"2\tC2T\tCHH\t5\t0\t12345678901234567890" in lines
    assert b"2\tC2T\tCHH\t3\t0\t0" in lines and lines[0] == b"2\tC2T\tCpG\t1\t0\t0"
    assert mbias.read_table(text, 16).tobytes() == c.tobytes()
    c[0, 1, 1, 15, 0] = 1
    text = mbias_format_host(c)[0]
    assert text == mbias.format_table(c) and text.count(b"\n") == 1 + 6 * 16 + 6 * 5
    # cap one short: the need, nothing written (the wrapper checks the bytes); the exact room
    assert mbias_format_host(c, cap=len(text) - 1) == (None, len(text))
    assert mbias_format_host(c, cap=0) == (None, len(text))
    assert mbias_format_host(c, cap=len(text)) == (text, len(text))
    L = _lib.load()
    assert L.bsc_mbias_format(c.ctypes.data, C.byref(_lib.MbiasParams(0)), None, 0) < 0
    assert L.bsc_mbias_format(None, C.byref(_lib.MbiasParams(16)), None, 0) < 0


def test_host_form_under_sanitizers(tmp_path):
    """make mbias-san: integration/mbias_san.c + csrc/mbias.c under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "mbias_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "mbias_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "mbias.c"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
    assert "mbias-san:" in open(os.path.join(ROOT, "Makefile")).read()
