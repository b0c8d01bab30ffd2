"""The variant-only call set on the host: csrc/variants.c (bsc_variants_select_recs) against the Python form of the rule
(bs_call_amd/variants.py) on the same random records, with its room rule and NULL totals; the independent stream checker of the GPU tests
(tests/variants_ref.py) on a hand-made stream of three records, in both formats; and the host form under the address and
undefined-behaviour sanitizers as a stand-alone program (integration/variants_san.c).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bs_call_amd as B
import variants_ref as VR
from bs_call_amd import _lib, variants
from bs_call_amd.abi import VCF_REC
from variants_cases import PARAMS, random_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bscall_amd.h")).read()


def host_select(recs, par, cap=None, totals=True):
    L = _lib.load()
    recs = np.ascontiguousarray(recs)
    p = _lib.VarParams(**par)
    cap = len(recs) if cap is None else cap
    out = np.full(max(cap, 1) + 1, 0x5A, dtype=np.uint8).repeat(128).view(VCF_REC)
    n_out, tot = C.c_uint64(77), (C.c_uint64 * 10)(*([99] * 10))
    rc = L.bsc_variants_select_recs(recs.ctypes.data if len(recs) else None, len(recs), C.byref(p), out.ctypes.data, cap, C.byref(n_out),
                                    tot if totals else None)
    return rc, out, int(n_out.value), tuple(int(v) for v in tot)


def test_the_header_states_the_rule():
    for word in ("VARIANT", "PARAMS", "SELECTED", "TOTALS", "STREAM", "bsc_var_params", "bsc_variants_select_recs", "bsc_variants_sites_device",
                 "bsc_block_variants_kept", "bsc_variants_stream_read", "bsc_variants_stream_detach", "bsc_block_variants_csi_kept"):
        assert word in HEADER, word
    assert C.sizeof(_lib.VarParams) == 16
    p = _lib.VarParams(5, 6, 7, 8)
    _lib.load().bsc_var_params_default(C.byref(p))
    assert (p.min_phred, p.pass_only, p.known_only, p.reserved) == (0, 0, 0, 0)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4113])
def test_host_form_equals_the_python_rule(n):
    rng = np.random.default_rng(9000 + n)
    for present in ("some", "none", "all", "first", "last") if n else ("some",):
        recs = random_records(rng, n, present)
        for par in PARAMS:
            idx = variants.select(recs, par)
            want = recs[idx]
            rc, out, n_out, tot = host_select(recs, par)
            assert rc == 0 and n_out == len(idx) and out[:n_out].tobytes() == want.tobytes(), (present, par)
            assert tot == variants.totals(want), (present, par)
            assert (out[n_out:].view(np.uint8) == 0x5A).all()
            if present == "all" and not par:
                assert n_out == n
            if present in ("first", "last") and not par:
                assert n_out == (n + 63) // 64
            if present == "none":
                assert tot == (0,) * 10
    if n == 4113:
        recs = random_records(rng, n)
        idx = variants.select(recs)
        t = variants.totals(recs[idx])
        assert n // 5 < len(idx) < n // 2 and all(v > 0 for v in t), t  # about a third; every counter counts
        assert t[1] + t[2] == t[0] and t[7] + t[8] < t[1] and t[6] < min(t[4], t[5])
        core = recs[idx]["core"]
        assert (core["gt"] > 9).any() and (~np.isin(recs[idx].view(np.uint8).reshape(-1, 128)[:, 12], list(b"ACGT"))).any()
        # the room rule: one short -> the need, the totals, nothing written; NULL totals
        rc, out, n_out, tot = host_select(recs, {}, cap=len(idx) - 1)
        assert rc == -1 and n_out == len(idx) and tot == t and (out.view(np.uint8) == 0x5A).all()
        assert b"cap" in _lib.load().bsc_last_error()
        rc, out, n_out, tot = host_select(recs, {}, totals=False)
        assert rc == 0 and n_out == len(idx) and tot == (99,) * 10 and out[:n_out].tobytes() == recs[idx].tobytes()
        rc, _, n_out, _ = host_select(recs, {"reserved": 1})
        assert rc == -1 and n_out == 0 and b"reserved" in _lib.load().bsc_last_error()
        # the per-position gate of the Python form: a byte of 0 over an emitted record
        emit = np.ones(n, np.uint8)
        emit[idx[::2]] = 0
        assert variants.select(recs, None, emit).tolist() == idx[1::2].tolist()
        with pytest.raises(ValueError):
            variants.select(recs, {"reserved": 3})
        with pytest.raises(ValueError):
            variants.select(recs, {"min_qual": 3})


def test_transitions_and_transversions_by_hand():
    recs = np.zeros(9, VCF_REC)
    b = recs.view(np.uint8).reshape(-1, 128)
    b[:, 4] = 1
    #            ref_code alt0 alt1
    for k, (rc, a0, a1) in enumerate([(1, "G", 0), (3, "A", 0), (2, "T", 0), (4, "C", 0), (1, "C", 0), (2, "G", 0), (0, "A", 0), (1, "N", 0), (1, "G", "T")]):
        b[k, 6], b[k, 12], b[k, 13] = rc, ord(a0), ord(a1) if a1 else 0
    t = variants.totals(recs[variants.select(recs)])
    assert t[:3] == (9, 8, 1) and t[7:9] == (4, 2)
    rc, _, n_out, tot = host_select(recs, {})
    assert rc == 0 and tot == t


def _stream():
    """Three records, in both formats, written by hand from the formats' definitions: a hom-ref C at 100 (no ALT), a het C/T at 101 (QUAL 50,
    PASS) and a two-ALT record at 205 (REF A, ALT C,G, QUAL 20, FILTER fail)."""
    import struct

    def bcf(pos, ref, alts, qual, flt_id, gt):
        sh = b"\x07" + bytes([0x17]) + ref
        for a in alts:
            sh += bytes([0x17]) + a
        sh += bytes([0x11, flt_id])
        sh += bytes([0x11, 1, 0x57]) + b"CHHCG"  # INFO CX
        ind = bytes([0x11, 8, 0x21, (gt[0] + 1) << 1, (gt[1] + 1) << 1]) + bytes([0x11, 11, 0x11, qual])  # GT, GQ
        return struct.pack("<IIiiifII", 24 + len(sh), len(ind), 0, pos - 1, 1, float(qual), (1 + len(alts)) << 16 | 1, 2 << 24 | 1) + sh + ind

    def txt(pos, ref, alts, qual, flt, gt):
        return b"\t".join([b"chrQ", b"%d" % pos, b".", ref, b",".join(alts) or b".", b"%d" % qual, flt, b"CX=CHHCG", b"GT:GQ", b"%d/%d:%d" % (gt + (qual,))]) + b"\n"

    rows = [(100, b"C", [], 70, 0, (0, 0)), (101, b"C", [b"T"], 50, 0, (0, 1)), (205, b"A", [b"C", b"G"], 20, 2, (1, 2))]
    b = [bcf(*r) for r in rows]
    t = [txt(p, r, a, q, b"PASS" if f == 0 else b"fail", g) for p, r, a, q, f, g in rows]
    return b, t


def test_the_stream_checker_on_a_hand_made_stream():
    for text, parts in zip((False, True), _stream()):
        full = b"".join(parts)
        assert VR.select(full, text) == (parts[1] + parts[2], 2, (2, 1, 1, 2, 1, 0, 0, 1, 0, 70))
        assert VR.select(full, text, known={101, 100}) == (parts[1] + parts[2], 2, (2, 1, 1, 2, 1, 1, 1, 1, 0, 70))
        assert VR.select(full, text, {"min_phred": 21}) == (parts[1], 1, (1, 1, 0, 1, 1, 0, 0, 1, 0, 50))
        assert VR.select(full, text, {"pass_only": 1}, known={205}) == (parts[1], 1, (1, 1, 0, 1, 1, 0, 0, 1, 0, 50))
        assert VR.select(full, text, {"known_only": 1}, known={205}) == (parts[2], 1, (1, 0, 1, 1, 0, 1, 0, 0, 0, 20))
        assert VR.select(full, text, {"known_only": 1}) == (b"", 0, (0,) * 10)
        assert VR.select(b"", text) == (b"", 0, (0,) * 10)


def test_decoded_records_follow_the_same_rule():
    recs = [{"alt": [], "qual": 70, "filter": "PASS", "known": True, "ref": "C", "gt": (0, 0)},
            {"alt": ["T"], "qual": 50, "filter": "PASS", "known": False, "ref": "C", "gt": (0, 1)},
            {"alt": ["C", "G"], "qual": 20, "filter": "fail", "known": True, "ref": "A", "gt": (1, 2)}]
    assert variants.select_decoded(recs) == [1, 2] and variants.select_decoded(recs, {"known_only": 1}) == [2]
    assert variants.select_decoded(recs, {"pass_only": 1, "min_phred": 50}) == [1]
    assert variants.totals_decoded(recs[1:]) == (2, 1, 1, 2, 1, 1, 0, 1, 0, 70)


def test_host_form_under_sanitizers(tmp_path):
    """make variants-san: integration/variants_san.c + csrc/variants.c under ASan + UBSan, a program of its own."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "variants_san")
    subprocess.run([cc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "integration", "variants_san.c"),
                    os.path.join(ROOT, "bs_call_amd", "csrc", "variants.c"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
