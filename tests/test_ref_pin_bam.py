"""The record parser against the REFERENCE'S OWN BINARY: get_next_align_details of src/input_sam.c (with get_bam_misms,
get_seq_and_qual, get_bs_strand), compiled unchanged into oracle/_ref/libbscall_ref.so behind oracle/ref_driver.c
(refdrv_align_details: one call per BAM record), against its three forms here, field for field, on every record of
tests/bam_record_cases.py:
  bd_parse / bd_misms_of / bd_base_byte (csrc/bamdev_core.h: the statements the kernels of csrc/bamdev.hip run), compiled for the host
                          (tests/emul/bamdev_emul.cpp, bd_emul_record)
  csrc/bamio.c            through the host reader, on files where one used record is one template
  oracle/py_bam.py        its functions, called directly
Until now these three were only compared with each other, and all three are this project's readings of the same file.
CPU only (the kernels themselves: tests/test_gpu_ref_pin.py).  Where the binary is absent — or with BSC_REF_PIN_GOLDEN=1, which is
how the fallback is checked on a machine that has it — the reference's results come from tests/golden/ref_align_details.json / .bin,
recorded from the same binary by tools/make_ref_align_vectors.py over the reduced case set, and the output says so."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from bs_call_amd.bam import BamReader
from oracle import py_bam, ref_loader as R

import bam_record_cases as BC
import test_bamdev_emul as TE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_TREE = os.environ.get("REF", "/root/reference")
USE_GOLDEN = bool(os.environ.get("BSC_REF_PIN_GOLDEN"))
GROUPS = ["aux", "cigar", "seq", "mix", "fixed"]

BD_DESC = np.dtype([("off", "<u8"), ("hash", "<u8"), ("tid", "<i4"), ("fwd", "<u4"), ("rev", "<u4"), ("span", "<u4"), ("aln_len", "<u4"), ("l_seq", "<u4"),
                    ("del_len", "<u4"), ("bs", "<u4"), ("aflag", "<u2"), ("n_cigar", "<u2"), ("n_ms", "<u2"), ("status", "u1"), ("flt", "u1"), ("mapq", "u1"),
                    ("rev_ori", "u1"), ("bs_strand", "u1"), ("l_name", "u1"), ("q0", "u1"), ("q1", "u1"), ("pad_", "<u2")])
assert BD_DESC.itemsize == 64
ST_USE, ST_FILTERED, ST_MALFORMED_CIGAR = 0, 1, 3


@pytest.fixture(scope="module")
def sets():
    """group -> RefSet: the cases with the reference's results, from the binary or from the recorded fixture"""
    if not USE_GOLDEN and os.path.isdir(os.path.join(REF_TREE, "include")):
        assert R.build(REF_TREE), "`%s` did not produce oracle/_ref/libbscall_ref.so although %s/include exists" % (R.RECIPE, REF_TREE)
        assert R.has_align_details(), "the recipe's binary has no refdrv_align_details"
    if R.has_align_details() and not USE_GOLDEN:
        return BC.live_sets(lambda r, o, ku, idup: R.align_details(r, o, BC.MAPQ_THRESH, BC.MAX_TEMPLATE_LEN, ku, idup))
    print("\n[ref pin] the reference's binary is not used (absent, built before it had refdrv_align_details, or BSC_REF_PIN_GOLDEN; recipe: `%s`): the reduced case set and its results "
          "come from tests/golden/ref_align_details.json" % R.RECIPE)
    return BC.golden_sets()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emul_rec") / "libbamdev_emul.so")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", out, os.path.join(ROOT, "tests", "emul", "bamdev_emul.cpp")])
    return ctypes.CDLL(out)


def _report(what, n, diffs):
    print("\n[ref pin] %s: %d records compared, %d differ" % (what, n, len(diffs)))
    assert not diffs, "%s: %d of %d records differ from the reference, first:\n%s" % (what, len(diffs), n, "\n".join(diffs[:8]))


def _cmp(diffs, name, key, pairs):
    bad = ["%s reference %r, ours %r" % (f, a, b) for f, a, b in pairs if a != b]
    if bad:
        diffs.append("  %s [%s]: %s" % (name, key, "; ".join(bad)))


# ---- the device's statements -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_device_parser_statements_against_get_next_align_details(sets, emul, group):
    """bd_parse (with bd_bs_strand), bd_misms_of, bd_base_byte on every record, under every setting the group has results for.  A record
    whose CIGAR disagrees with l_seq is compared in its status alone: bd_parse drops it before it computes any other field."""
    rs = sets[group]
    diffs, n = [], 0
    for s in BC.SETTINGS:
        key = BC.setting_key(s)
        if key not in rs.res:
            continue
        a = rs.res[key][0]
        par = TE.Params(BC.MAPQ_THRESH, int(s[0]), int(s[1]), 0, BC.MAX_TEMPLATE_LEN, 0, 0, 0, len(BC.REFS), 0, None)
        for i, raw in enumerate(rs.raws):
            d = np.zeros(1, dtype=BD_DESC)
            n_cig, l_seq = int.from_bytes(raw[16:18], "little"), int.from_bytes(raw[20:24], "little")
            ms = np.zeros(max(1, n_cig), dtype=BC.MISMS_T)
            by = np.zeros(max(1, l_seq), dtype=np.uint8)
            buf = (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw)
            st = emul.bd_emul_record(buf, ctypes.c_uint64(len(raw)), ctypes.byref(par), d.ctypes.data_as(ctypes.c_void_p), ms.ctypes.data_as(ctypes.c_void_p),
                                     by.ctypes.data_as(ctypes.c_void_p))
            n += 1
            if rs.cpu_only[i]:
                _cmp(diffs, rs.names[i], key, [("status of a dropped record", ST_MALFORMED_CIGAR, st)])
                continue
            d, r = d[0], a[i]
            used = int(r["ret"]) == 0
            pairs = [("ret", int(r["ret"]), {ST_USE: 0, ST_FILTERED: 1}.get(st, "status %d" % st)), ("filtered", int(r["filtered"]), int(d["flt"])),
                     ("reverse", int(r["reverse"]), int(d["rev_ori"]) & 1), ("orientation", int(r["orientation"]), int(d["rev_ori"]) >> 1),
                     ("alignment_flag", int(r["alignment_flag"]), int(d["aflag"])), ("forward_position", int(r["forward_position"]), int(d["fwd"])),
                     ("reverse_position", int(r["reverse_position"]), int(d["rev"])), ("mapq", int(r["mapq"]), int(d["mapq"])),
                     ("align_length", int(r["align_length"]), int(d["aln_len"])), ("reference_span", int(r["reference_span"]), int(d["span"])),
                     ("bs_strand", int(r["bs_strand"]), int(d["bs_strand"]))]
            if used:
                pairs += [("n_misms", int(r["n_misms"]), int(d["n_ms"])), ("l_qseq", int(r["read_len"]), int(d["l_seq"])),
                          ("mismatches", rs.misms(key, i), [[int(m["type"]), int(m["position"]), int(m["size"])] for m in ms[: int(d["n_ms"])]]),
                          ("read", rs.read(key, i), by[:l_seq].tolist())]
            _cmp(diffs, rs.names[i], key, pairs)
    _report("bd_parse / bd_misms_of / bd_base_byte, group %s" % group, n, diffs)


# ---- the Python restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_py_bam_against_get_next_align_details(sets, group):
    """oracle/py_bam.get_next_align_details (with its get_bs_strand), every record and every field — the records whose CIGAR disagrees
    with l_seq too: py_bam walks them as the reference does."""
    rs = sets[group]
    diffs, n = [], 0
    for s in BC.SETTINGS:
        key = BC.setting_key(s)
        if key not in rs.res:
            continue
        a = rs.res[key][0]
        for i, raw in enumerate(rs.raws):
            ret, al, reverse, filtered, align_length, aflag = py_bam.get_next_align_details(BC.parse_record(raw), BC.MAPQ_THRESH, BC.MAX_TEMPLATE_LEN, s[0], s[1])
            r = a[i]
            ix = 1 if reverse else 0
            n += 1
            _cmp(diffs, rs.names[i], key,
                 [("ret", int(r["ret"]), ret), ("filtered", int(r["filtered"]), filtered), ("reverse", int(r["reverse"]), int(reverse)),
                  ("orientation", int(r["orientation"]), al["orientation"]), ("alignment_flag", int(r["alignment_flag"]), aflag),
                  ("forward_position", int(r["forward_position"]), al["pos"][0]), ("reverse_position", int(r["reverse_position"]), al["pos"][1]),
                  ("mapq", int(r["mapq"]), al["mapq"][ix]), ("align_length", int(r["align_length"]), align_length),
                  ("reference_span", int(r["reference_span"]), al["span"][ix]), ("bs_strand", int(r["bs_strand"]), al["bs_strand"]),
                  ("mismatches", rs.misms(key, i), al["misms"][ix]), ("read", rs.read(key, i), al["reads"][ix] or [])])
    _report("oracle/py_bam.py, group %s" % group, n, diffs)


# ---- the host reader ---------------------------------------------------------------------------------------------------------------------------
def host_blocks(path, **kw):
    """(templates of all blocks in file order as tests/test_bam.py's c_blocks shapes them, filter counts, filter bases, dropped records)"""
    import test_bam as TB

    blocks, cts, bases = TB.c_blocks(path, **kw)
    with BamReader(path, **kw) as r:
        for _ in r.blocks():
            pass
        dropped = r.malformed()
    return BC.flatten_blocks(blocks), cts, bases, dropped


def _same_templates(what, got, want_idx, rs, key):
    want = [BC.template_of(rs, key, i) for i in want_idx]
    assert len(got) == len(want), "%s: %d templates, the reference uses %d records" % (what, len(got), len(want))
    for t, w, i in zip(got, want, want_idx):
        assert t == w, "%s: %s: reference %s, ours %s" % (what, rs.names[i], w, t)


@pytest.mark.parametrize("group", BC.FILE_GROUPS)
def test_host_reader_against_get_next_align_details(sets, tmp_path, group):
    """csrc/bamio.c (next_record, store_read) on the group as a file: its templates are the reference's used records one for one, its
    fifteen filter counters and base sums the tally of the reference's `filtered` and l_qseq; the records whose CIGAR disagrees with
    l_seq are in the file and are counted as dropped."""
    rs = sets[group]
    key = BC.setting_key(BC.SETTINGS[0])
    a = rs.res[key][0]
    path = str(tmp_path / (group + ".bam"))
    BC.write_bam_raw(path, rs.raws)
    got, cts, bases, dropped = host_blocks(path)
    keep = BC.file_records(rs, key)
    _same_templates("csrc/bamio.c, group %s" % group, got, [i for i in keep if int(a["ret"][i]) == 0], rs, key)
    assert (cts, bases) == BC.tally(rs, key, keep)
    assert dropped == len(rs) - len(keep)
    print("\n[ref pin] csrc/bamio.c, group %s: %d records in the file, %d templates compared, %d dropped (CIGAR / l_seq)" % (group, len(rs), len(got), dropped))


@pytest.mark.parametrize("setting", BC.SETTINGS, ids=BC.setting_key)
def test_host_reader_flag_sweep_against_get_next_align_details(sets, tmp_path, setting):
    """The fixed-field group as a file: the records the reference filters and those it uses with PAIRED cleared (lone mates are what
    read_input asserts on, and are left out: at most 2 % of the records).  The host reader accepts the file; its counters and base sums
    equal the reference's tally, its templates the reference's used records."""
    rs = sets["fixed"]
    key = BC.setting_key(setting)
    a = rs.res[key][0]
    keep, out = BC.gpu_flag_file(rs, key)
    n_out, n_sweep = BC.sweep_share(rs, out)
    assert n_out <= 0.02 * n_sweep, "left out %d of the sweep's %d records" % (n_out, n_sweep)
    path = str(tmp_path / "flags.bam")
    BC.write_bam_raw(path, [rs.raws[i] for i in keep])
    got, cts, bases, dropped = host_blocks(path, keep_unmatched=setting[0], ignore_duplicates=setting[1])
    _same_templates("csrc/bamio.c, flag sweep %s" % key, got, [i for i in keep if int(a["ret"][i]) == 0], rs, key)
    assert (cts, bases) == BC.tally(rs, key, keep) and dropped == 0
    print("\n[ref pin] csrc/bamio.c, flag sweep %s: %d records in the file, %d templates, %d filtered; left out %d of the sweep's %d (%.2f %%), %d of all %d"
          % (key, len(keep), len(got), sum(cts), n_out, n_sweep, 100.0 * n_out / n_sweep, len(out), len(rs)))


# ---- the case set says what it claims --------------------------------------------------------------------------------------------------------
def test_the_case_set_reaches_the_branches_it_names(sets):
    """what the groups' names promise, read off the reference's own results: the walk reaches the strand tag behind every skipped tag,
    the 32-bit product wraps, every filter reason the parser can give occurs, every list type, the clamp and every nibble code"""
    key = BC.setting_key(BC.SETTINGS[0])
    rs = sets["aux"]
    a = rs.res[key][0]
    by_name = {n.split("/", 1)[1]: int(a["bs_strand"][i]) for i, n in enumerate(rs.names)}
    assert all(v == 1 for n, v in by_name.items() if n.startswith("skip ")) and sum(n.startswith("skip ") for n in by_name) == 12 + 27
    assert by_name["B product wraps to 0"] == 1 and by_name["B product wraps to 4"] == 1 and by_name["B product of s wraps to 0"] == 2
    assert by_name["B product just below the wrap"] == 2 and by_name["B count beyond the end"] == 2 and by_name["B array of 8 KB"] == 1
    assert by_name["two tags, the later decides"] == 2 and by_name["a later tag without a meaning"] == 2
    rs = sets["cigar"]
    a, ms, _ = rs.res[key]
    assert set(ms["type"].tolist()) == {1, 2, 3} and int(a["n_misms"].max()) >= 150 and sum(rs.cpu_only) == 4
    i = [n.split("/", 1)[1] for n in rs.names].index("5M2P5M")
    assert int(a["align_length"][i]) == 12 and int(a["reference_span"][i]) == 10 and rs.misms(key, i) == [[3, 5, 2]]
    rs = sets["seq"]
    a, _, seq = rs.res[key]
    assert set(BC.LENGTHS) <= set(a["read_len"].tolist()) and int(seq.max()) >> 2 == 43 and set((seq & 3).tolist()) == {0, 1, 2, 3}
    rs = sets["fixed"]
    reasons = set()
    for s in BC.SETTINGS:
        a = rs.res[BC.setting_key(s)][0]
        reasons |= set(a["filtered"].tolist())
        assert (a["ret"] == 0).any() and (a["ret"] == 1).any()
    assert reasons == {0, 1, 2, 3, 4, 5, 8, 9, 10, 12, 13}
    if not USE_GOLDEN and R.has_align_details():
        assert len(rs) >= 2 * 4096 and len(sets["mix"]) >= 2000


# ---- the recorded fixture ----------------------------------------------------------------------------------------------------------------------
def test_golden_align_vectors_regenerate_to_the_same_file(tmp_path):
    if not R.has_align_details():
        pytest.skip("no oracle/_ref/libbscall_ref.so with refdrv_align_details to regenerate the fixture with (recipe: `%s REF=<reference root>`)" % R.RECIPE)
    spec = importlib.util.spec_from_file_location("make_ref_align_vectors", os.path.join(ROOT, "tools", "make_ref_align_vectors.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    out = tmp_path / "ref_align_details.json"
    M.write(str(out))
    for new, old in ((out, BC.GOLDEN), (tmp_path / "ref_align_details.bin", os.path.splitext(BC.GOLDEN)[0] + ".bin")):
        with open(old, "rb") as f:
            assert new.read_bytes() == f.read(), "tools/make_ref_align_vectors.py no longer reproduces %s" % os.path.relpath(old, ROOT)
        assert os.path.getsize(old) < 300 * 1024
