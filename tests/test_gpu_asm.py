"""The allele-specific methylation table on the device (csrc/asmdev.hip) — the rule of include/bscall_amd.h (SNP, ALLELE, WINDOW, RECORD, AQ,
TOTALS, LINE):

  1. bsc_asm_device against the host form (csrc/asm.c) and the Python rule (bs_call_amd/asm.py), byte for byte and total for total, on the
     blocks of tests/asm_cases.py: the hand-worked block, the 48 entries of ALLELE, the targeted and the tile-position blocks, block lengths
     around a tile, a long read, contention, 46 341 templates on one pair (DEEP), 20 003 positions on the default and on a one-CU grid and
     twice, the rooms with their guard bytes, the refusals
  2. bsc_asm_text_device against the host formatter
  3. bsc_block_asm_kept behind both _keep calls on a device reader's blocks, against the Python rule over the host pre-processing of the same
     raw block and the decoded kept stream's records; what the context keeps beside it is untouched
  4. bam2bcf --meth-asm and pipeline.run(asm_path=) file to file"""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import asm_cases as A
import bs_call_amd as B
import csi_ref
import variants_ref
from bs_call_amd import _lib, asm, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import asm_format_host, asm_pairs_host, prepare_templates
from oracle import py_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
PAD = 0xEE
GUARD = 3  # records of guard bytes behind the room
MARK = 0x7777777777777777
LFACT = asm.lfact_table()


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        assert c.tables()[1].tobytes() == LFACT.tobytes()  # the context's ln k! is the table the host form and the Python rule are given
        yield c


@pytest.fixture(scope="module")
def one_cu():
    old = os.environ.get("BSC_NUM_CUS")
    os.environ["BSC_NUM_CUS"] = "1"
    try:
        c = B.SiteCaller()
    finally:
        if old is None:
            os.environ.pop("BSC_NUM_CUS", None)
        else:
            os.environ["BSC_NUM_CUS"] = old
    yield c
    c.close()


def dev(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(a.copy() if a.size else np.zeros(8, np.uint8)).to("cuda")
    torch.cuda.synchronize()
    return t


def host(b, cap=None):
    return asm_pairs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["core"], b["emit"], LFACT, b["min_qual"], b["params"], cap=cap)


def run_device(caller, b, cap=None, params=None, expect_refusal=False, keep=False, need=None):
    """bsc_asm_device over a block of tests/asm_cases.py.  Returns (records[min(count, room)], count, totals) after checking the guard bytes
    behind the count and behind the room.  cap None: the room is the count the host form gives (need, where the caller has it)."""
    assert caller.params["min_qual"] == b["min_qual"]
    d_tpl, d_seq, d_ref, d_core = dev(b["tpl"]), dev(b["seq"]), dev(b["ref"]), dev(b["core"])
    d_emit = None if b["emit"] is None else dev(b["emit"])
    room = (host(b, cap=0)[1] if need is None else need) if cap is None else cap
    d_pairs = torch.full(((room + GUARD) * 32,), PAD, dtype=torch.uint8, device="cuda")
    d_n = torch.full((1,), MARK, dtype=torch.int64, device="cuda")
    d_tot = torch.full((8,), MARK, dtype=torch.int64, device="cuda")
    par = b["params"] if params is None else params
    args = (d_tpl.data_ptr(), len(b["tpl"]), d_seq.data_ptr(), len(b["seq"]), b["x"], b["y"], d_ref.data_ptr(), d_core.data_ptr(),
            None if d_emit is None else d_emit.data_ptr(), d_pairs.data_ptr(), room, d_n.data_ptr(), d_tot.data_ptr())
    if expect_refusal:
        with pytest.raises(B.BscError):
            caller.asm_device(*args, params=_lib.AsmParams(**par))
        torch.cuda.synchronize()
        assert (d_pairs.cpu().numpy() == PAD).all() and int(d_n.cpu()[0]) == MARK and (d_tot.cpu().numpy() == MARK).all()
        return None
    caller.asm_device(*args, params=par)
    torch.cuda.synchronize()
    count = int(d_n.cpu().numpy().view(np.uint64)[0])
    tot = tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64))
    out = d_pairs.cpu().numpy()
    stored = min(count, room)
    assert (out[stored * 32 :] == PAD).all(), "bytes behind the count or behind the room were written"
    recs = out[: stored * 32].view(asm.PAIR)
    if keep:
        return d_pairs, d_n, recs, count, tot
    return recs, count, tot


def check_block(caller, b, python_too=True):
    want, n, wtot = host(b)
    got, count, tot = run_device(caller, b, need=n)
    assert count == n == len(want), (b["name"], count, n)
    assert tot == wtot, (b["name"], tot, wtot)
    bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(axis=1))
    assert got.tobytes() == want.tobytes(), (b["name"], got[bad[:2]], want[bad[:2]])
    if python_too:
        p_recs, p_tot = asm.pairs(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["core"], b["emit"], b["min_qual"], py_model.fisher, LFACT, b["params"])
        assert p_recs.tobytes() == got.tobytes() and p_tot == tot, b["name"]
    return got, tot


# ---- 1. the records -------------------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_block(caller):
    got, tot = check_block(caller, A.hand_block())
    assert [tuple(int(v) for v in r) for r in got] == A.HAND_RECORDS and tot == A.HAND_TOTALS


def test_the_48_entries_of_allele(caller):
    for b, al in A.allele_blocks():
        got, tot = check_block(caller, b)
        assert tuple(int(got[0][f]) for f in ("m1", "u1", "m2", "u2")) == {0: (0, 0, 0, 0), 1: (1, 0, 0, 0), 2: (0, 0, 1, 0)}[al], b["name"]


@pytest.mark.parametrize("b", A.targeted_blocks() + A.tile_blocks(), ids=lambda b: b["name"])
def test_targeted_blocks(caller, b):
    check_block(caller, b)


@pytest.mark.parametrize("n_pos", [63, 64, 65, 127, 128, 129])
def test_block_lengths_around_a_tile(caller, n_pos):
    for seed in (0, 1):
        b = A.random_block(100 * n_pos + seed, n_pos, 60, 6, params={"max_dist": 40 + 60 * seed, "min_cov": 1})
        got, tot = check_block(caller, b)
        assert tot[4] > 0 and len(got) > 3
        check_block(caller, dict(b, emit=None))


def test_a_long_read(caller):
    got, tot = check_block(caller, A.long_read_block())
    assert tot[0] == 2 and tot[2] == 4 and tot[4] > 20


def test_contention(caller):
    b = A.contention_block(5000)
    got, tot = check_block(caller, b, python_too=False)
    x = b["x"]
    assert [tuple(int(v) for v in r)[:6] for r in got] == [(x + 10, x + 3, 2500, 0, 0, 2500), (x + 10, x + 15, 0, 2500, 2500, 0)]
    assert tot == (1, 2, 5000, 2500, 10000, 0, 0, 0) and [int(v) for v in got["aq"]] == [1000, 1000]


def test_deep_on_the_device(caller):
    got, tot = check_block(caller, A.repeated_block(46_341), python_too=False)
    assert [tuple(int(v) for v in r) for r in got] == [(60, 61, 46_341, 0, 0, 0, 0, 3 | 2 << 8)] and tot == (1, 1, 46_341, 46_341, 46_341, 1, 0, 0)
    got, tot = check_block(caller, A.repeated_block(46_340), python_too=False)
    assert [tuple(int(v) for v in r) for r in got] == [(60, 61, 46_340, 0, 0, 0, 0, 3)] and tot[5] == 0


@pytest.fixture(scope="module")
def big():
    """20 003 positions, 3 000 templates, about 40 SNPs.  The seed was chosen on the CPU so that the block shows a record with aq == 0, one with
    0 < aq < 1000 and an OVERLAPPED one."""
    b = A.random_block(20003, 20_003, 3_000, 40, params={"max_dist": 500, "min_cov": 1})
    want, n, tot = host(b)
    free = (want["info"] >> 8) == 0
    assert 35 <= tot[0] <= 50 and n == len(want) > 2000 and tot[4] > 1000
    assert (free & (want["aq"] == 0)).any() and (free & (want["aq"] > 0) & (want["aq"] < 1000)).any() and ((want["info"] >> 8) == 1).any()
    return b, want, tot


def test_20003_positions(caller, big):
    b, want, wtot = big
    got, count, tot = run_device(caller, b, need=len(want))
    assert count == len(want) and tot == wtot and got.tobytes() == want.tobytes()
    # the same input twice gives the same bytes
    again, _, tot2 = run_device(caller, b, need=len(want))
    assert again.tobytes() == got.tobytes() and tot2 == tot
    # a room one short, then exact: counted, not stored, nothing behind the room
    part, count, tot3 = run_device(caller, b, cap=len(want) - 1)
    assert count == len(want) and tot3 == wtot and part.tobytes() == want[:-1].tobytes()
    half, count, tot3 = run_device(caller, b, cap=len(want) // 2)
    assert count == len(want) and tot3[:5] == wtot[:5] and half.tobytes() == want[: len(want) // 2].tobytes()
    none, count, tot4 = run_device(caller, b, cap=0)
    assert count == len(want) and len(none) == 0 and tot4[:5] == wtot[:5]
    p_recs, p_tot = asm.pairs(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["core"], b["emit"], 20, py_model.fisher, LFACT, b["params"])
    assert p_recs.tobytes() == got.tobytes() and p_tot == tot


def test_20003_positions_on_a_one_cu_grid(one_cu, big):
    b, want, wtot = big
    got, count, tot = run_device(one_cu, b, need=len(want))
    assert count == len(want) and tot == wtot and got.tobytes() == want.tobytes()
    d_pairs, d_n, _, _, _ = run_device(one_cu, b, need=len(want), keep=True)
    table, lines = asm_format_host("chr20", want, b["params"])
    out, t2 = text_device(one_cu, d_pairs, d_n, len(want), "chr20", b["params"], len(table))
    assert t2 == (len(table), lines) and out.tobytes() == table


def test_refusals_leave_the_guard_bytes(caller):
    b = A.random_block(5, 300, 30, 5)
    for bad in ({"max_dist": 0}, {"max_dist": 65536}):
        run_device(caller, b, cap=4, params=dict(b["params"], **bad), expect_refusal=True)
    run_device(caller, dict(b, y=b["x"] - 1), cap=4, expect_refusal=True)
    # unaligned dense records
    d_core = dev(np.concatenate([np.zeros(8, np.uint8), b["core"].view(np.uint8)]))
    d_n = torch.full((1,), MARK, dtype=torch.int64, device="cuda")
    d_tot = torch.full((8,), MARK, dtype=torch.int64, device="cuda")
    d_tpl, d_seq, d_ref = dev(b["tpl"]), dev(b["seq"]), dev(b["ref"])
    with pytest.raises(B.BscError):
        caller.asm_device(d_tpl.data_ptr(), len(b["tpl"]), d_seq.data_ptr(), len(b["seq"]), b["x"], b["y"], d_ref.data_ptr(), d_core.data_ptr() + 8, None, None, 0,
                          d_n.data_ptr(), d_tot.data_ptr(), params=b["params"])
    torch.cuda.synchronize()
    assert int(d_n.cpu()[0]) == MARK and (d_tot.cpu().numpy() == MARK).all()
    check_block(caller, b)  # the context is usable behind the refusals


# ---- 2. the lines ---------------------------------------------------------------------------------------------------------------------------
def text_device(caller, d_pairs, d_n, max_pairs, contig, par, cap):
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_t2 = torch.full((2,), MARK, dtype=torch.int64, device="cuda")
    caller.asm_text_device(d_pairs.data_ptr(), d_n.data_ptr(), max_pairs, contig, d_out.data_ptr(), cap, d_t2.data_ptr(), params=par)
    torch.cuda.synchronize()
    t2 = tuple(int(v) for v in d_t2.cpu().numpy().view(np.uint64))
    out = d_out.cpu().numpy()
    assert (out[cap:] == PAD).all(), "bytes behind the room were written"
    return out[:cap], t2


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4113])
def test_text_device_equals_the_host_formatter(caller, n):
    rng = np.random.default_rng(900 + n)
    recs = np.zeros(n, asm.PAIR)
    for f in asm.PAIR.names:  # numbers of 1 .. 10 digits
        recs[f] = (10 ** rng.integers(0, 10, n) * rng.integers(1, 10, n)).clip(1, 0xFFFFFFFF)
    recs["info"] = rng.choice([1, 2, 3, 5, 6, 8, 0, 9, 200, 3 | 1 << 8, 5 | 2 << 8], n)
    recs["m1"][::5] = 0
    recs["u1"][::5] = 0
    recs["m2"][2::5] = 1
    recs["u2"][2::5] = 0
    if n > 6:
        recs[5] = (0xFFFFFFFF, 1_000_000_001, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 3)  # the longest line
        recs[6] = (1, 0xFFFFFFFF, 1, 0, 0, 1, 0, 8)
    d_pairs = dev(recs) if n else torch.zeros(32, dtype=torch.uint8, device="cuda")
    for name, mc, count in (("chr1", 1, n), ("c", 2, n), ("x" * 255, 0, n), ("chr1", 1, n // 2), ("chr1", 1, n + 7)):
        par = {"min_cov": mc}
        d_n = torch.tensor([count], dtype=torch.int64, device="cuda")  # the device count decides, never beyond max_pairs
        used = recs[: min(count, n)]
        want, lines = asm_format_host(name, used, par)
        assert (want, lines) == asm.format_pairs(name, used, par)
        out, t2 = text_device(caller, d_pairs, d_n, n, name, par, len(want))
        assert t2 == (len(want), lines) and out.tobytes() == want, (n, name, mc, count)
        if want:  # one short: the full length is reported, the stream is cut at a 64-record boundary
            out, t2 = text_device(caller, d_pairs, d_n, n, name, par, len(want) - 1)
            assert t2 == (len(want), lines)
            whole = asm_format_host(name, used[: (len(used) - 1) // 64 * 64], par)[0]
            assert out[: len(whole)].tobytes() == whole and (out[len(whole) :] == PAD).all()
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(B.BscError):
            text_device(caller, d_pairs, torch.tensor([n], dtype=torch.int64, device="cuda"), n, bad, {}, 64)


def test_text_device_takes_the_walk_s_records_and_count(caller, big):
    b, want, _ = big
    d_pairs, d_n, recs, count, _ = run_device(caller, b, keep=True, need=len(want))
    for par in (b["params"], dict(b["params"], min_cov=2)):
        table, lines = asm_format_host("chr20", want, par)
        out, t2 = text_device(caller, d_pairs, d_n, len(want) + GUARD, "chr20", par, len(table))  # the guard records are not lines
        assert t2 == (len(table), lines) and out.tobytes() == table
    assert lines > 20


# ---- 3. the block entry ---------------------------------------------------------------------------------------------------------------------
def _fixture_files(d, reference, recs, name):
    refs = [(k, len(v)) for k, v in reference.items()]
    bam, fa = str(d / (name + ".bam")), str(d / (name + ".fa"))
    W.write_bam(bam, refs, recs)
    with open(fa, "w") as f:
        for nm, codes in reference.items():
            f.write(">%s\n" % nm)
            s = "".join("NACGT"[c] for c in codes)
            for o in range(0, len(s), 60):
                f.write(s[o : o + 60] + "\n")
    return bam, fa, refs


HET_EVERY = 300
PLANTED = {1: "AC", 5: "CG", 8: "GT", 3: "AT"}  # what tools/make_bam.py plants over a reference A, C, G, T: the next letter, on every other template


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """A BAM of three contigs: chrA, 6 000 positions at ~40x whose every 300th position is a planted heterozygous site — reference A, C, G, T in
    turn, so AC, CG, GT and AT — with a CpG planted 7 bases in front and 12 behind each; chrT, 60 positions (a block shorter than a tile);
    chrG, 30 000 positions in several blocks with gaps between the reads."""
    d = tmp_path_factory.mktemp("asm_files")
    rng = np.random.default_rng(4714)
    a = rng.integers(1, 5, 6_000).astype(np.uint8)
    for k, g in enumerate(range(HET_EVERY - 1, 6_000 - 20, HET_EVERY)):  # g: 0-based
        a[g - 1], a[g], a[g + 1] = 1, 1 + k % 4, 1  # A x A: the site is no part of a CpG
        a[g - 7 : g - 5] = (2, 3)
        a[g + 12 : g + 14] = (2, 3)
    reference = {"chrA": a, "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8), "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=HET_EVERY) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50, err=0.0)
            + W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


PAR = {"min_phred": 20, "pass_only": 0, "max_dist": 200, "min_cov": 2}


def cores_of_stream(stream, text, x, y):
    """The dense records the rule needs, from the DECODED kept stream: a record per written position with emit = 1, the genotype from the
    alleles and FORMAT GT, phred = QUAL, flt = 0 / 1 from FILTER."""
    from bs_call_amd.abi import VCF_CORE

    core = np.zeros(y - x + 1, VCF_CORE)
    for _, _, r in (variants_ref.text_records if text else variants_ref.bcf_records)(stream):
        alleles = [r["ref"]] + list(r["alt"])
        letters = sorted(alleles[g].decode() for g in r["gt"])
        c = core[r["pos"] - x]
        c["pos"], c["emit"], c["phred"], c["flt"] = r["pos"], 1, r["qual"], 0 if r["passed"] else 1
        c["gt"] = asm.GENOTYPES.index("".join(letters)) if all(l in "ACGT" for l in letters) else 255
    return core


def python_table(name, raw, seq, ms, x, y, ref, core, par=PAR):
    """The Python rule over the HOST pre-processing of a raw block and the decoded stream's records: (table, lines, totals, records)."""
    tpl, pseq, _ = prepare_templates(raw, seq, ms)
    recs, tot = asm.pairs(tpl, pseq, x, y, ref, core, None, 20, py_model.fisher, LFACT, par)
    table, lines = asm.format_pairs(name, recs, par)
    return table, lines, tot, recs


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    n_blocks = n_lines = n_aq = 0
    seen_gt = set()
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            raw, seq, ms = rd.fetch(blk)
            kw = dict(reg_stop=len(codes))
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, keep=True, **kw)
            core = cores_of_stream(bcf0, False, x, y)
            want, w_lines, w_tot, w_recs = python_table(name, raw, seq, ms, x, y, ref, core)
            ent0, r0 = caller.block_csi_kept(14)
            merge0 = caller.block_meth_kept(name, merge=True)
            var0 = caller.block_variants_kept()
            reads0 = caller.block_cpg_reads_kept(name)
            got, lines, tot = caller.block_asm_kept(name, PAR)
            assert got == want and lines == w_lines and tot == w_tot, (name, x, tot, w_tot)
            assert caller.block_asm_kept(name, PAR) == (got, lines, tot)  # twice: the same bytes
            n_lines += lines
            _, back = asm.read_table(got)
            n_aq += int((back["aq"] > 0).sum())
            seen_gt |= set(int(v) for v in back["info"])
            # other parameters
            for par in ({"min_phred": 0, "pass_only": 1, "max_dist": 1, "min_cov": 0}, {"min_phred": 30, "pass_only": 0, "max_dist": 65535, "min_cov": 5}):
                assert caller.block_asm_kept(name, par) == python_table(name, raw, seq, ms, x, y, ref, core, par)[:3], (name, x, par)
            # a room one short, then the exact room; a read past the end
            nb, nl, t8 = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
            cp = _lib.AsmParams(**PAR)
            if got:
                assert L.bsc_block_asm_kept(h, name.encode(), C.byref(cp), len(got) - 1, C.byref(nb), C.byref(nl), t8) == -1
                assert nb.value == len(got) and b"dev_cap" in L.bsc_last_error() and tuple(int(v) for v in t8) == tot
                out = np.zeros(8, np.uint8)
                assert L.bsc_asm_stream_read(h, 0, 1, out.ctypes.data) == -1  # a refused call left no table
            assert L.bsc_block_asm_kept(h, name.encode(), C.byref(cp), max(len(got), 1), C.byref(nb), C.byref(nl), None) == 0
            assert (nb.value, nl.value) == (len(got), lines)
            assert caller.asm_stream_read(0, len(got)) == got
            out = np.zeros(len(got) + 8, np.uint8)
            assert L.bsc_asm_stream_read(h, 1, len(got), out.ctypes.data) == -1 and b"beyond" in L.bsc_last_error()
            # what the context keeps beside it is untouched
            assert kept_stream(caller, len(bcf0)) == bcf0
            ent1, r1 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() and r0 == r1 == n_rec
            assert caller.block_meth_kept(name, merge=True) == merge0
            assert caller.block_variants_kept() == var0
            assert caller.cpg_reads_stream_read(0, len(reads0[0])) == reads0[0]  # the read-level table where it was left ...
            assert caller.block_cpg_reads_kept(name) == reads0
            assert caller.asm_stream_read(0, len(got)) == got  # ... and this one behind the other follow-ups
            assert caller.block_asm_kept(name, PAR)[0] == got
            # the refusals of the arguments leave the block where it is
            for bad_name, bad_par in ((b"a\tb", cp), (name.encode(), _lib.AsmParams(20, 0, 0, 2)), (name.encode(), _lib.AsmParams(20, 0, 65536, 2))):
                assert L.bsc_block_asm_kept(h, bad_name, C.byref(bad_par), 1 << 20, C.byref(nb), C.byref(nl), None) == -1 and nb.value == 0
            # behind the text encoder's keep call: the same table
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, **kw)
            assert n_txt == n_rec and cores_of_stream(text, True, x, y).tobytes() == core.tobytes()
            assert caller.block_asm_kept(name, PAR) == (got, lines, tot)
            assert kept_stream(caller, len(text)) == text
            # refused behind a call that kept nothing: the reads are gone
            caller.block_bcf_rawdev(blk, ref, tid, **kw)
            assert L.bsc_block_asm_kept(h, name.encode(), C.byref(cp), 1 << 20, C.byref(nb), C.byref(nl), None) == -1
            assert b"no single block" in L.bsc_last_error() and nb.value == 0
            n_blocks += 1
    assert n_blocks > 4 and n_lines > 40 and n_aq >= 1, (n_blocks, n_lines, n_aq)
    assert set(PLANTED) <= seen_gt, seen_gt  # a SNP of every het genotype the fixture plants, called by the caller itself


def test_a_detached_table_goes_through_the_device_writer(caller, small):
    import gzip

    from bs_call_amd import vcf

    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    with DeviceBamReader(caller, bam, threads=2) as rd:
        blk = next(iter(rd.device_blocks()))
        name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
        ref = block_reference(codes, int(blk.x), int(blk.y))
        caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
        full, lines, _ = caller.block_asm_kept(name, PAR)
        assert lines > 0
        p, nb = C.c_void_p(), C.c_uint64()
        assert L.bsc_asm_stream_detach(h, C.byref(p), C.byref(nb)) == 0 and nb.value == len(full) and p.value
        p2, nb2 = C.c_void_p(), C.c_uint64(9)
        assert L.bsc_asm_stream_detach(h, C.byref(p2), C.byref(nb2)) == -1 and not p2.value and nb2.value == 0  # once
        z = caller.bgzf()
        z.write_device(p.value, len(full))
        comp = z.take() + z.close()
        assert gzip.decompress(comp) == full and comp.endswith(vcf.BGZF_EOF)
        assert L.bsc_detached_free(h, p) == 0
        assert caller.block_asm_kept(name, PAR)[0] == full  # the next call takes a buffer again


def test_refused_before_any_block(small):
    with B.SiteCaller() as c:
        nb, nl = C.c_uint64(5), C.c_uint64(5)
        cp = _lib.AsmParams()
        assert c._L.bsc_block_asm_kept(c._h, b"chr1", C.byref(cp), 1 << 16, C.byref(nb), C.byref(nl), None) == -1
        assert b"no single block" in c._L.bsc_last_error() and (nb.value, nl.value) == (0, 0)


# ---- 4. file to file ------------------------------------------------------------------------------------------------------------------------
def run_exe(*args, env=None, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout
    return r


def file_table(caller, bam, refs, reference, par):
    """The concatenated per-block Python tables of a file and the sums of their totals."""
    out, tot = [], np.zeros(8, np.int64)
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            raw, seq, ms = rd.fetch(blk)
            bcf, _, _ = caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes))
            table, _, t, _ = python_table(name, raw, seq, ms, x, y, ref, cores_of_stream(bcf, False, x, y), par)
            out.append(table)
            tot += np.array(t)
    return b"".join(out), tuple(int(v) for v in tot)


def stdout_line(table, tot):
    return ("%d heterozygous SNPs in the allele-specific methylation table, %d SNP-CpG pairs, %d lines written (allele observations %d)\n"
            % (tot[0], tot[1], table.count(b"\n"), tot[2]))


def test_bam2bcf_meth_asm_and_pipeline(caller, small):
    from bs_call_amd import vcf

    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("f" + s))
    rd = lambda path: open(path, "rb").read()
    default = dict(A.DEFAULT)
    want, tot = file_table(caller, bam, refs, reference, default)
    assert want.count(b"\n") > 100 and tot[0] >= 15
    # plain: the table is the concatenated per-block tables; the main file, the report and the --meth-reads table as without the switch
    base = run_exe("--meth-reads", p(".u.reads"), bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    out = run_exe("--meth-asm", p(".ua.tsv"), "--meth-reads", p(".ua.reads"), bam, fa, p(".ua.bcf"), p(".ua.json"), "S9")
    assert rd(p(".ua.tsv")) == want
    for a, b in ((".ua.bcf", ".u.bcf"), (".ua.json", ".u.json"), (".ua.reads", ".u.reads")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    assert out == base + stdout_line(want, tot)
    # every line joins the --meth-reads table on (chrom, start, end), and the four counts are at most that line's m and u
    reads = {tuple(l.split(b"\t")[:3]): l.split(b"\t") for l in rd(p(".u.reads")).splitlines()}
    for line in want.splitlines():
        f = line.split(b"\t")
        r = reads[tuple(f[:3])]
        assert int(f[5]) + int(f[7]) <= int(r[3]) and int(f[6]) + int(f[8]) <= int(r[4]), line
    # a name that ends in .gz: BGZF, the same table; so under -O b, beside the compressed main file and its index
    out = run_exe("--meth-asm", p(".z.tsv.gz"), "--meth-reads", p(".z.reads"), bam, fa, p(".z.bcf"), p(".z.json"), "S9")
    blob = rd(p(".z.tsv.gz"))
    assert blob.endswith(vcf.BGZF_EOF) and csi_ref.inflate(blob) == want and out == base + stdout_line(want, tot)
    assert rd(p(".z.bcf")) == rd(p(".u.bcf")) and rd(p(".z.reads")) == rd(p(".u.reads"))
    base_b = run_exe("-O", "b", "--index", bam, fa, p(".b.bcf"), p(".b.json"), "S9")
    out = run_exe("-O", "b", "--index", "--meth-asm", p(".ba.tsv"), bam, fa, p(".ba.bcf"), p(".ba.json"), "S9")
    assert csi_ref.inflate(rd(p(".ba.tsv"))) == want and out == base_b + stdout_line(want, tot)
    for a, b in ((".ba.bcf", ".b.bcf"), (".ba.bcf.csi", ".b.bcf.csi"), (".ba.json", ".b.json")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    # the thresholds
    par = {"min_phred": 30, "pass_only": 1, "max_dist": 50, "min_cov": 5}
    want_t, tot_t = file_table(caller, bam, refs, reference, par)
    out = run_exe("--meth-asm", p(".t.tsv"), "--meth-asm-window", "50", "--meth-asm-min-qual", "30", "--meth-asm-min-cov", "5", "--meth-asm-pass", bam, fa,
                  p(".t.bcf"), p(".t.json"), "S9")
    assert rd(p(".t.tsv")) == want_t and 0 < want_t.count(b"\n") < want.count(b"\n") and out.endswith(stdout_line(want_t, tot_t))
    # pipeline.run(asm_path=...) writes the same file, compressed or not
    for compressed in (False, True):
        out = p(".pipe%d" % compressed)
        s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, compressed=compressed, asm_path=out + ".tsv", asm_params=par)
        got = rd(out + ".tsv")
        got = csi_ref.inflate(got) if compressed else got
        assert got == want_t and s["asm_lines"] == want_t.count(b"\n") and s["asm_totals"] == tot_t
    # refused where --meth-reads is: sharded runs, the host paths; no file is left behind
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), asm_path=p(".no.tsv"))
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, asm_path=p(".no.tsv"), shard_rank=0, shard_world=2)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, asm_params={"max_dist": 9})
    for args, env in ((["--rank", "0", "--world", "2"], None), ([], {"BAM2BCF_HOST_READER": "1"}), ([], {"BAM2BCF_HOST_BCF": "1"})):
        r = run_exe(*args, "--meth-asm", p(".no.tsv"), bam, fa, p(".no"), p(".no.json"), env=env, ok=False)
        assert r.returncode == 2 and "--meth-asm" in r.stderr
    for args in (["--meth-asm-window", "3"], ["--meth-asm-pass"], ["--meth-asm", p(".no.tsv"), "--meth-asm-window", "0"],
                 ["--meth-asm", p(".no.tsv"), "--meth-asm-window", "65536"], ["--meth-asm", p(".no.tsv"), "--meth-asm-min-cov", "x"]):
        r = run_exe(*args, bam, fa, p(".no"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--meth-asm" in r.stderr
    assert not os.path.exists(p(".no.tsv"))
