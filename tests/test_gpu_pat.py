"""The per-read CpG pattern table (PAT) on the device (csrc/patdev.hip, the radix sort of csrc/sort.hip) — the rule of include/bscall_amd.h
(ORDINAL, PATTERN, PIECES, RECORD, TOTALS, LINE over the COUNTS, SITE, BYTE, STATE of the read-level CpG table):

  1. bsc_pat_device against the host form (csrc/pat.c), record for record, total for total and — through bsc_pat_text_device — byte for byte,
     on the blocks of tests/pat_cases.py: the hand-worked block, the cuts at 64 sites, the placement blocks, block lengths around a tile, the
     long reads, 5 000 templates identical / in 16 patterns / all distinct, piece counts around a wave and a workgroup, 20 003 positions on the
     default and on a one-CU grid, a room one short, the refusals
  2. bsc_pat_text_device against the host formatter over records made by hand and over the walk's own
  3. bsc_block_pat_kept behind both _keep calls on a device reader's blocks, against the Python rule over the host pre-processing of the same
     raw block; what the context keeps beside it is untouched
  4. bam2bcf --meth-pat and pipeline.run(pat_path=) file to file"""
import ctypes as C
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import csi_ref
import pat_cases as P
from bs_call_amd import _lib, pat, pipeline, vcf
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import pat_count_sites, pat_format_host, pat_recs_host, prepare_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
PAD = 0xEE
GUARD = 3  # records of guard bytes behind the room
REC = 24
FILL = 0x7777777777777777


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
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


def run_device(caller, b, room, params=None, expect_refusal=False, keep=False):
    """bsc_pat_device over a block of tests/pat_cases.py.  Returns (records[min(count, room)], count, totals) after checking the guard bytes
    behind the count and behind the room."""
    assert caller.params["min_qual"] == b["min_qual"]
    d_tpl, d_seq, d_ref = dev(b["tpl"]), dev(b["seq"]), dev(b["ref"])
    d_rec = torch.full(((room + GUARD) * REC,), PAD, dtype=torch.uint8, device="cuda")
    d_n = torch.full((2,), FILL, dtype=torch.int64, device="cuda")  # [1]: the guard behind the count
    d_tot = torch.full((9,), FILL, dtype=torch.int64, device="cuda")  # [8]: the guard behind the totals
    par = b["params"] if params is None else params
    args = (d_tpl.data_ptr(), len(b["tpl"]), d_seq.data_ptr(), len(b["seq"]), b["x"], b["y"], d_ref.data_ptr(), d_rec.data_ptr(), room, d_n.data_ptr(),
            d_tot.data_ptr())
    if expect_refusal:
        with pytest.raises(B.BscError):
            caller.pat_device(*args, params=_lib.PatParams(**par))
        torch.cuda.synchronize()
        assert (d_rec.cpu().numpy() == PAD).all() and (d_n.cpu().numpy() == FILL).all() and (d_tot.cpu().numpy() == FILL).all()
        return None
    caller.pat_device(*args, params=par)
    torch.cuda.synchronize()
    assert int(d_n.cpu()[1]) == FILL and int(d_tot.cpu()[8]) == FILL, "words behind the count or the totals were written"
    count = int(d_n.cpu().numpy().view(np.uint64)[0])
    tot = tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64)[:8])
    out = d_rec.cpu().numpy()
    stored = min(count, room)
    assert (out[stored * REC :] == PAD).all(), "bytes behind the count or behind the room were written"
    recs = out[: stored * REC].view(pat.REC)
    if keep:
        return d_rec, d_n, recs, count, tot
    return recs, count, tot


def text_device(caller, d_rec, d_n, max_rec, contig, base, cap, par=None):
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_t2 = torch.full((3,), FILL, dtype=torch.int64, device="cuda")
    try:
        caller.pat_text_device(d_rec.data_ptr(), d_n.data_ptr(), max_rec, contig, base, d_out.data_ptr(), cap, d_t2.data_ptr(), params=par)
    except B.BscError:
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == PAD).all() and (d_t2.cpu().numpy() == FILL).all(), "a refusal wrote something"
        raise
    torch.cuda.synchronize()
    assert int(d_t2.cpu()[2]) == FILL
    t2 = tuple(int(v) for v in d_t2.cpu().numpy().view(np.uint64)[:2])
    out = d_out.cpu().numpy()
    assert (out[cap:] == PAD).all(), "bytes behind the room were written"
    return out[:cap], t2


def check_block(caller, b, want=None, base=77):
    """Device == host form: the records, the count, the totals, and the table's bytes through the device encoder."""
    if want is None:
        want = pat_recs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    w_recs, n, wtot = want
    d_rec, d_n, got, count, tot = run_device(caller, b, n + 2, keep=True)
    assert count == n == len(w_recs), (b["name"], count, n)
    assert tot == wtot, (b["name"], tot, wtot)
    bad = np.flatnonzero((got.view(np.uint64).reshape(-1, 3) != w_recs.view(np.uint64).reshape(-1, 3)).any(axis=1))
    assert got.tobytes() == w_recs.tobytes(), (b["name"], got[bad[:1]], w_recs[bad[:1]])
    table, lines = pat_format_host("chrP", base, w_recs)
    out, t2 = text_device(caller, d_rec, d_n, n + 2, "chrP", base, len(table))
    assert t2 == (len(table), lines) and out.tobytes() == table, b["name"]
    return got, tot


# ---- 1. the records -------------------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_block(caller):
    b = P.hand_block()
    got, tot = check_block(caller, b, base=P.HAND_INDEX_BASE)
    assert pat.unpack(got) == P.HAND_RECORDS and tot == P.HAND_TOTALS
    got, tot = check_block(caller, dict(b, params={"min_sites": 3}))
    assert pat.unpack(got) == P.HAND_RECORDS_3 and tot == P.HAND_TOTALS_3
    assert pat.format("chrP", P.HAND_INDEX_BASE, pat.unpack(got))[0] == P.HAND_TABLE_3


@pytest.mark.parametrize("b,want", P.cut_blocks(), ids=lambda v: v["name"] if isinstance(v, dict) else "")
def test_templates_cut_at_64_sites(caller, b, want):
    got, _ = check_block(caller, b)
    assert pat.unpack(got) == want


@pytest.mark.parametrize("b", P.placement_blocks(), ids=lambda b: "%s, %d sites" % (b["name"], len(pat.site_positions(b["x"], b["y"], b["ref"]))))
def test_placement_blocks(caller, b):
    if b["min_qual"] != 20:
        with B.SiteCaller(min_qual=b["min_qual"]) as c:
            got, tot = check_block(c, b)
    else:
        got, tot = check_block(caller, b)
    recs, p_tot = pat.patterns(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    assert pat.unpack(got) == recs and tot == p_tot


@pytest.mark.parametrize("n_pos,seed", P.TILE_EDGE_BLOCKS)
def test_block_lengths_around_a_tile(caller, n_pos, seed):
    b = P.dense_block(seed, n_pos, 60)
    got, tot = check_block(caller, b)
    assert tot[1] > 0 and len(got) >= 1
    check_block(caller, dict(b, params={"min_sites": 4}))


@pytest.fixture(scope="module")
def big():
    b = P.big_block()
    want = pat_recs_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    assert want[1] >= 1000 and all(v > 0 for v in want[2][:6])
    return b, want


def test_20003_positions(caller, big):
    b, want = big
    w_recs, n, wtot = want
    got, tot = check_block(caller, b, want)
    recs, p_tot = pat.patterns(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    assert pat.unpack(got) == recs and tot == p_tot
    # the same input twice gives the same bytes
    again, _, tot2 = run_device(caller, b, n)
    assert again.tobytes() == got.tobytes() and tot2 == tot
    # a room one short: counted, not stored, nothing behind the room (run_device checks the guard bytes); the full count is still reported
    part, count, tot3 = run_device(caller, b, n - 1)
    assert count == n and tot3 == wtot and part.tobytes() == w_recs[:-1].tobytes()
    none, count, tot4 = run_device(caller, b, 0)
    assert count == n and len(none) == 0 and tot4 == wtot
    check_block(caller, dict(b, params={"min_sites": 5}))


def test_20003_positions_on_a_one_cu_grid(one_cu, big):
    b, want = big
    check_block(one_cu, b, want)


@pytest.mark.parametrize("k", range(3))
def test_a_5000_base_read(caller, k):
    b = P.long_read_blocks()[k]
    got, tot = check_block(caller, b)
    if tot[7] == 2500 and b["params"]["min_sites"] == 1:
        assert tot[1] == 120 and tot[6] == 3  # three reads of 40 pieces


def test_5000_templates_identical_in_16_patterns_and_distinct(caller):
    got, tot = check_block(caller, P.identical_block(5000))
    assert pat.unpack(got) == [(0, "CTCT", 5000)] and tot == (1, 5000, 5000, 10000, 10000, 0, 0, 4)
    got, tot = check_block(caller, P.sixteen_block(5000))
    assert len(got) == 16 and set(got["idx"]) == {0} and sorted(got["count"]) == [312] * 8 + [313] * 8
    got, tot = check_block(caller, P.distinct_block(5000))
    assert len(got) == 5000 and (got["count"] == 1).all() and tot[:3] == (5000, 5000, 5000)


@pytest.mark.parametrize("n", P.PIECE_COUNTS)
def test_piece_counts_where_the_sort_and_the_heads_change_blocks(caller, n):
    got, tot = check_block(caller, P.distinct_block(n))
    assert len(got) == n and tot[1] == n
    got, tot = check_block(caller, P.identical_block(n))
    assert len(got) == min(n, 1) and tot[1] == n


def test_no_template_and_the_refusals(caller):
    b = P.dense_block(5, 300, 10)
    empty = dict(b, tpl=b["tpl"][:0], seq=b["seq"][:0], name="no template")
    got, tot = check_block(caller, empty)
    assert len(got) == 0 and tot[:7] == (0,) * 7 and tot[7] > 5
    run_device(caller, b, 64, params={"min_sites": 1, "reserved": 1}, expect_refusal=True)
    run_device(caller, dict(b, y=b["x"] - 1), 64, expect_refusal=True)
    check_block(caller, b)  # the context is usable behind the refusal


# ---- 2. the lines ---------------------------------------------------------------------------------------------------------------------------
def hand_made_records(n):
    """n records made by hand, in no order: patterns of 1 .. 64 sites, counts of 1 .. 10 digits, idx up to 2^32 - 2."""
    rng = np.random.default_rng(900 + n)
    recs = []
    for k in range(n):
        ln = (1, 64, 2, 33, 32, 63)[k % 6] if k < 12 else int(rng.integers(1, 65))
        s = "".join(".CT"[int(v)] for v in rng.integers(0, 3, ln))
        s = "CT"[k & 1] + s[1:-1] + ("TC"[k & 1] if ln > 1 else "")
        recs.append((int(min(10 ** int(rng.integers(0, 10)) * int(rng.integers(1, 10)), 0xFFFFFFFE)), s[:ln], int(min(10 ** int(rng.integers(0, 10)) * int(rng.integers(1, 10)), 0xFFFFFFFF))))
    if n > 3:
        recs[1] = (0xFFFFFFFE, "C" * 64, 0xFFFFFFFF)
        recs[2] = (0, "T", 1)
    return pat.pack(recs)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4113])
def test_text_device_equals_the_host_formatter(caller, n):
    recs = hand_made_records(n)
    d_rec = dev(recs) if n else torch.zeros(REC, dtype=torch.uint8, device="cuda")
    for name, base, count in (("chr1", 0, n), ("c", 9, n), ("x" * 255, 2 ** 63, n), ("chr1", 2 ** 32 - 1, n), ("chr1", 2 ** 63 - 2 ** 32, n // 2), ("chr1", 10 ** 16 - 5, n + 7)):
        d_n = torch.tensor([count], dtype=torch.int64, device="cuda")  # the device count decides, never beyond max_rec
        used = recs[: min(count, n)]
        want, lines = pat_format_host(name, base, used)
        assert (want, lines) == pat.format(name, base, used)
        out, t2 = text_device(caller, d_rec, d_n, n, name, base, len(want))
        assert t2 == (len(want), lines) and out.tobytes() == want, (n, name, base, count)
        if want:  # one short: the full length is reported, the stream is cut at a 64-record boundary
            out, t2 = text_device(caller, d_rec, d_n, n, name, base, len(want) - 1)
            assert t2 == (len(want), lines)
            whole = pat_format_host(name, base, used[: 64 * ((len(used) - 1) // 64)])[0]
            assert out[: len(whole)].tobytes() == whole and (out[len(whole) :] == PAD).all()
    if n >= 129:  # out_cap cuts the stream at a 64-record boundary exactly: the first tile alone is written, the full length reported
        d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
        want, lines = pat_format_host("chr1", 5, recs)
        first = pat_format_host("chr1", 5, recs[:64])[0]
        out, t2 = text_device(caller, d_rec, d_n, n, "chr1", 5, len(first))
        assert t2 == (len(want), lines) and out.tobytes() == first
        out, t2 = text_device(caller, d_rec, d_n, n, "chr1", 5, len(first) + 7)  # ... and nothing of the second
        assert t2 == (len(want), lines) and out[: len(first)].tobytes() == first and (out[len(first) :] == PAD).all()
    d_n = torch.tensor([n], dtype=torch.int64, device="cuda")
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(B.BscError):
            text_device(caller, d_rec, d_n, n, bad, 0, 64)
    with pytest.raises(B.BscError):
        text_device(caller, d_rec, d_n, n, "chr1", 0, 64, par=_lib.PatParams(1, 3))
    with pytest.raises(B.BscError):
        text_device(caller, d_rec, d_n, n, "chr1", 2 ** 63 + 1, 64)


def test_text_device_takes_the_walk_s_records_and_count(caller, big):
    b, (w_recs, n, _) = big
    d_rec, d_n, recs, count, _ = run_device(caller, b, n, keep=True)
    table, lines = pat_format_host("chr20", 123456, w_recs)
    out, t2 = text_device(caller, d_rec, d_n, n + GUARD, "chr20", 123456, len(table))  # the guard records are not lines
    assert t2 == (len(table), lines) and out.tobytes() == table and lines == n
    back = pat.read_pat(table)
    assert [(i - 123457, s, c) for _, i, s, c in back] == pat.unpack(w_recs)
    assert back == sorted(back, key=lambda r: (r[1], r[2].encode()))


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


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """A BAM of three contigs: chrA, 6 000 positions at ~40x with a heterozygous site every 300; chrT, 60 positions of CG A T CG ... (a block
    shorter than a tile, 20 sites); chrG, 30 000 positions in several blocks with gaps between the reads.  The reads carry clips and indels."""
    d = tmp_path_factory.mktemp("pat_files")
    rng = np.random.default_rng(4715)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50, err=0.0)
            + W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


PAR = {"min_sites": 2}


def sites_in_front(codes, x):
    """The contig's sites p < x, in Python."""
    c = np.asarray(codes[: max(x, 1)])
    return int(((c[:-1] == 2) & (c[1:] == 3))[: x - 1].sum())


def python_table(name, raw, seq, ms, x, y, ref, base, par=PAR):
    """The Python rule over the HOST pre-processing of a raw block: (table, lines, totals)."""
    tpl, pseq, _ = prepare_templates(raw, seq, ms)
    recs, tot = pat.patterns(tpl, pseq, x, y, ref, 20, par)
    table, lines = pat.format(name, base, recs, par)
    return table, lines, tot


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    n_blocks = n_short = n_lines = n_pieces = 0
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            base = sites_in_front(codes, x)
            assert base == pat_count_sites(codes, 1, x)
            raw, seq, ms = rd.fetch(blk)
            want, w_lines, w_tot = python_table(name, raw, seq, ms, x, y, ref, base)
            kw = dict(reg_stop=len(codes))
            n_short += y - x + 1 < 64
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, keep=True, **kw)
            ent0, r0 = caller.block_csi_kept(14)
            merge0 = caller.block_meth_kept(name, merge=True)
            reads0 = caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1})
            asm0 = caller.block_asm_kept(name)
            epi0 = caller.block_epi_kept(name, {"min_cov": 2})
            got, lines, tot = caller.block_pat_kept(name, PAR, index_base=base)
            assert got == want and lines == w_lines and tot == w_tot, (name, x)
            assert caller.block_pat_kept(name, PAR, index_base=base) == (got, lines, tot)  # twice: the same bytes
            n_lines += lines
            n_pieces += tot[1]
            # other parameters, another base
            for par, b2 in (({"min_sites": 1}, 0), ({"min_sites": 10}, 2 ** 40)):
                assert caller.block_pat_kept(name, par, index_base=b2) == python_table(name, raw, seq, ms, x, y, ref, b2, par), (name, x, par)
            # a room one short, then the exact room; a read past the end
            nb, nl, t8 = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
            pp = _lib.PatParams(**PAR)
            if got:
                assert L.bsc_block_pat_kept(h, name.encode(), C.byref(pp), base, len(got) - 1, C.byref(nb), C.byref(nl), t8) == -1
                assert nb.value == len(got) and b"dev_cap" in L.bsc_last_error() and tuple(int(v) for v in t8) == tot
                out = np.zeros(8, np.uint8)
                assert L.bsc_pat_stream_read(h, 0, 1, out.ctypes.data) == -1  # a refused call left no table
            assert L.bsc_block_pat_kept(h, name.encode(), C.byref(pp), base, max(len(got), 1), C.byref(nb), C.byref(nl), None) == 0
            assert (nb.value, nl.value) == (len(got), lines)
            assert caller.pat_stream_read(0, len(got)) == got
            out = np.zeros(len(got) + 8, np.uint8)
            assert L.bsc_pat_stream_read(h, 1, len(got), out.ctypes.data) == -1 and b"beyond" in L.bsc_last_error()
            # what the context keeps beside it is untouched
            assert kept_stream(caller, len(bcf0)) == bcf0
            ent1, r1 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() and r0 == r1 == n_rec
            assert caller.block_meth_kept(name, merge=True) == merge0
            assert caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1}) == reads0
            assert caller.block_asm_kept(name) == asm0
            assert caller.block_epi_kept(name, {"min_cov": 2}) == epi0
            assert caller.block_pat_kept(name, PAR, index_base=base)[0] == got  # ... and behind the other tables' calls
            # the refusals of the arguments leave the block where it is
            for bad_name, bad_par, bad_base in ((b"a\tb", pp, 0), (name.encode(), _lib.PatParams(2, 1), 0), (name.encode(), pp, 2 ** 63 + 1)):
                assert L.bsc_block_pat_kept(h, bad_name, C.byref(bad_par), bad_base, 1 << 20, C.byref(nb), C.byref(nl), None) == -1 and nb.value == 0
            # behind the text encoder's keep call: the same table
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, **kw)
            assert n_txt == n_rec
            assert caller.block_pat_kept(name, PAR, index_base=base) == (got, lines, tot)
            assert kept_stream(caller, len(text)) == text
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, **kw)
            assert L.bsc_block_pat_kept(h, name.encode(), C.byref(pp), base, 1 << 20, C.byref(nb), C.byref(nl), None) == -1
            assert b"no single block" in L.bsc_last_error() and nb.value == 0
            n_blocks += 1
    assert n_blocks > 4 and n_short >= 1 and n_lines > 100 and n_pieces > 1000, (n_blocks, n_short, n_lines, n_pieces)


def test_a_detached_table_goes_through_the_device_writer(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    with DeviceBamReader(caller, bam, threads=2) as rd:
        blk = next(iter(rd.device_blocks()))
        name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
        ref = block_reference(codes, int(blk.x), int(blk.y))
        caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
        full, lines, _ = caller.block_pat_kept(name, PAR)
        assert lines > 0
        p, nb = C.c_void_p(), C.c_uint64()
        assert L.bsc_pat_stream_detach(h, C.byref(p), C.byref(nb)) == 0 and nb.value == len(full) and p.value
        p2, nb2 = C.c_void_p(), C.c_uint64(9)
        assert L.bsc_pat_stream_detach(h, C.byref(p2), C.byref(nb2)) == -1 and not p2.value and nb2.value == 0  # once
        z = caller.bgzf()
        z.write_device(p.value, len(full))
        comp = z.take() + z.close()
        assert gzip.decompress(comp) == full and comp.endswith(vcf.BGZF_EOF)
        assert L.bsc_detached_free(h, p) == 0
        assert caller.block_pat_kept(name, PAR)[0] == full  # the next call takes a buffer again


def test_refused_before_any_block():
    with B.SiteCaller() as c:
        nb, nl = C.c_uint64(5), C.c_uint64(5)
        pp = _lib.PatParams()
        assert c._L.bsc_block_pat_kept(c._h, b"chr1", C.byref(pp), 0, 1 << 16, C.byref(nb), C.byref(nl), None) == -1
        assert b"no single block" in c._L.bsc_last_error() and (nb.value, nl.value) == (0, 0)


# ---- 4. file to file ------------------------------------------------------------------------------------------------------------------------
def run_exe(*args, env=None, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout
    return r


def file_table(caller, bam, refs, reference, par):
    """The concatenated per-block Python tables of a file, each with the running index_base of its contig, and the sums of their totals."""
    out, tot = [], np.zeros(8, np.int64)
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
            x, y = int(blk.x), int(blk.y)
            raw, seq, ms = rd.fetch(blk)
            table, _, t = python_table(name, raw, seq, ms, x, y, block_reference(codes, x, y), sites_in_front(codes, x), par)
            out.append(table)
            tot += np.array(t)
    return b"".join(out), tuple(int(v) for v in tot)


def stdout_line(table, tot):
    return "%d records in the per-read CpG pattern table, %d lines written (pieces %d, templates %d, C %d T %d)\n" % (
        tot[0], table.count(b"\n"), tot[1], tot[2], tot[3], tot[4])


def test_bam2bcf_meth_pat_and_pipeline(caller, small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("f" + s))  # noqa: E731
    rd = lambda path: open(path, "rb").read()  # noqa: E731
    want, tot = file_table(caller, bam, refs, reference, {"min_sites": 1})  # the default threshold
    assert tot[1] > 1000 and want.count(b"\n") > 500
    # sorted within each contig, by index and then pattern, no key twice; the index is the CpG's ordinal within its contig
    lines = pat.read_pat(want)
    for name, codes in reference.items():
        own = [(i, s.encode()) for c, i, s, _ in lines if c == name.encode()]
        assert own and own == sorted(set(own)) and own[0][0] >= 1 and own[-1][0] + len(own[-1][1]) - 1 <= sites_in_front(codes, len(codes) + 1)
    # plain: the table is the concatenated per-block tables; everything else as without the switch
    base = run_exe("--meth", p(".u.cpg"), "--meth-merge", "--meth-epialleles", p(".u.epi"), bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    out = run_exe("--meth-pat", p(".up.pat"), "--meth", p(".up.cpg"), "--meth-merge", "--meth-epialleles", p(".up.epi"), bam, fa, p(".up.bcf"), p(".up.json"), "S9")
    assert rd(p(".up.pat")) == want
    for a, b in ((".up.bcf", ".u.bcf"), (".up.json", ".u.json"), (".up.cpg", ".u.cpg"), (".up.epi", ".u.epi")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    assert out == base + stdout_line(want, tot)
    # the threshold
    want_t, tot_t = file_table(caller, bam, refs, reference, {"min_sites": 12})
    out = run_exe("--meth-pat", p(".t.pat"), "--meth-pat-min-sites", "12", bam, fa, p(".t.bcf"), p(".t.json"), "S9")
    assert rd(p(".t.pat")) == want_t and 0 < want_t.count(b"\n") < want.count(b"\n") and out.endswith(stdout_line(want_t, tot_t))
    # a name that ends in .gz: BGZF, whatever -O says; the main file is the uncompressed run's
    run_exe("--meth-pat", p(".g.pat.gz"), bam, fa, p(".g.bcf"), p(".g.json"), "S9")
    blob = rd(p(".g.pat.gz"))
    assert blob.endswith(vcf.BGZF_EOF) and csi_ref.inflate(blob) == want and rd(p(".g.bcf")) == rd(p(".u.bcf"))
    assert pat.read_pat(p(".g.pat.gz")) == lines
    # -O b --index: the inflated table is the plain one; the main file, its .csi, the report and the epiallele table are those of the run without
    opts = ["-O", "b", "--index", "--meth-epialleles"]
    base = run_exe(*opts, p(".b.epi"), bam, fa, p(".b.bcf"), p(".b.json"), "S9")
    out = run_exe(*opts, p(".bp.epi"), "--meth-pat", p(".bp.pat"), bam, fa, p(".bp.bcf"), p(".bp.json"), "S9")
    blob = rd(p(".bp.pat"))
    assert blob.endswith(vcf.BGZF_EOF) and csi_ref.inflate(blob) == want and out == base + stdout_line(want, tot)
    for a, b in ((".bp.bcf", ".b.bcf"), (".bp.bcf.csi", ".b.bcf.csi"), (".bp.json", ".b.json"), (".bp.epi", ".b.epi")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    # pipeline.run(pat_path=...) writes the same file, compressed or not
    for compressed in (False, True):
        out = p(".pipe%d" % compressed)
        s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, compressed=compressed, pat_path=out + ".pat",
                         pat_params={"min_sites": 12})
        got = rd(out + ".pat")
        got = csi_ref.inflate(got) if compressed else got
        assert got == want_t and s["pat_lines"] == want_t.count(b"\n") and s["pat_totals"] == tot_t
    s = pipeline.run(bam, reference, p(".pipeg"), sample="S9", benchmark_mode=True, device_reader=True, pat_path=p(".pipeg.pat.gz"))
    assert csi_ref.inflate(rd(p(".pipeg.pat.gz"))) == want and s["pat_lines"] == want.count(b"\n") and s["pat_totals"] == tot
    # refused where --meth-epialleles is: sharded runs, the host paths; no file is left behind
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), pat_path=p(".no.pat"))
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, pat_path=p(".no.pat"), shard_rank=0, shard_world=2)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, pat_params={"min_sites": 2})
    for args, env in ((["--rank", "0", "--world", "2"], None), ([], {"BAM2BCF_HOST_READER": "1"}), ([], {"BAM2BCF_HOST_BCF": "1"}), ([], {"BAM2BCF_HOST_PREP": "1"})):
        r = run_exe(*args, "--meth-pat", p(".no.pat"), bam, fa, p(".no"), p(".no.json"), env=env, ok=False)
        assert r.returncode == 2 and "--meth-pat" in r.stderr
    for args in (["--meth-pat-min-sites", "3"], ["--meth-pat", p(".no.pat"), "--meth-pat-min-sites", "x"], ["--meth-pat", p(".no.pat"), "--meth-pat-min-sites", "-1"]):
        r = run_exe(*args, bam, fa, p(".no"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--meth-pat" in r.stderr
    assert not os.path.exists(p(".no.pat"))
