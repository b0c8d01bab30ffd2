"""The epiallele table on the device (csrc/epidev.hip) — the rule of include/bscall_amd.h (WINDOW, PATTERN, RECORD, TOTALS, LINE over the
COUNTS, SITE, BYTE, STATE of the read-level CpG table):

  1. bsc_epi_device against the host form (csrc/epi.c) and the Python rule (bs_call_amd/epialleles.py), record for record and total for
     total, on the blocks of tests/epi_cases.py: the hand-worked block, the targeted blocks, block lengths around a tile, the long read, both
     contention blocks, 20 003 positions on the default and on a one-CU grid, a room one short, no template, the refusals
  2. bsc_epi_text_device against the host formatter over records made by hand and over the walk's own
  3. bsc_block_epi_kept behind both _keep calls on a device reader's blocks, against the Python rule over the host pre-processing of the same
     raw block; what the context keeps beside it is untouched
  4. bam2bcf --meth-epialleles and pipeline.run(epi_path=) file to file"""
import ctypes as C
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import cpg_reads_cases as K
import csi_ref
import epi_cases as E
from bs_call_amd import _lib, epialleles, pipeline, vcf
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import epi_format_host, epi_windows_host, prepare_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
PAD = 0xEE
GUARD = 3  # records of guard bytes behind the room
REC = 72
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


def run_device(caller, b, cap=None, params=None, expect_refusal=False, keep=False):
    """bsc_epi_device over a block of tests/epi_cases.py.  Returns (records[min(count, room)], count, totals) after checking the guard bytes
    behind the count and behind the room."""
    assert caller.params["min_qual"] == b["min_qual"]
    d_tpl, d_seq, d_ref = dev(b["tpl"]), dev(b["seq"]), dev(b["ref"])
    n_pos = b["y"] - b["x"] + 1
    room = (n_pos + 1) // 2 if cap is None else cap
    d_win = torch.full(((room + GUARD) * REC,), PAD, dtype=torch.uint8, device="cuda")
    d_n = torch.full((1,), FILL, dtype=torch.int64, device="cuda")
    d_tot = torch.full((8,), FILL, dtype=torch.int64, device="cuda")
    par = b["params"] if params is None else params
    args = (d_tpl.data_ptr(), len(b["tpl"]), d_seq.data_ptr(), len(b["seq"]), b["x"], b["y"], d_ref.data_ptr(), d_win.data_ptr(), room, d_n.data_ptr(),
            d_tot.data_ptr())
    if expect_refusal:
        with pytest.raises(B.BscError):
            caller.epi_device(*args, params=_lib.EpiParams(**par))
        torch.cuda.synchronize()
        assert (d_win.cpu().numpy() == PAD).all() and int(d_n.cpu()[0]) == FILL and (d_tot.cpu().numpy() == FILL).all()
        return None
    caller.epi_device(*args, params=par)
    torch.cuda.synchronize()
    count = int(d_n.cpu().numpy().view(np.uint64)[0])
    tot = tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64))
    out = d_win.cpu().numpy()
    stored = min(count, room)
    assert (out[stored * REC :] == PAD).all(), "bytes behind the count or behind the room were written"
    recs = out[: stored * REC].view(epialleles.WINDOW)
    if keep:
        return d_win, d_n, recs, count, tot
    return recs, count, tot


def check_block(caller, b, python_too=True):
    want, n, wtot = epi_windows_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    got, count, tot = run_device(caller, b)
    assert count == n == len(want), (b["name"], count, n)
    assert tot == wtot, (b["name"], tot, wtot)
    bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 18) != want.view(np.uint32).reshape(-1, 18)).any(axis=1))
    assert got.tobytes() == want.tobytes(), (b["name"], got[bad[:1]], want[bad[:1]])
    if python_too:
        p_recs, p_tot = epialleles.windows(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
        assert p_recs.tobytes() == got.tobytes() and p_tot == tot, b["name"]
    return got, tot


# ---- 1. the records -------------------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_block(caller):
    got, tot = check_block(caller, E.hand_block())
    assert E.as_tuples(got) == E.HAND_RECORDS and tot == E.HAND_TOTALS
    got, tot = check_block(caller, dict(K.hand_block(), params=E.PAR))
    assert E.as_tuples(got) == E.ANCHOR_RECORDS and tot == E.ANCHOR_TOTALS


@pytest.mark.parametrize("n_pos,seed", E.TILE_EDGE_BLOCKS)
def test_block_lengths_around_a_tile(caller, n_pos, seed):
    got, tot = check_block(caller, E.dense_block(seed, n_pos, 60))
    assert tot[1] > 0 and len(got) >= 1


@pytest.fixture(scope="module")
def big():
    b = E.big_block()
    want, n, tot = epi_windows_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    assert int((want["c"].sum(axis=1) > 0).sum()) >= 1000 and all(v > 0 for v in tot[:5])
    return b, want, tot


def test_20003_positions(caller, big):
    b, want, wtot = big
    got, count, tot = run_device(caller, b)
    assert count == len(want) and tot == wtot and got.tobytes() == want.tobytes()
    p_recs, p_tot = epialleles.windows(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    assert p_recs.tobytes() == got.tobytes() and p_tot == tot
    # the same input twice gives the same bytes
    again, _, tot2 = run_device(caller, b)
    assert again.tobytes() == got.tobytes() and tot2 == tot
    # a room one short, then exact: counted, not stored, nothing behind the room (run_device checks the guard bytes)
    part, count, tot3 = run_device(caller, b, cap=len(want) - 1)
    assert count == len(want) and tot3 == wtot and part.tobytes() == want[:-1].tobytes()
    exact, count, _ = run_device(caller, b, cap=len(want))
    assert count == len(want) and exact.tobytes() == want.tobytes()
    none, count, tot4 = run_device(caller, b, cap=0)
    assert count == len(want) and len(none) == 0 and tot4 == wtot


def test_20003_positions_on_a_one_cu_grid(one_cu, big):
    b, want, wtot = big
    got, count, tot = run_device(one_cu, b)
    assert count == len(want) and tot == wtot and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("b", E.targeted_blocks(), ids=lambda b: b["name"])
def test_targeted_blocks(caller, b):
    got, _ = check_block(caller, b)
    if b["name"] == "mates":
        assert E.as_tuples(got) == E.MATES_RECORDS


def test_a_long_read(caller):
    got, tot = check_block(caller, E.long_read_block())
    assert tot[0] == 2497 and tot[2] == 3 and tot[1] > 6000


def test_contention(caller):
    got, tot = check_block(caller, E.contention_block(5000))
    assert E.as_tuples(got) == [E.rec(53, 18, c5=5000)] and tot == (1, 5000, 5000, 10000, 5000, 0, 0, 0)
    got, tot = check_block(caller, E.contention_block(5000, spread=True))
    assert E.as_tuples(got) == [(53, 18, [313] * 8 + [312] * 8)] and tot[:3] == (1, 5000, 5000)


def test_no_template_and_the_refusals(caller):
    b = E.dense_block(5, 300, 10)
    empty = dict(b, tpl=b["tpl"][:0], seq=b["seq"][:0], name="no template")
    got, tot = check_block(caller, empty)
    assert len(got) > 5 and tot == (len(got), 0, 0, 0, 0, 0, 0, 0) and not got["c"].any() and (got["span"] >= 6).all()
    run_device(caller, b, params={"min_cov": 1, "reserved": 1}, expect_refusal=True)
    check_block(caller, b)  # the context is usable behind the refusal


# ---- 2. the lines ---------------------------------------------------------------------------------------------------------------------------
def text_device(caller, d_win, d_n, max_win, contig, par, cap):
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_t2 = torch.full((2,), FILL, dtype=torch.int64, device="cuda")
    try:
        caller.epi_text_device(d_win.data_ptr(), d_n.data_ptr(), max_win, contig, d_out.data_ptr(), cap, d_t2.data_ptr(), params=par)
    except B.BscError:
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == PAD).all() and (d_t2.cpu().numpy() == FILL).all(), "a refusal wrote something"
        raise
    torch.cuda.synchronize()
    t2 = tuple(int(v) for v in d_t2.cpu().numpy().view(np.uint64))
    out = d_out.cpu().numpy()
    assert (out[cap:] == PAD).all(), "bytes behind the room were written"
    return out[:cap], t2


def hand_made_records(n):
    """n records made by hand: counts of 1 .. 10 digits, empty windows, windows of n = 1, and the extreme ones (2^32 - 1 in one code and in
    all sixteen, pos at 1 and at 2^32 - 2 - span)."""
    rng = np.random.default_rng(700 + n)
    recs = np.zeros(n, epialleles.WINDOW)
    recs["pos"] = (10 ** rng.integers(0, 9, n) * rng.integers(1, 10, n)).clip(1, 0x7FFFFFFF)
    recs["span"] = rng.integers(6, 5000, n)
    recs["c"] = np.where(rng.random((n, 16)) < 0.6, 0, 10 ** rng.integers(0, 10, (n, 16)) * rng.integers(1, 10, (n, 16))).clip(0, 0xFFFFFFFF)
    recs["c"][::5] = 0
    recs["c"][2::5] = 0
    recs["c"][2::5, 7] = 1
    top = 0xFFFFFFFF
    extreme = [(1, 6, [0] * 9 + [top] + [0] * 6), (1, 60, [top] * 16), (top - 1 - 6, 6, [top] * 16), (top - 1 - 4000, 4000, [1] + [0] * 15)]
    for k, r in enumerate(extreme):
        if 5 + k < n:
            recs[5 + k] = r
    return recs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4113])
def test_text_device_equals_the_host_formatter(caller, n):
    recs = hand_made_records(n)
    d_win = dev(recs) if n else torch.zeros(REC, dtype=torch.uint8, device="cuda")
    for name, mc, count in (("chr1", 1, n), ("c", 10, n), ("x" * 255, 0, n), ("chr1", 0xFFFFFFFF, n), ("chr1", 1, n // 2), ("chr1", 1, n + 7)):
        par = {"min_cov": mc}
        d_n = torch.tensor([count], dtype=torch.int64, device="cuda")  # the device count decides, never beyond max_win
        used = recs[: min(count, n)]
        want, lines = epi_format_host(name, used, par)
        assert (want, lines) == epialleles.format(name, used, par)
        out, t2 = text_device(caller, d_win, d_n, n, name, par, len(want))
        assert t2 == (len(want), lines) and out.tobytes() == want, (n, name, mc, count)
        if want:  # one short: the full length is reported, the stream is cut at a 64-record boundary
            out, t2 = text_device(caller, d_win, d_n, n, name, par, len(want) - 1)
            assert t2 == (len(want), lines)
            k = (len(used) - 1) // 64  # the tiles of 64 records that end in front of the room's end: the last line may lie in an earlier tile
            while k and len(epi_format_host(name, used[: 64 * k], par)[0]) >= len(want):
                k -= 1
            whole = epi_format_host(name, used[: 64 * k], par)[0]
            assert out[: len(whole)].tobytes() == whole and (out[len(whole) :] == PAD).all()
    if n >= 129:  # out_cap cuts the stream at a 64-record boundary exactly: the first tile alone is written, the full length reported
        par, d_n = {"min_cov": 1}, torch.tensor([n], dtype=torch.int64, device="cuda")
        want, lines = epi_format_host("chr1", recs, par)
        first = epi_format_host("chr1", recs[:64], par)[0]
        out, t2 = text_device(caller, d_win, d_n, n, "chr1", par, len(first))
        assert t2 == (len(want), lines) and out.tobytes() == first
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(B.BscError):
            text_device(caller, d_win, torch.tensor([n], dtype=torch.int64, device="cuda"), n, bad, {"min_cov": 1}, 64)
    with pytest.raises(B.BscError):
        text_device(caller, d_win, torch.tensor([n], dtype=torch.int64, device="cuda"), n, "chr1", _lib.EpiParams(1, 3), 64)


def test_text_device_takes_the_walk_s_records_and_count(caller, big):
    b, want, _ = big
    d_win, d_n, recs, count, _ = run_device(caller, b, keep=True)
    for mc in (1, 10):
        table, lines = epi_format_host("chr20", want, {"min_cov": mc})
        out, t2 = text_device(caller, d_win, d_n, len(want) + GUARD, "chr20", {"min_cov": mc}, len(table))  # the guard records are not lines
        assert t2 == (len(table), lines) and out.tobytes() == table and lines > 100
    table = epi_format_host("chr20", want, E.PAR)[0]
    assert epialleles.read_table(table)[1].tobytes() == want[want["c"].sum(axis=1) > 0].tobytes()


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
    shorter than a tile, 20 sites); chrG, 30 000 positions in several blocks with gaps between the reads."""
    d = tmp_path_factory.mktemp("epi_files")
    rng = np.random.default_rng(4714)
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


PAR = {"min_cov": 2}


def python_table(name, raw, seq, ms, x, y, ref, par=PAR):
    """The Python rule over the HOST pre-processing of a raw block: (table, lines, totals)."""
    tpl, pseq, _ = prepare_templates(raw, seq, ms)
    recs, tot = epialleles.windows(tpl, pseq, x, y, ref, 20, par)
    table, lines = epialleles.format(name, recs, par)
    return table, lines, tot


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    n_blocks = n_short = n_lines = n_obs = 0
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            raw, seq, ms = rd.fetch(blk)
            want, w_lines, w_tot = python_table(name, raw, seq, ms, x, y, ref)
            kw = dict(reg_stop=len(codes))
            n_short += y - x + 1 < 64
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, keep=True, **kw)
            ent0, r0 = caller.block_csi_kept(14)
            merge0 = caller.block_meth_kept(name, merge=True)
            reads0 = caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1})
            got, lines, tot = caller.block_epi_kept(name, PAR)
            assert got == want and lines == w_lines and tot == w_tot, (name, x)
            assert caller.block_epi_kept(name, PAR) == (got, lines, tot)  # twice: the same bytes
            n_lines += lines
            n_obs += tot[1]
            # other parameters
            for par in ({"min_cov": 1}, {"min_cov": 10}):
                assert caller.block_epi_kept(name, par) == python_table(name, raw, seq, ms, x, y, ref, par), (name, x, par)
            # a room one short, then the exact room; a read past the end
            nb, nl, t8 = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
            ep = _lib.EpiParams(**PAR)
            if got:
                assert L.bsc_block_epi_kept(h, name.encode(), C.byref(ep), len(got) - 1, C.byref(nb), C.byref(nl), t8) == -1
                assert nb.value == len(got) and b"dev_cap" in L.bsc_last_error() and tuple(int(v) for v in t8) == tot
                out = np.zeros(8, np.uint8)
                assert L.bsc_epi_stream_read(h, 0, 1, out.ctypes.data) == -1  # a refused call left no table
            assert L.bsc_block_epi_kept(h, name.encode(), C.byref(ep), max(len(got), 1), C.byref(nb), C.byref(nl), None) == 0
            assert (nb.value, nl.value) == (len(got), lines)
            assert caller.epi_stream_read(0, len(got)) == got
            out = np.zeros(len(got) + 8, np.uint8)
            assert L.bsc_epi_stream_read(h, 1, len(got), out.ctypes.data) == -1 and b"beyond" in L.bsc_last_error()
            # what the context keeps beside it is untouched
            assert kept_stream(caller, len(bcf0)) == bcf0
            ent1, r1 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() and r0 == r1 == n_rec
            assert caller.block_meth_kept(name, merge=True) == merge0
            assert caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1}) == reads0
            assert caller.block_epi_kept(name, PAR)[0] == got  # ... and behind the other tables' calls
            # the refusals of the arguments leave the block where it is
            for bad_name, bad_par in ((b"a\tb", ep), (name.encode(), _lib.EpiParams(2, 1))):
                assert L.bsc_block_epi_kept(h, bad_name, C.byref(bad_par), 1 << 20, C.byref(nb), C.byref(nl), None) == -1 and nb.value == 0
            # behind the text encoder's keep call: the same table
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, **kw)
            assert n_txt == n_rec
            assert caller.block_epi_kept(name, PAR) == (got, lines, tot)
            assert kept_stream(caller, len(text)) == text
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, **kw)
            assert L.bsc_block_epi_kept(h, name.encode(), C.byref(ep), 1 << 20, C.byref(nb), C.byref(nl), None) == -1
            assert b"no single block" in L.bsc_last_error() and nb.value == 0
            n_blocks += 1
    assert n_blocks > 4 and n_short >= 1 and n_lines > 100 and n_obs > 1000, (n_blocks, n_short, n_lines, n_obs)


def test_a_detached_table_goes_through_the_device_writer(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    with DeviceBamReader(caller, bam, threads=2) as rd:
        blk = next(iter(rd.device_blocks()))
        name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
        ref = block_reference(codes, int(blk.x), int(blk.y))
        caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
        full, lines, _ = caller.block_epi_kept(name, PAR)
        assert lines > 0
        p, nb = C.c_void_p(), C.c_uint64()
        assert L.bsc_epi_stream_detach(h, C.byref(p), C.byref(nb)) == 0 and nb.value == len(full) and p.value
        p2, nb2 = C.c_void_p(), C.c_uint64(9)
        assert L.bsc_epi_stream_detach(h, C.byref(p2), C.byref(nb2)) == -1 and not p2.value and nb2.value == 0  # once
        z = caller.bgzf()
        z.write_device(p.value, len(full))
        comp = z.take() + z.close()
        assert gzip.decompress(comp) == full and comp.endswith(vcf.BGZF_EOF)
        assert L.bsc_detached_free(h, p) == 0
        assert caller.block_epi_kept(name, PAR)[0] == full  # the next call takes a buffer again


def test_refused_before_any_block():
    with B.SiteCaller() as c:
        nb, nl = C.c_uint64(5), C.c_uint64(5)
        ep = _lib.EpiParams()
        assert c._L.bsc_block_epi_kept(c._h, b"chr1", C.byref(ep), 1 << 16, C.byref(nb), C.byref(nl), None) == -1
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
            name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
            x, y = int(blk.x), int(blk.y)
            raw, seq, ms = rd.fetch(blk)
            table, _, t = python_table(name, raw, seq, ms, x, y, block_reference(codes, x, y), par)
            out.append(table)
            tot += np.array(t)
    return b"".join(out), tuple(int(v) for v in tot)


def stdout_line(table, tot):
    return "%d windows of four CpGs in the epiallele table, %d lines written (patterns %d, templates with one %d)\n" % (tot[0], table.count(b"\n"), tot[1], tot[2])


def test_bam2bcf_meth_epialleles_and_pipeline(caller, small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("f" + s))
    rd = lambda path: open(path, "rb").read()
    want, tot = file_table(caller, bam, refs, reference, {"min_cov": 10})  # the default threshold
    assert tot[1] > 1000 and want.count(b"\n") > 50
    # plain: the table is the concatenated per-block tables; everything else as without the switch
    base = run_exe("--meth", p(".u.cpg"), "--meth-merge", "--meth-reads", p(".u.reads"), bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    out = run_exe("--meth-epialleles", p(".ue.tsv"), "--meth", p(".ue.cpg"), "--meth-merge", "--meth-reads", p(".ue.reads"), bam, fa, p(".ue.bcf"), p(".ue.json"),
                  "S9")
    assert rd(p(".ue.tsv")) == want
    for a, b in ((".ue.bcf", ".u.bcf"), (".ue.json", ".u.json"), (".ue.cpg", ".u.cpg"), (".ue.reads", ".u.reads")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    assert out == base + stdout_line(want, tot)
    # every line's start is the start of a --meth-reads line: the tables join
    starts = {(ln.split(b"\t")[0], ln.split(b"\t")[1]) for ln in rd(p(".u.reads")).splitlines()}
    assert all((ln.split(b"\t")[0], ln.split(b"\t")[1]) in starts for ln in want.splitlines())
    # the threshold
    want_t, tot_t = file_table(caller, bam, refs, reference, {"min_cov": 2})
    out = run_exe("--meth-epialleles", p(".t.tsv"), "--meth-epialleles-min-cov", "2", bam, fa, p(".t.bcf"), p(".t.json"), "S9")
    assert rd(p(".t.tsv")) == want_t and want_t.count(b"\n") > want.count(b"\n") and out.endswith(stdout_line(want_t, tot_t)) and tot_t == tot
    # a name that ends in .gz: BGZF, whatever -O says; the main file is the uncompressed run's
    out = run_exe("--meth-epialleles", p(".g.tsv.gz"), bam, fa, p(".g.bcf"), p(".g.json"), "S9")
    blob = rd(p(".g.tsv.gz"))
    assert blob.endswith(vcf.BGZF_EOF) and csi_ref.inflate(blob) == want and rd(p(".g.bcf")) == rd(p(".u.bcf"))
    # -O b --index: the inflated table is the plain one; the main file, its .csi, the report and the merge table are those of the run without
    opts = ["-O", "b", "--index", "--meth", p(".b.cpg.gz"), "--meth-merge"]
    base = run_exe(*opts, bam, fa, p(".b.bcf"), p(".b.json"), "S9")
    out = run_exe(*opts[:4], p(".be.cpg.gz"), "--meth-merge", "--meth-epialleles", p(".be.tsv"), bam, fa, p(".be.bcf"), p(".be.json"), "S9")
    blob = rd(p(".be.tsv"))
    assert blob.endswith(vcf.BGZF_EOF) and csi_ref.inflate(blob) == want and out == base + stdout_line(want, tot)
    for a, b in ((".be.bcf", ".b.bcf"), (".be.bcf.csi", ".b.bcf.csi"), (".be.json", ".b.json"), (".be.cpg.gz", ".b.cpg.gz")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    # --meth-bgzf compresses the table of an uncompressed run
    run_exe("--meth-bgzf", "--meth-epialleles", p(".z.tsv"), bam, fa, p(".z.bcf"), p(".z.json"), "S9")
    assert csi_ref.inflate(rd(p(".z.tsv"))) == want and rd(p(".z.bcf")) == rd(p(".u.bcf"))
    # pipeline.run(epi_path=...) writes the same file, compressed or not
    for compressed in (False, True):
        out = p(".pipe%d" % compressed)
        s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, compressed=compressed, epi_path=out + ".tsv",
                         epi_params={"min_cov": 2})
        got = rd(out + ".tsv")
        got = csi_ref.inflate(got) if compressed else got
        assert got == want_t and s["epi_lines"] == want_t.count(b"\n") and s["epi_totals"] == tot_t
    s = pipeline.run(bam, reference, p(".pipeg"), sample="S9", benchmark_mode=True, device_reader=True, epi_path=p(".pipeg.tsv.gz"))
    assert csi_ref.inflate(rd(p(".pipeg.tsv.gz"))) == want and s["epi_lines"] == want.count(b"\n")
    # refused where --meth-reads is: sharded runs, the host paths; no file is left behind
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), epi_path=p(".no.tsv"))
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, epi_path=p(".no.tsv"), shard_rank=0, shard_world=2)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, epi_params={"min_cov": 2})
    for args, env in ((["--rank", "0", "--world", "2"], None), ([], {"BAM2BCF_HOST_READER": "1"}), ([], {"BAM2BCF_HOST_BCF": "1"}), ([], {"BAM2BCF_HOST_PREP": "1"})):
        r = run_exe(*args, "--meth-epialleles", p(".no.tsv"), bam, fa, p(".no"), p(".no.json"), env=env, ok=False)
        assert r.returncode == 2 and "--meth-epialleles" in r.stderr
    for args in (["--meth-epialleles-min-cov", "3"], ["--meth-epialleles", p(".no.tsv"), "--meth-epialleles-min-cov", "x"],
                 ["--meth-epialleles", p(".no.tsv"), "--meth-epialleles-min-cov", "-1"]):
        r = run_exe(*args, bam, fa, p(".no"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--meth-epialleles" in r.stderr
    assert not os.path.exists(p(".no.tsv"))
