"""The read-level CpG concordance table on the device (csrc/cpgreadsdev.hip) — the rule of include/bscall_amd.h (COUNTS, SITE, BYTE, STATE,
RECORD, TOTALS, LINE):

  1. bsc_cpg_reads_device against the host form (csrc/cpgreads.c) and the Python rule (bs_call_amd/cpgreads.py), record for record and total
     for total, on synthetic templates: block lengths around a tile, 20 003 positions, a one-CU grid, the targeted blocks of
     tests/cpg_reads_cases.py, contention, no template, no site, a room one short, the refusal, and twice the same bytes
  2. bsc_cpg_reads_text_device against the host formatter over the same records
  3. bsc_block_cpg_reads_kept behind both _keep calls on a device reader's blocks, against the Python rule over the host pre-processing of
     the same raw block, and against the caller's own counts; what the context keeps beside it is untouched
  4. bam2bcf --meth-reads and pipeline.run(cpg_reads_path=) file to file"""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import cpg_reads_cases as K
import csi_ref
from bs_call_amd import _lib, cpgreads, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import cpg_reads_format_host, cpg_reads_sites_host, prepare_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
PAD = 0xEE
GUARD = 3  # records of guard bytes behind the room


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
    """bsc_cpg_reads_device over a block of tests/cpg_reads_cases.py.  Returns (records[min(count, room)], count, totals) after checking the
    guard bytes behind the count and behind the room."""
    assert caller.params["min_qual"] == b["min_qual"]
    d_tpl, d_seq, d_ref = dev(b["tpl"]), dev(b["seq"]), dev(b["ref"])
    n_pos = b["y"] - b["x"] + 1
    room = (n_pos + 1) // 2 if cap is None else cap
    d_sites = torch.full(((room + GUARD) * 40,), PAD, dtype=torch.uint8, device="cuda")
    d_n = torch.full((1,), 0x7777777777777777, dtype=torch.int64, device="cuda")
    d_tot = torch.full((8,), 0x7777777777777777, dtype=torch.int64, device="cuda")
    par = b["params"] if params is None else params
    args = (d_tpl.data_ptr(), len(b["tpl"]), d_seq.data_ptr(), len(b["seq"]), b["x"], b["y"], d_ref.data_ptr(), d_sites.data_ptr(), room, d_n.data_ptr(),
            d_tot.data_ptr())
    if expect_refusal:
        with pytest.raises(B.BscError):
            caller.cpg_reads_device(*args, params=_lib.CpgReadsParams(**par))
        torch.cuda.synchronize()
        assert (d_sites.cpu().numpy() == PAD).all() and int(d_n.cpu()[0]) == 0x7777777777777777 and (d_tot.cpu().numpy() == 0x7777777777777777).all()
        return None
    caller.cpg_reads_device(*args, params=par)
    torch.cuda.synchronize()
    count = int(d_n.cpu().numpy().view(np.uint64)[0])
    tot = tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64))
    out = d_sites.cpu().numpy()
    stored = min(count, room)
    assert (out[stored * 40 :] == PAD).all(), "bytes behind the count or behind the room were written"
    recs = out[: stored * 40].view(cpgreads.SITE)
    if keep:
        return d_sites, d_n, recs, count, tot
    return recs, count, tot


def check_block(caller, b, python_too=True):
    want, n, wtot = cpg_reads_sites_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    got, count, tot = run_device(caller, b)
    assert count == n == len(want), (b["name"], count, n)
    assert tot == wtot, (b["name"], tot, wtot)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1, 10) != want.view(np.uint32).reshape(-1, 10))
    assert got.tobytes() == want.tobytes(), (b["name"], got[bad[:1] // 10], want[bad[:1] // 10])
    if python_too:
        p_recs, p_tot = cpgreads.sites(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
        assert p_recs.tobytes() == got.tobytes() and p_tot == tot, b["name"]
    return got, tot


# ---- 1. the records -------------------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_block(caller):
    b = K.hand_block()
    got, tot = check_block(caller, b)
    assert [tuple(int(v) for v in r) for r in got] == K.HAND_RECORDS and tot == K.HAND_TOTALS


@pytest.mark.parametrize("n_pos", [63, 64, 65, 127, 128, 129])
def test_block_lengths_around_a_tile(caller, n_pos):
    for seed in (0, 1):
        got, tot = check_block(caller, K.random_block(100 * n_pos + seed, n_pos, 60))
        assert tot[1] + tot[2] > 0 and len(got) > 3


@pytest.fixture(scope="module")
def big():
    b = K.random_block(20003, 20_003, 3_000, params={"min_sites": 4, "min_cov": 1})
    want, n, tot = cpg_reads_sites_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["min_qual"], b["params"])
    assert all(v > 0 for v in tot[:7]) and tot[6] < tot[5] < tot[4]
    return b, want, tot


def test_20003_positions(caller, big):
    b, want, wtot = big
    got, count, tot = run_device(caller, b)
    assert count == len(want) and tot == wtot and got.tobytes() == want.tobytes()
    # the same input twice gives the same bytes
    again, _, tot2 = run_device(caller, b)
    assert again.tobytes() == got.tobytes() and tot2 == tot
    # a room one short, then exact: counted, not stored, nothing behind the room
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


@pytest.mark.parametrize("b", K.targeted_blocks(), ids=lambda b: b["name"])
def test_targeted_blocks(caller, b):
    if b["min_qual"] != 20:
        with B.SiteCaller(min_qual=b["min_qual"]) as c:
            check_block(c, b)
    else:
        check_block(caller, b)


def test_a_long_read(caller):
    got, tot = check_block(caller, K.long_read_block())
    assert tot[0] == 80 and tot[4] == 3


def test_contention(caller):
    b = K.contention_block(5000)
    got, tot = check_block(caller, b, python_too=False)
    x = b["x"]
    assert [tuple(int(v) for v in r) for r in got] == [(x + 3, 6, 5000, 0, 5000, 5000, 0, 5000, 0, 0), (x + 9, 0, 0, 5000, 5000, 5000, 0, 0, 0, 0)]
    assert tot == (2, 5000, 5000, 5000, 5000, 5000, 5000, 0)


def test_no_template_no_site_and_the_refusal(caller):
    b = K.random_block(5, 300, 10)
    empty = dict(b, tpl=b["tpl"][:0], seq=b["seq"][:0], name="no template")
    got, tot = check_block(caller, empty)
    assert len(got) > 10 and tot == (len(got), 0, 0, 0, 0, 0, 0, 0) and not got["m"].any()
    bare = dict(b, ref=np.where(b["ref"] == 3, 1, b["ref"]).astype(np.uint8), name="no site")
    got, tot = check_block(caller, bare)
    assert len(got) == 0 and tot == (0,) * 8
    run_device(caller, b, params={"min_sites": 0, "min_cov": 1}, expect_refusal=True)
    check_block(caller, b)  # the context is usable behind the refusal


# ---- 2. the lines ---------------------------------------------------------------------------------------------------------------------------
def text_device(caller, d_sites, d_n, max_sites, contig, par, cap):
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_t2 = torch.full((2,), 0x7777777777777777, dtype=torch.int64, device="cuda")
    caller.cpg_reads_text_device(d_sites.data_ptr(), d_n.data_ptr(), max_sites, contig, d_out.data_ptr(), cap, d_t2.data_ptr(), params=par)
    torch.cuda.synchronize()
    t2 = tuple(int(v) for v in d_t2.cpu().numpy().view(np.uint64))
    out = d_out.cpu().numpy()
    assert (out[cap:] == PAD).all(), "bytes behind the room were written"
    return out[:cap], t2


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4113])
def test_text_device_equals_the_host_formatter(caller, n):
    rng = np.random.default_rng(700 + n)
    recs = np.zeros(n, cpgreads.SITE)
    for f in cpgreads.SITE.names:  # numbers of 1 .. 10 digits
        recs[f] = (10 ** rng.integers(0, 10, n) * rng.integers(1, 10, n)).clip(1, 0xFFFFFFFF)
    recs["m"][::5] = 0
    recs["u"][::5] = 0
    recs["m"][2::5] = 1
    recs["u"][2::5] = 0
    if n > 5:
        recs[5] = (0xFFFFFFFF,) * 10
    d_sites = dev(recs) if n else torch.zeros(40, dtype=torch.uint8, device="cuda")
    for name, mc, count in (("chr1", 1, n), ("c", 2, n), ("x" * 255, 0, n), ("chr1", 1, n // 2), ("chr1", 1, n + 7)):
        par = {"min_sites": 4, "min_cov": mc}
        d_n = torch.tensor([count], dtype=torch.int64, device="cuda")  # the device count decides, never beyond max_sites
        used = recs[: min(count, n)]
        want, lines = cpg_reads_format_host(name, used, par)
        assert (want, lines) == cpgreads.format(name, used, par)
        out, t2 = text_device(caller, d_sites, d_n, n, name, par, len(want))
        assert t2 == (len(want), lines) and out.tobytes() == want, (n, name, mc, count)
        if want:  # one short: the full length is reported, the stream is cut at a 64-record boundary
            out, t2 = text_device(caller, d_sites, d_n, n, name, par, len(want) - 1)
            assert t2 == (len(want), lines)
            whole = cpg_reads_format_host(name, used[: (len(used) - 1) // 64 * 64], par)[0]
            assert out[: len(whole)].tobytes() == whole and (out[len(whole) :] == PAD).all()
    for bad in ("", "x" * 256, "a\tb", "a\nb"):
        with pytest.raises(B.BscError):
            text_device(caller, d_sites, torch.tensor([n], dtype=torch.int64, device="cuda"), n, bad, {}, 64)


def test_text_device_takes_the_walk_s_records_and_count(caller, big):
    b, want, _ = big
    d_sites, d_n, recs, count, _ = run_device(caller, b, keep=True)
    table, lines = cpg_reads_format_host("chr20", want, b["params"])
    out, t2 = text_device(caller, d_sites, d_n, len(want) + GUARD, "chr20", b["params"], len(table))  # the guard records are not lines
    assert t2 == (len(table), lines) and out.tobytes() == table and lines > 100
    assert cpgreads.read_table(table)[1].tobytes() == want[(want["m"] + want["u"]) > 0].tobytes()


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
    """A BAM of three contigs: chrA, 6 000 positions at ~40x with a heterozygous site every 300; chrT, 60 positions (a block shorter than a
    tile); chrG, 30 000 positions in several blocks with gaps between the reads."""
    d = tmp_path_factory.mktemp("cpg_reads_files")
    rng = np.random.default_rng(4713)
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


PAR = {"min_sites": 3, "min_cov": 1}


def python_table(name, raw, seq, ms, x, y, ref, par=PAR):
    """The Python rule over the HOST pre-processing of a raw block: (table, lines, totals, records, templates with two counting bytes at a
    position)."""
    tpl, pseq, _ = prepare_templates(raw, seq, ms)
    recs, tot = cpgreads.sites(tpl, pseq, x, y, ref, 20, par)
    table, lines = cpgreads.format(name, recs, par)
    return table, lines, tot, recs, cpgreads.double_covered(tpl, pseq, x, y, 20)


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    n_blocks = n_short = n_lines = n_compared = n_disc = 0
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            raw, seq, ms = rd.fetch(blk)
            want, w_lines, w_tot, w_recs, doubles = python_table(name, raw, seq, ms, x, y, ref)
            assert doubles == 0, "the fixture must have no template with two counting bytes at one position"
            kw = dict(reg_stop=len(codes))
            n_short += y - x + 1 < 64
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, keep=True, **kw)
            ent0, r0 = caller.block_csi_kept(14)
            merge0 = caller.block_meth_kept(name, merge=True)
            got, lines, tot = caller.block_cpg_reads_kept(name, PAR)
            assert got == want and lines == w_lines and tot == w_tot, (name, x)
            assert caller.block_cpg_reads_kept(name, PAR) == (got, lines, tot)  # twice: the same bytes
            n_lines += lines
            n_disc += tot[6]
            # other parameters
            for par in ({"min_sites": 1, "min_cov": 3}, {"min_sites": 9, "min_cov": 1}):
                w = python_table(name, raw, seq, ms, x, y, ref, par)
                assert caller.block_cpg_reads_kept(name, par) == w[:3], (name, x, par)
            # a room one short, then the exact room; a read past the end
            nb, nl, t8 = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
            cp = _lib.CpgReadsParams(**PAR)
            if got:
                assert L.bsc_block_cpg_reads_kept(h, name.encode(), C.byref(cp), len(got) - 1, C.byref(nb), C.byref(nl), t8) == -1
                assert nb.value == len(got) and b"dev_cap" in L.bsc_last_error() and tuple(int(v) for v in t8) == tot
                out = np.zeros(8, np.uint8)
                assert L.bsc_cpg_reads_stream_read(h, 0, 1, out.ctypes.data) == -1  # a refused call left no table
            assert L.bsc_block_cpg_reads_kept(h, name.encode(), C.byref(cp), max(len(got), 1), C.byref(nb), C.byref(nl), None) == 0
            assert (nb.value, nl.value) == (len(got), lines)
            assert caller.cpg_reads_stream_read(0, len(got)) == got
            out = np.zeros(len(got) + 8, np.uint8)
            assert L.bsc_cpg_reads_stream_read(h, 1, len(got), out.ctypes.data) == -1 and b"beyond" in L.bsc_last_error()
            # what the context keeps beside it is untouched
            assert kept_stream(caller, len(bcf0)) == bcf0
            ent1, r1 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() and r0 == r1 == n_rec
            assert caller.block_meth_kept(name, merge=True) == merge0
            assert caller.block_cpg_reads_kept(name, PAR)[0] == got  # ... and behind the table call
            # the refusals of the arguments leave the block where it is
            for bad_name, bad_par in ((b"a\tb", cp), (name.encode(), _lib.CpgReadsParams(0, 1))):
                assert L.bsc_block_cpg_reads_kept(h, bad_name, C.byref(bad_par), 1 << 20, C.byref(nb), C.byref(nl), None) == -1 and nb.value == 0
            # behind the text encoder's keep call: the same table
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, **kw)
            assert n_txt == n_rec
            assert caller.block_cpg_reads_kept(name, PAR) == (got, lines, tot)
            assert kept_stream(caller, len(text)) == text
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, **kw)
            assert L.bsc_block_cpg_reads_kept(h, name.encode(), C.byref(cp), 1 << 20, C.byref(nb), C.byref(nl), None) == -1
            assert b"no single block" in L.bsc_last_error() and nb.value == 0
            # the caller's own counts: where positions p and p + 1 both have a record, the informative C / T of the C2T templates at p and
            # the informative G / A of the G2A templates at p + 1 are this table's m and u (no template has two counting bytes at a position)
            recs, _ = caller.block_records_raw(raw, seq, ms, x, y, ref, **kw)
            cts = {int(r["core"]["pos"]): r["counts"] for r in recs}
            for s in w_recs:
                p = int(s["pos"])
                if p in cts and p + 1 in cts:
                    assert int(s["m"]) == int(cts[p][5]) + int(cts[p + 1][6]) and int(s["u"]) == int(cts[p][7]) + int(cts[p + 1][4]), (name, p)
                    n_compared += 1
            n_blocks += 1
    assert n_blocks > 4 and n_short >= 1 and n_lines > 200 and n_disc > 10 and n_compared > 100, (n_blocks, n_short, n_lines, n_disc, n_compared)


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
        full, lines, _ = caller.block_cpg_reads_kept(name, PAR)
        assert lines > 0
        p, nb = C.c_void_p(), C.c_uint64()
        assert L.bsc_cpg_reads_stream_detach(h, C.byref(p), C.byref(nb)) == 0 and nb.value == len(full) and p.value
        p2, nb2 = C.c_void_p(), C.c_uint64(9)
        assert L.bsc_cpg_reads_stream_detach(h, C.byref(p2), C.byref(nb2)) == -1 and not p2.value and nb2.value == 0  # once
        z = caller.bgzf()
        z.write_device(p.value, len(full))
        comp = z.take() + z.close()
        assert gzip.decompress(comp) == full and comp.endswith(vcf.BGZF_EOF)
        assert L.bsc_detached_free(h, p) == 0
        assert caller.block_cpg_reads_kept(name, PAR)[0] == full  # the next call takes a buffer again


def test_refused_before_any_block(small):
    with B.SiteCaller() as c:
        nb, nl = C.c_uint64(5), C.c_uint64(5)
        cp = _lib.CpgReadsParams()
        assert c._L.bsc_block_cpg_reads_kept(c._h, b"chr1", C.byref(cp), 1 << 16, C.byref(nb), C.byref(nl), None) == -1
        assert b"no single block" in c._L.bsc_last_error() and (nb.value, nl.value) == (0, 0)


# ---- 4. file to file ------------------------------------------------------------------------------------------------------------------------
def run_exe(*args, env=None, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout
    return r


def file_table(caller, bam, refs, reference, par):
    """The concatenated per-block Python tables of a file, the sums of their totals, and the templates with two counting bytes at a position."""
    out, tot, doubles = [], np.zeros(8, np.int64), 0
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
            x, y = int(blk.x), int(blk.y)
            raw, seq, ms = rd.fetch(blk)
            table, _, t, _, dbl = python_table(name, raw, seq, ms, x, y, block_reference(codes, x, y), par)
            out.append(table)
            tot += np.array(t)
            doubles += dbl
    return b"".join(out), tuple(int(v) for v in tot), doubles


def stdout_line(table, tot):
    return "%d CpG sites in the read-level table, %d lines written (eligible templates %d, discordant %d)\n" % (tot[0], table.count(b"\n"), tot[5], tot[6])


def test_bam2bcf_meth_reads_and_pipeline(caller, small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("f" + s))
    rd = lambda path: open(path, "rb").read()
    want, tot, doubles = file_table(caller, bam, refs, reference, {"min_sites": 4, "min_cov": 1})
    assert doubles == 0 and tot[6] > 10 and want.count(b"\n") > 500
    # plain: the table is the concatenated per-block tables; everything else as without the switch
    base = run_exe("--meth", p(".u.cpg"), "--meth-merge", bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    out = run_exe("--meth-reads", p(".ur.tsv"), "--meth", p(".ur.cpg"), "--meth-merge", bam, fa, p(".ur.bcf"), p(".ur.json"), "S9")
    assert rd(p(".ur.tsv")) == want
    for a, b in ((".ur.bcf", ".u.bcf"), (".ur.json", ".u.json"), (".ur.cpg", ".u.cpg")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    assert out == base + stdout_line(want, tot)
    # every pair line of the merge table joins on (start, end), and m + u there is A + B
    _, recs = cpgreads.read_table(want)
    names = cpgreads.read_table(want)[0]
    table = {(nm, int(r["pos"]) - 1): int(r["m"]) + int(r["u"]) for nm, r in zip(names, recs)}
    n_pairs = 0
    for line in rd(p(".u.cpg")).splitlines():
        f = line.split(b"\t")
        assert int(f[2]) - int(f[1]) == 2
        if f[5] != b".":
            continue  # a single half
        key = (f[0], int(f[1]))
        cov = int(f[9])  # coverage = A + B
        assert key in table and table[key] == cov, (key, cov, table.get(key))
        n_pairs += 1
    assert n_pairs > 100
    # the thresholds
    want_t, tot_t, _ = file_table(caller, bam, refs, reference, {"min_sites": 2, "min_cov": 5})
    out = run_exe("--meth-reads", p(".t.tsv"), "--meth-reads-min-sites", "2", "--meth-reads-min-cov", "5", bam, fa, p(".t.bcf"), p(".t.json"), "S9")
    assert rd(p(".t.tsv")) == want_t and 0 < want_t.count(b"\n") < want.count(b"\n") and out.endswith(stdout_line(want_t, tot_t))
    # -O b --index: the inflated table is the plain one; the main file, its .csi, the report and the merge table are those of the run without
    opts = ["-O", "b", "--index", "--meth", p(".b.cpg.gz"), "--meth-merge"]
    base = run_exe(*opts, bam, fa, p(".b.bcf"), p(".b.json"), "S9")
    opts_r = ["-O", "b", "--index", "--meth", p(".br.cpg.gz"), "--meth-merge", "--meth-reads", p(".br.tsv.gz")]
    out = run_exe(*opts_r, bam, fa, p(".br.bcf"), p(".br.json"), "S9")
    blob = rd(p(".br.tsv.gz"))
    from bs_call_amd import vcf

    assert blob.endswith(vcf.BGZF_EOF) and csi_ref.inflate(blob) == want and out == base + stdout_line(want, tot)
    for a, b in ((".br.bcf", ".b.bcf"), (".br.bcf.csi", ".b.bcf.csi"), (".br.json", ".b.json"), (".br.cpg.gz", ".b.cpg.gz")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    # --meth-bgzf compresses the table of an uncompressed run
    run_exe("--meth-bgzf", "--meth-reads", p(".z.tsv.gz"), bam, fa, p(".z.bcf"), p(".z.json"), "S9")
    assert csi_ref.inflate(rd(p(".z.tsv.gz"))) == want and rd(p(".z.bcf")) == rd(p(".u.bcf"))
    # pipeline.run(cpg_reads_path=...) writes the same file, compressed or not
    for compressed in (False, True):
        out = p(".pipe%d" % compressed)
        s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, compressed=compressed, cpg_reads_path=out + ".tsv",
                         cpg_reads_params={"min_sites": 2, "min_cov": 5})
        got = rd(out + ".tsv")
        got = csi_ref.inflate(got) if compressed else got
        assert got == want_t and s["cpg_reads_lines"] == want_t.count(b"\n") and s["cpg_reads_totals"] == tot_t
    # refused where --meth is: sharded runs, the host paths; no file is left behind
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), cpg_reads_path=p(".no.tsv"))
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, cpg_reads_path=p(".no.tsv"), shard_rank=0, shard_world=2)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, cpg_reads_params={"min_sites": 2})
    for args, env in ((["--rank", "0", "--world", "2"], None), ([], {"BAM2BCF_HOST_READER": "1"}), ([], {"BAM2BCF_HOST_BCF": "1"})):
        r = run_exe(*args, "--meth-reads", p(".no.tsv"), bam, fa, p(".no"), p(".no.json"), env=env, ok=False)
        assert r.returncode == 2 and "--meth-reads" in r.stderr
    for args in (["--meth-reads-min-sites", "3"], ["--meth-reads", p(".no.tsv"), "--meth-reads-min-sites", "0"],
                 ["--meth-reads", p(".no.tsv"), "--meth-reads-min-cov", "x"]):
        r = run_exe(*args, bam, fa, p(".no"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--meth-reads" in r.stderr
    assert not os.path.exists(p(".no.tsv"))
