"""The per-region fragment methylation summary on the device: bsc_frag_attach / _device / _read / _reset and bsc_block_frag_kept
(csrc/fragdev.hip behind the read-level table's site pass) against the host form (csrc/frag.c) and the Python rule (bs_call_amd/frag.py),
accumulator for accumulator and total for total, on the blocks of tests/frag_cases.py; the block entry behind both _keep calls; bam2bcf
--meth-frags and pipeline.run(frag_path=...) file to file against frag.from_pat of the --meth-pat table of the same run."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import epi_cases as E
import frag_cases as F
from bs_call_amd import _lib, frag, methbed, pat, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import frag_regions_host, prepare_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
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


def add_device(caller, b, tpl=None, params=None, expect_refusal=False):
    """bsc_frag_device over a block (or over tpl, a part of its templates) into whatever is attached.  Returns the call's totals after
    checking the guard words around them."""
    assert caller.params["min_qual"] == b["min_qual"]
    tpl = b["tpl"] if tpl is None else tpl
    d_tpl, d_seq, d_ref = dev(tpl), dev(b["seq"]), dev(b["ref"])
    d_tot = torch.full((8 + 2,), FILL, dtype=torch.int64, device="cuda")
    par = b["params"] if params is None else params
    args = (d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), len(b["seq"]), b["x"], b["y"], d_ref.data_ptr(), d_tot.data_ptr() + 8)
    if expect_refusal:
        with pytest.raises(B.BscError):
            caller.frag_device(*args, params=par if isinstance(par, _lib.FragParams) else _lib.FragParams(**par))
        torch.cuda.synchronize()
        assert (d_tot.cpu().numpy() == FILL).all()
        return None
    caller.frag_device(*args, params=par)
    torch.cuda.synchronize()
    out = d_tot.cpu().numpy().view(np.uint64)
    assert int(out[0]) == FILL and int(out[9]) == FILL, "a word beside the totals was written"
    return tuple(int(v) for v in out[1:9])


def check_block(caller, b, python_too=False):
    want, wtot = frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], b["params"])
    assert caller.frag_attach(b["regions"]) == len(b["regions"])
    tot = add_device(caller, b)
    got = caller.frag_read()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.tolist() == want.tolist(), (b["name"], [(b["regions"][i], got[i].tolist(), want[i].tolist()) for i in bad[:3]])
    assert tot == wtot, (b["name"], tot, wtot)
    if python_too:
        p_acc, p_tot = frag.region_frags(b, b["regions"], b["params"])
        assert p_acc.tolist() == got.tolist() and p_tot == tot, b["name"]
    return got, tot


# ---- 1. the accumulators ----------------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_block(caller):
    got, tot = check_block(caller, F.hand_block(), python_too=True)
    assert [tuple(int(v) for v in r) for r in got] == F.HAND_ACC and tot == F.HAND_TOTALS


@pytest.mark.parametrize("b", F.small_blocks()[1:], ids=lambda b: b["name"])
def test_small_blocks(caller, b):
    """Class borders, region edges around sites, tiles and the block's ends, duplicate / nested / staggered regions, 1 .. 129 candidates, a
    whole-block region ahead of 300 short ones, the 5 000-base read, 5 000 templates on one region (tests/frag_cases.py)."""
    got, tot = check_block(caller, b, python_too=len(b["tpl"]) <= 16)
    if b["name"].startswith("contention, one"):
        assert tuple(int(v) for v in got[0]) == (5000, 0, 5000, 0, 20000, 10000, 5000, 0)
    if b["name"].startswith("long read, one"):
        assert int(got[0][0]) == 3 and int(got[0][4]) > 7000  # three fragments of about 2 450 states each


@pytest.mark.parametrize("nr", F.COUNTS)
def test_template_counts(caller, nr):
    check_block(caller, F.count_block(nr))


@pytest.fixture(scope="module")
def big():
    b = F.big_block()
    return b, frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], b["params"])


def test_20003_positions(caller, big):
    b, (want, wtot) = big
    got, tot = check_block(caller, b)
    assert wtot[1] > 1000 and int((got[:, 0] > 0).sum()) > 500
    # two calls over two halves of the templates == one call; reset; a second attach zeroes; detach
    caller.frag_reset()
    assert not caller.frag_read().any()
    half = len(b["tpl"]) // 2
    t1 = add_device(caller, b, tpl=b["tpl"][:half])
    t2 = add_device(caller, b, tpl=b["tpl"][half:])
    assert caller.frag_read().tolist() == want.tolist() and tuple(u + v for u, v in zip(t1, t2)) == wtot
    add_device(caller, b)
    assert caller.frag_read().tolist() == (2 * want).tolist()  # the accumulators add over calls
    assert add_device(caller, b, tpl=b["tpl"][:0]) == (0,) * 8  # no template: legal, adds nothing
    assert caller.frag_read().tolist() == (2 * want).tolist()
    hand = F.hand_block()
    caller.frag_attach(hand["regions"])
    assert caller.frag_read().shape == (5, 8) and not caller.frag_read().any()
    caller.frag_attach([])
    assert caller.frag_read().shape == (0, 8)
    add_device(caller, hand, expect_refusal=True)  # nothing attached


def test_20003_positions_on_a_one_cu_grid(one_cu, big):
    b, (want, wtot) = big
    got, tot = check_block(one_cu, b)
    assert got.tolist() == want.tolist() and tot == wtot


def set_long_bases(c, bases):
    """bsc_frag_long_bases_set: a test-only entry that is not in the header — the bound the NEXT attach takes (0: the default)."""
    fn = c._L.bsc_frag_long_bases_set
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_uint32]
    assert fn(c._h, bases) == 0


def test_long_regions_go_through_the_separate_list(big):
    """With a bound of 100 bases most of the 1 000 random intervals and the whole-block region are long and go through the list every
    template tests; the sums are the same."""
    b, (want, wtot) = big
    with B.SiteCaller() as c:
        set_long_bases(c, 100)
        got, tot = check_block(c, b)
        assert got.tolist() == want.tolist() and tot == wtot
        check_block(c, F.first_long_block())
        check_block(c, F.long_read_blocks()[2])
        set_long_bases(c, 0)
        check_block(c, F.first_long_block())


@pytest.mark.parametrize("side", [False, True], ids=["the default stream", "a side stream"])
def test_read_and_reset_wait_for_the_caller_s_stream(caller, big, side):
    """bsc_frag_read and bsc_frag_reset wait for the stream of the last accumulating call themselves — the NULL stream as any other (the
    context's own stream is non-blocking and does not order against it): no synchronize between the calls and the read."""
    b, (want, _) = big
    d_tpl, d_seq, d_ref = dev(b["tpl"]), dev(b["seq"]), dev(b["ref"])
    d_tot = torch.zeros(8, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream() if side else None
    handle = st.cuda_stream if side else None
    caller.frag_attach(b["regions"])
    torch.cuda.synchronize()
    args = (d_tpl.data_ptr(), len(b["tpl"]), d_seq.data_ptr(), len(b["seq"]), b["x"], b["y"], d_ref.data_ptr(), d_tot.data_ptr())
    n = 6
    for _ in range(n):
        caller.frag_device(*args, params=b["params"], stream=handle)
    got = caller.frag_read()  # (no torch.cuda.synchronize() in front of it)
    assert got.tolist() == (n * want).tolist()
    for _ in range(n):
        caller.frag_device(*args, params=b["params"], stream=handle)
    caller.frag_reset()  # zeroes behind the last add, not among them
    assert not caller.frag_read().any()
    caller.frag_device(*args, params=b["params"], stream=handle)
    assert caller.frag_read().tolist() == want.tolist()
    torch.cuda.synchronize()
    caller.frag_attach([])


def test_the_refusals_write_nothing(caller):
    b = F.hand_block()
    want, _ = frag_regions_host(b["tpl"], b["seq"], b["x"], b["y"], b["ref"], b["regions"], b["min_qual"], b["params"])
    caller.frag_attach(b["regions"])
    add_device(caller, b)
    for bad in ({"min_sites": 0}, {"u_max_pct": 101, "m_min_pct": 102}, {"m_min_pct": 101}, {"u_max_pct": 75}, {"reserved": 1}):
        add_device(caller, b, params=dict(F.PAR, **bad), expect_refusal=True)
    add_device(caller, dict(b, x=b["y"], y=b["x"]), expect_refusal=True)  # y < x
    assert caller.frag_read().tolist() == want.tolist()  # the accumulators are as they were
    # attach: unsorted, start > end, and the previous attachment stays
    for regs in ([(10, 20), (5, 30)], [(10, 20), (10, 15)], [(30, 20)]):
        with pytest.raises(B.BscError):
            caller.frag_attach(regs)
    assert caller.frag_read().tolist() == want.tolist()
    # the read path's bound: guard words in front of and behind the host buffer's n x 8 words; a count that is not the attached one writes nothing
    buf = np.full(8 + 5 * 8 + 8, FILL, np.uint64)
    for n_bad in (4, 6, 0):
        assert caller._L.bsc_frag_read(caller._h, buf[8:].ctypes.data, n_bad) == -1 and (buf == FILL).all()  # five are attached
    assert caller._L.bsc_frag_read(caller._h, buf[8:].ctypes.data, 5) == 0
    assert (buf[:8] == FILL).all() and (buf[48:] == FILL).all(), "a word beside the accumulators was written"
    assert buf[8:48].reshape(5, 8).tolist() == want.tolist()
    # the region summary's accumulators are another set
    assert caller.meth_regions_read().shape[0] != 5 or not caller.meth_regions_read().any()
    caller.frag_attach([])


# ---- 2. the block entry -----------------------------------------------------------------------------------------------------------------------
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
    """The fixture tests/test_gpu_epi.py uses: chrA, 6 000 positions at ~40x; chrT, 60 positions of CG A T CG ...; chrG, 30 000 positions in
    several blocks — and a BED file over them."""
    d = tmp_path_factory.mktemp("frag_files")
    rng = np.random.default_rng(4714)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50, err=0.0)
            + W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    rows = [("chrG", 0, 30_000, "whole"), ("chrA", 0, 6_000, None), ("chrT", 0, 60, "tiny"), ("chrT", 10, 40, None), ("chrZ", 5, 50, "absent")]
    rows += [("chrA", int(s), int(s + n), "a%d" % i) for i, (s, n) in enumerate(zip(rng.integers(0, 5_900, 80), rng.integers(1, 600, 80)))]
    rows += [("chrG", int(s), int(s + n), None) for s, n in zip(rng.integers(0, 29_900, 150), rng.integers(1, 600, 150))]
    bed = str(d / "r.bed")
    with open(bed, "w") as f:
        for r in rows:
            f.write("\t".join(str(v) for v in r[: 4 if r[3] else 3]) + "\n")
    return d, bam, fa, refs, reference, bed


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference, bed = small
    L, h = caller._L, caller._h
    sets = methbed.read_regions(bed)
    n_blocks = n_frags = 0
    cur = None
    par = {"min_sites": 2}
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            raw, seq, ms = rd.fetch(blk)
            tpl, pseq, _ = prepare_templates(raw, seq, ms)
            regs = sets[name][0]
            if name != cur:
                cur = name
                assert caller.frag_attach(regs) == len(regs)
                caller.meth_regions_attach(regs)
                want = np.zeros((len(regs), 8), np.uint64)
            p_acc, p_tot = frag.region_frags(dict(tpl=tpl, seq=pseq, x=x, y=y, ref=ref, min_qual=20), regs, par)
            want = want + p_acc
            kw = dict(reg_stop=len(codes))
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, keep=True, **kw)
            ent0, r0 = caller.block_csi_kept(14)
            merge0 = caller.block_meth_kept(name, merge=True)
            reads0 = caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1})
            epi0 = caller.block_epi_kept(name, {"min_cov": 2})
            caller.block_meth_regions_kept()
            mr0 = caller.meth_regions_read()
            assert caller.block_frag_kept(par) == p_tot, (name, x)
            assert caller.frag_read().tolist() == want.tolist(), (name, x)
            n_frags += p_tot[1]
            # what the context keeps beside it is untouched
            assert kept_stream(caller, len(bcf0)) == bcf0
            ent1, r1 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() and r0 == r1 == n_rec
            assert caller.block_meth_kept(name, merge=True) == merge0
            assert caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1}) == reads0
            assert caller.block_epi_kept(name, {"min_cov": 2}) == epi0
            assert caller.meth_regions_read().tobytes() == mr0.tobytes()
            # the refusals of the arguments leave the accumulators where they are
            t8 = (C.c_uint64 * 8)(*([5] * 8))
            assert L.bsc_block_frag_kept(h, C.byref(_lib.FragParams(0)), t8) == -1 and list(t8) == [0] * 8
            assert L.bsc_block_frag_kept(h, C.byref(_lib.FragParams(3, 80, 75)), None) == -1
            assert caller.frag_read().tolist() == want.tolist()
            # behind the text encoder's keep call: the same sums once more
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, **kw)
            assert n_txt == n_rec
            assert caller.block_frag_kept(par) == p_tot
            want = want + p_acc
            assert caller.frag_read().tolist() == want.tolist() and kept_stream(caller, len(text)) == text
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, **kw)
            assert L.bsc_block_frag_kept(h, C.byref(_lib.FragParams()), t8) == -1 and b"no single block" in L.bsc_last_error()
            n_blocks += 1
    caller.frag_attach([])
    caller.meth_regions_attach([])
    assert n_blocks > 4 and n_frags > 1000, (n_blocks, n_frags)


def test_refused_before_any_block_and_with_nothing_attached():
    with B.SiteCaller() as c:
        t8 = (C.c_uint64 * 8)(*([5] * 8))
        assert c._L.bsc_block_frag_kept(c._h, C.byref(_lib.FragParams()), t8) == -1
        assert b"no single block" in c._L.bsc_last_error() and list(t8) == [0] * 8
        assert c.frag_read().shape == (0, 8)
        c.frag_reset()


# ---- 3. file to file --------------------------------------------------------------------------------------------------------------------------
def run_exe(*args, env=None, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout
    return r


def table_from_pat(pat_file, refs, reference, sets, params, window=None):
    """frag.from_pat over the --meth-pat table of a run, contig by contig in the header's order: the lines --meth-frags should write."""
    lines = pat.read_pat(open(pat_file, "rb").read())
    out = []
    for name, length in refs:
        if window is not None:
            regs, names = methbed.window_regions(length, window), None
        elif name in sets:
            regs, names = sets[name]
        else:
            continue
        own = [ln for ln in lines if ln[0] == name.encode()]
        if not own:
            continue  # no block of this contig: nothing is attached, no line
        codes = reference[name]
        sp = [i + 1 for i in range(len(codes) - 1) if codes[i] == 2 and codes[i + 1] == 3]
        acc, _ = frag.from_pat(own, sp, regs, params)
        out.append(frag.format_regions(name, regs, names, acc))
    return b"".join(out)


def test_bam2bcf_meth_frags_and_pipeline(caller, small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference, bed = small
    p = lambda s: str(d / ("f" + s))
    rd = lambda path: open(path, "rb").read()
    sets = methbed.read_regions(bed)
    # --meth-regions with --meth-frags and --meth-pat: the summary is from_pat of the pattern table; everything else as without the switch
    base = run_exe("--meth-regions", bed, "--meth-regions-out", p(".u.reg"), "--meth-pat", p(".u.pat"), bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    out = run_exe("--meth-regions", bed, "--meth-regions-out", p(".f.reg"), "--meth-frags", p(".f.tsv"), "--meth-pat", p(".f.pat"), bam, fa, p(".f.bcf"),
                  p(".f.json"), "S9")
    want = table_from_pat(p(".f.pat"), refs, reference, sets, None)
    got = rd(p(".f.tsv"))
    assert got == want and want.count(b"\n") > 200
    rows = frag.read_table(got)
    assert int(rows["frags"].sum()) > 1000 and int(rows["U"].sum()) > 0 and int(rows["M"].sum()) > 0 and int(rows["X"].sum()) > 0
    for a, b in ((".f.bcf", ".u.bcf"), (".f.json", ".u.json"), (".f.reg", ".u.reg"), (".f.pat", ".u.pat")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    more = [ln for ln in out.splitlines() if ln not in base.splitlines()]  # stdout gets one more line
    assert len(out.splitlines()) == len(base.splitlines()) + 1 and len(more) == 1, more
    assert more[0].startswith("%d fragment summary lines written (templates with a CpG state " % want.count(b"\n"))
    assert "fragments in regions %d: " % int(rows["frags"].sum()) in more[0]
    # the lines join the region summary's on the first four columns
    assert [ln.split(b"\t")[:4] for ln in got.splitlines()] == [ln.split(b"\t")[:4] for ln in rd(p(".f.reg")).splitlines()]
    # without --meth-regions-out, and the thresholds
    run_exe("--meth-regions", bed, "--meth-frags", p(".o.tsv"), bam, fa, p(".o.bcf"), p(".o.json"), "S9")
    assert rd(p(".o.tsv")) == want and rd(p(".o.bcf")) == rd(p(".u.bcf")) and rd(p(".o.json")) == rd(p(".u.json"))
    par = {"min_sites": 1, "u_max_pct": 10, "m_min_pct": 60}
    run_exe("--meth-regions", bed, "--meth-frags", p(".t.tsv"), "--meth-frags-min-sites", "1", "--meth-frags-u-max", "10", "--meth-frags-m-min", "60", bam, fa,
            p(".t.bcf"), p(".t.json"), "S9")
    assert rd(p(".t.tsv")) == table_from_pat(p(".f.pat"), refs, reference, sets, par) != want
    # --meth-window 1000
    run_exe("--meth-window", "1000", "--meth-regions-out", p(".w.reg"), "--meth-frags", p(".w.tsv"), bam, fa, p(".w.bcf"), p(".w.json"), "S9")
    want_w = table_from_pat(p(".f.pat"), refs, reference, sets, None, window=1000)
    assert rd(p(".w.tsv")) == want_w and want_w.count(b"\n") == 6 + 1 + 30 and rd(p(".w.bcf")) == rd(p(".u.bcf"))
    # pipeline.run gives the same table
    s = pipeline.run(bam, reference, p(".pipe"), sample="S9", benchmark_mode=True, device_reader=True, meth_regions=bed, frag_path=p(".pipe.tsv"))
    assert rd(p(".pipe.tsv")) == want and s["frag_lines"] == want.count(b"\n") and s["frag_totals"][1] == int(rows["frags"].sum())
    s = pipeline.run(bam, reference, p(".pipew"), sample="S9", benchmark_mode=True, device_reader=True, meth_window=1000, meth_regions_path=p(".pipew.reg"),
                     frag_path=p(".pipew.tsv"), frag_params=par)
    assert rd(p(".pipew.tsv")) == table_from_pat(p(".f.pat"), refs, reference, sets, par, window=1000) and rd(p(".pipew.reg")) == rd(p(".w.reg"))
    # the refusals; no file is left behind
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, frag_path=p(".no.tsv"))  # no intervals
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), meth_regions=bed, frag_path=p(".no.tsv"))  # not the device reader
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, meth_regions=bed, meth_regions_path=p(".no.reg"), frag_params=par)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, meth_regions=bed, frag_path=p(".no.tsv"), frag_params={"u_max_pct": 80})
    for args, env in ((["--rank", "0", "--world", "2"], None), ([], {"BAM2BCF_HOST_READER": "1"}), ([], {"BAM2BCF_HOST_BCF": "1"}), ([], {"BAM2BCF_HOST_PREP": "1"})):
        r = run_exe(*args, "--meth-regions", bed, "--meth-frags", p(".no.tsv"), bam, fa, p(".no"), p(".no.json"), env=env, ok=False)
        assert r.returncode == 2 and "--meth-frags" in r.stderr
    for args in (["--meth-frags", p(".no.tsv")], ["--meth-regions", bed, "--meth-regions-out", p(".no.reg"), "--meth-frags-min-sites", "3"],
                 ["--meth-regions", bed, "--meth-frags", p(".no.tsv"), "--meth-frags-min-sites", "0"],
                 ["--meth-regions", bed, "--meth-frags", p(".no.tsv"), "--meth-frags-u-max", "x"],
                 ["--meth-regions", bed, "--meth-frags", p(".no.tsv"), "--meth-frags-u-max", "80"],
                 ["--meth-regions", bed, "--meth-frags", p(".no.tsv"), "--meth-frags-m-min", "101"]):
        r = run_exe(*args, bam, fa, p(".no"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--meth-frags" in r.stderr, args
    assert not os.path.exists(p(".no.tsv"))
    r = run_exe("--meth-regions", bed, bam, fa, p(".no"), p(".no.json"), ok=False)  # as before the switch existed
    assert r.returncode == 2 and "--meth-regions-out" in r.stderr
