"""The M-bias table on the device (csrc/mbiasdev.hip) — the rule of include/bscall_amd.h (READ, END, CYCLE, G(j), COUNTS, CONTEXT, TABLE, TOTALS,
LINE):

  1. bsc_mbias_device against the host form (csrc/mbias.c) and the Python rule (bs_call_amd/mbias.py), cell for cell and total for total, on
     the blocks of tests/mbias_cases.py: template counts around a workgroup's eight waves, 20 003 templates on the default and on a one-CU
     grid, read lengths around a round of 64 bytes, reads of 1 025 and 5 000 bytes, every hand-made case in one block, contention, every
     n_cycles, guard bytes, the refusal, two halves == the whole, twice the same bytes
  2. bsc_block_mbias_rawdev behind both _keep calls on a device reader's blocks of a fixture with soft clips and indels, against the Python
     rule over the reader's host copy of the same raw block; accumulation, reset, n_cycles changed; what the context keeps is untouched
  3. bam2bcf --mbias and pipeline.run(mbias_path=) file to file"""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import mbias_cases as K
from bs_call_amd import _lib, mbias, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import mbias_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
PAD = 0x7777777777777777
GUARD = 16  # u64 of guard behind the table and behind the totals


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
    t = torch.from_numpy(a.copy() if a.size else np.zeros(16, np.uint8)).to("cuda")
    torch.cuda.synchronize()
    return t


class Device:
    """A block's arrays on the device and a zeroed table + totals with guard words behind each."""

    def __init__(self, b, n_cycles):
        self.b, self.n_cycles, self.cells = b, n_cycles, 12 * max(1, min(n_cycles, 1024)) * 2
        self.d_raw, self.d_seq, self.d_misms, self.d_ref = dev(b["raw"]), dev(b["seq"]), dev(b["misms"]), dev(b["ref"])
        self.d_counts = torch.full((self.cells + GUARD,), PAD, dtype=torch.int64, device="cuda")
        self.d_tot = torch.full((8 + GUARD,), PAD, dtype=torch.int64, device="cuda")
        self.zero()

    def zero(self):
        self.d_counts[: self.cells] = 0
        self.d_tot[:8] = 0
        torch.cuda.synchronize()

    def run(self, caller, first=0, n=None, params=None):
        b = self.b
        assert caller.params["min_qual"] == b["min_qual"]
        n = len(b["raw"]) - first if n is None else n
        caller.mbias_device(self.d_raw.data_ptr() + 72 * first, n, self.d_seq.data_ptr(), len(b["seq"]), self.d_misms.data_ptr(), len(b["misms"]), b["x"], b["y"],
                            self.d_ref.data_ptr(), self.d_counts.data_ptr(), self.d_tot.data_ptr(), params=self.n_cycles if params is None else params)
        torch.cuda.synchronize()

    def read(self):
        c, t = self.d_counts.cpu().numpy(), self.d_tot.cpu().numpy()
        assert (c[self.cells :] == PAD).all() and (t[8:] == PAD).all(), "words behind the table or the totals were written"
        return c[: self.cells].view(np.uint64).reshape(2, 2, 3, -1, 2).copy(), tuple(int(v) for v in t[:8].view(np.uint64))


def check_block(caller, b, n_cycles=512, python_too=True):
    want, wtot = mbias_host(b["raw"], b["seq"], b["misms"], b["x"], b["y"], b["ref"], b["min_qual"], n_cycles)
    d = Device(b, n_cycles)
    d.run(caller)
    got, tot = d.read()
    assert tot == tuple(int(v) for v in wtot), (b["name"], n_cycles, tot, wtot)
    assert got.tobytes() == want.tobytes(), (b["name"], n_cycles, np.argwhere(got != want)[:4])
    if python_too:
        p, ptot = mbias.table(b["raw"], b["seq"], b["misms"], b["x"], b["y"], b["ref"], b["min_qual"], n_cycles)
        assert p.tobytes() == got.tobytes() and tuple(int(v) for v in ptot) == tot, b["name"]
    return d, got, tot


# ---- 1. the walk --------------------------------------------------------------------------------------------------------------------------------
def test_the_hand_worked_block(caller):
    _, got, tot = check_block(caller, K.hand_worked(), 8)
    assert tot == K.HAND_TOTALS and {tuple(i) for i in np.argwhere(got)} == set(K.HAND_CELLS)


@pytest.fixture(scope="module")
def big():
    return K.random_block(41, 4113, n_pos=3000)


@pytest.mark.parametrize("nr", [0, 1, 63, 64, 65, 4113])
def test_template_counts(caller, big, nr):
    b = dict(big, raw=big["raw"][:nr], name="first %d" % nr)
    _, _, tot = check_block(caller, b)
    assert (tot[0] > nr // 2 and tot[6] > 0) or nr < 63


@pytest.fixture(scope="module")
def huge():
    b = K.random_block(43, 1000, n_pos=4000, max_len=150)
    # 20 003 templates over the reads and lists of 1 000: every template's bytes are real, the buffers stay small
    idx = np.random.default_rng(7).integers(0, 1000, 20_003)
    b = dict(b, raw=b["raw"][idx], name="20 003 templates")
    want = mbias_host(b["raw"], b["seq"], b["misms"], b["x"], b["y"], b["ref"], b["min_qual"], 512)
    return b, want


def test_20003_templates(caller, huge):
    b, (want, wtot) = huge
    d = Device(b, 512)
    d.run(caller)
    got, tot = d.read()
    assert tot == tuple(int(v) for v in wtot) and got.tobytes() == want.tobytes() and tot[2] > 200_000
    # the same call twice into zeroed tables: the same bytes
    d.zero()
    d.run(caller)
    assert d.read()[0].tobytes() == got.tobytes()
    # two calls on two halves of the templates == one call on all of them
    d.zero()
    d.run(caller, 0, 9_999)
    d.run(caller, 9_999, 20_003 - 9_999)
    got2, tot2 = d.read()
    assert got2.tobytes() == got.tobytes() and tot2 == tot


def test_20003_templates_on_a_one_cu_grid(one_cu, huge):
    b, (want, wtot) = huge
    d = Device(b, 512)
    d.run(one_cu)
    got, tot = d.read()
    assert tot == tuple(int(v) for v in wtot) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("n_cycles", [1, 64, 512, 1024])
def test_every_hand_made_case_in_one_block(caller, n_cycles):
    b = K.merge("all targeted", K.targeted())
    _, _, tot = check_block(caller, b, n_cycles)
    assert tot[6] == 15 + 28 and tot[2] + tot[3] > 300 and tot[2] > 0


@pytest.mark.parametrize("n_cycles", [1, 64, 512, 1024])
def test_read_lengths_and_long_reads(caller, n_cycles):
    check_block(caller, K.lengths_block(), n_cycles)
    _, got, tot = check_block(caller, K.long_reads(), n_cycles)
    assert tot[3] > 0 and tot[0] == 8
    if n_cycles == 1024:
        assert got[:, :, :, 256:].sum() > 400  # the cells beyond the LDS table's cycles


def test_contention(caller):
    _, got, tot = check_block(caller, K.contention(5000), 64, python_too=False)
    assert tot == (5000, 5000 * 64, 5000 * 32, 0, 5000 * 32, 0, 0, 0) and (got[0, 0, 0, 0:64:2, 0] == 5000).all() and got.sum() == 5000 * 32


def test_the_refusal_writes_nothing(caller):
    b = K.hand_worked()
    for n in (0, 1025):
        d = Device(b, 8)
        d.d_counts[:] = PAD
        d.d_tot[:] = PAD
        with pytest.raises(B.BscError):
            d.run(caller, params=_lib.MbiasParams(n))
        torch.cuda.synchronize()
        assert (d.d_counts.cpu().numpy() == PAD).all() and (d.d_tot.cpu().numpy() == PAD).all()
    d = Device(b, 8)
    with pytest.raises(B.BscError):  # y < x
        caller.mbias_device(d.d_raw.data_ptr(), 3, d.d_seq.data_ptr(), len(b["seq"]), d.d_misms.data_ptr(), len(b["misms"]), b["y"] + 1, b["y"], d.d_ref.data_ptr(),
                            d.d_counts.data_ptr(), d.d_tot.data_ptr(), params=8)
    with pytest.raises(B.BscError):  # a table that is not 8-byte aligned
        caller.mbias_device(d.d_raw.data_ptr(), 3, d.d_seq.data_ptr(), len(b["seq"]), d.d_misms.data_ptr(), len(b["misms"]), b["x"], b["y"], d.d_ref.data_ptr(),
                            d.d_counts.data_ptr() + 4, d.d_tot.data_ptr(), params=8)
    assert d.read()[1] == (0,) * 8


# ---- 2. the block entry -------------------------------------------------------------------------------------------------------------------------
def clipped_records(rng, ref_codes, tid, n_pairs, **kw):
    """tools/make_bam.py's pairs with soft clips and indels put into their CIGARs: a right clip, a CIGAR I, a CIGAR D, two indels (the
    record's position stays), and a left clip (the record moves right by the clip, its mate's mpos with it)."""
    recs = W.wgbs_records(rng, ref_codes, tid, n_pairs, **kw)
    by_name = {}
    for r in recs:
        by_name.setdefault(r["name"], []).append(r)
    for i, r in enumerate(recs):
        n = len(r["seq"])
        kind = i % 7
        if kind == 1:
            r["cigar"] = [("M", n - 5), ("S", 5)]
        elif kind == 2:
            r["cigar"] = [("M", 40), ("I", 2), ("M", n - 42)]
        elif kind == 3:
            r["cigar"] = [("M", 30), ("D", 3), ("M", n - 30)]
        elif kind == 4:
            r["cigar"] = [("S", 3), ("M", 20), ("D", 1), ("M", 20), ("I", 4), ("M", n - 51), ("S", 4)]
            r["pos"] += 3
            for m in by_name[r["name"]]:
                if m is not r:
                    m["mpos"] = r["pos"]
        elif kind == 5:
            r["cigar"] = [("S", 6), ("M", n - 6)]
            r["pos"] += 6
            for m in by_name[r["name"]]:
                if m is not r:
                    m["mpos"] = r["pos"]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs


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
    """A BAM of three contigs whose reads carry soft clips and indels: chrA, 6 000 positions at ~30x; chrT, 60 positions (a block shorter than a
    tile); chrG, 30 000 positions in several blocks with gaps between the reads."""
    d = tmp_path_factory.mktemp("mbias_files")
    rng = np.random.default_rng(4717)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (clipped_records(rng, reference["chrA"], 0, 900, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50, err=0.0)
            + clipped_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


def rawdev(caller, blk, params=None):
    return caller.block_mbias_rawdev(blk.d_tpl, blk.nr, blk.d_seq, blk.seq_bytes, blk.d_misms, blk.n_misms, params)


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    caller.mbias_reset()
    with pytest.raises(B.BscError):
        caller.mbias_read(64)  # no accumulator yet
    acc, atot = mbias.empty(256)
    n_blocks = n_clip = n_indel = n_region_sites = 0
    cur = None
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            if name != cur:  # the contig's regions: the whole contig and tiles of 100 bases
                cur = name
                caller.meth_regions_attach(sorted([(0, len(codes))] + [(s, min(s + 100, len(codes))) for s in range(0, len(codes), 100)]))
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            raw, seq, ms = rd.fetch(blk)
            n_clip += int((ms["type"] == 3).sum())
            n_indel += int(((ms["type"] == 1) | (ms["type"] == 2)).sum())
            one, one_tot = mbias.table(raw, seq, ms, x, y, ref, 20, 256)
            kw = dict(reg_stop=len(codes))
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, keep=True, **kw)
            ent0, r0 = caller.block_csi_kept(14)
            meth0 = caller.block_meth_kept(name)
            merge0 = caller.block_meth_kept(name, merge=True)
            reads0 = caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1})
            asm0 = caller.block_asm_kept(name)
            caller.meth_regions_reset()
            sums0 = caller.block_meth_regions_kept({})
            reg0 = caller.meth_regions_read().copy()
            n_region_sites += int(reg0[:, 0].max())  # (only to show that the sums compared below are not empty)
            # a table of this block alone, then the run's accumulator
            caller.mbias_reset()
            tot = rawdev(caller, blk, 256)
            assert caller.meth_regions_read().tobytes() == reg0.tobytes()  # the region sums as they were
            got, tot2 = caller.mbias_read(256)
            assert got.tobytes() == one.tobytes() and tot == tot2 == tuple(int(v) for v in one_tot), (name, x)
            assert one_tot[6] == 0 and one_tot[0] > 0
            # a different n_cycles without a reset is refused and changes nothing; the refusal of the parameters too
            for bad in (64, 0, 1025):
                with pytest.raises(B.BscError):
                    rawdev(caller, blk, _lib.MbiasParams(bad))
            assert caller.mbias_read(256)[0].tobytes() == one.tobytes()
            # adding: the same block again doubles it
            rawdev(caller, blk, 256)
            got, tot2 = caller.mbias_read(256)
            assert (got == 2 * one).all() and tot2 == tuple(2 * int(v) for v in one_tot)
            # what the context keeps beside it is untouched
            assert kept_stream(caller, len(bcf0)) == bcf0
            ent1, r1 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() and r0 == r1 == n_rec
            assert caller.block_meth_kept(name) == meth0 and caller.block_meth_kept(name, merge=True) == merge0
            assert caller.block_cpg_reads_kept(name, {"min_sites": 3, "min_cov": 1}) == reads0 and caller.block_asm_kept(name) == asm0
            assert caller.meth_regions_read().tobytes() == reg0.tobytes()
            caller.meth_regions_reset()
            assert caller.block_meth_regions_kept({}) == sums0 and caller.meth_regions_read().tobytes() == reg0.tobytes()  # ... and behind the call
            # behind the text encoder's keep call: the same table
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, **kw)
            caller.mbias_reset()
            tot = rawdev(caller, blk, 256)
            assert caller.mbias_read(256)[0].tobytes() == one.tobytes() and kept_stream(caller, len(text)) == text
            # refused behind a call that kept nothing, with the accumulator unchanged
            caller.block_bcf_rawdev(blk, ref, tid, **kw)
            with pytest.raises(B.BscError) as e:
                rawdev(caller, blk, 256)
            assert "no single block" in str(e.value)
            assert caller.mbias_read(256)[0].tobytes() == one.tobytes()
            mbias.add_block(acc, atot, raw, seq, ms, x, y, ref, 20)
            n_blocks += 1
    caller.meth_regions_attach([])
    assert n_blocks > 4 and n_clip > 100 and n_indel > 100 and atot[2] > 10_000 and n_region_sites > 100, (n_blocks, n_clip, n_indel, atot, n_region_sites)
    # accumulation over every block of the file, in a second pass with one accumulator
    caller.mbias_reset()
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            codes = reference[refs[tid][0]]
            ref = block_reference(codes, int(blk.x), int(blk.y))
            caller.block_bcf_rawdev(blk, ref, tid, keep=True, reg_stop=len(codes))
            tot = rawdev(caller, blk, 256)
    got, tot2 = caller.mbias_read(256)
    assert got.tobytes() == acc.tobytes() and tot == tot2 == tuple(int(v) for v in atot)
    assert caller.mbias_read()[0].tobytes() == acc.tobytes()  # without a size: the accumulator's own
    with pytest.raises(ValueError):
        caller.mbias_read(64)
    # an accumulator larger than the default: read() sizes its array by the accumulator, not by the caller's belief
    caller.mbias_reset()
    with DeviceBamReader(caller, bam, threads=2) as rd:
        blk = next(iter(rd.device_blocks()))
        codes = reference[refs[int(blk.tid)][0]]
        x, y = int(blk.x), int(blk.y)
        ref = block_reference(codes, x, y)
        raw, seq, ms = rd.fetch(blk)
        caller.block_bcf_rawdev(blk, ref, int(blk.tid), keep=True, reg_stop=len(codes))
        rawdev(caller, blk, 1024)
        got, tot = caller.mbias_read()
        want, wtot = mbias.table(raw, seq, ms, x, y, ref, 20, 1024)
        assert got.shape == (2, 2, 3, 1024, 2) and got.tobytes() == want.tobytes() and tot == tuple(int(v) for v in wtot)
    caller.mbias_reset()
    caller.mbias_reset()  # twice is fine


def test_refused_before_any_block():
    with B.SiteCaller() as c:
        t8 = (C.c_uint64 * 8)()
        mp = _lib.MbiasParams(64)
        assert c._L.bsc_block_mbias_rawdev(c._h, None, 0, None, 0, None, 0, C.byref(mp), t8) == -1
        assert b"no single block" in c._L.bsc_last_error()
        assert c._L.bsc_mbias_read(c._h, None, t8) == -1 and c._L.bsc_mbias_reset(c._h) == 0


# ---- 3. file to file ----------------------------------------------------------------------------------------------------------------------------
def run_exe(*args, env=None, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout
    return r


def file_table(caller, bam, refs, reference, n_cycles):
    acc, tot = mbias.empty(n_cycles)
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            codes = reference[refs[int(blk.tid)][0]]
            x, y = int(blk.x), int(blk.y)
            raw, seq, ms = rd.fetch(blk)
            mbias.add_block(acc, tot, raw, seq, ms, x, y, block_reference(codes, x, y), 20)
    return mbias.format_table(acc), tuple(int(v) for v in tot)


def stdout_line(tot):
    return "M-bias table: %d reads walked, %d bytes mapped, %d counted, %d beyond the table, CpG %d meth %d unmeth, %d reads skipped\n" % tot[:7]


def test_bam2bcf_mbias_and_pipeline(caller, small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("f" + s))
    rd = lambda path: open(path, "rb").read()
    want, tot = file_table(caller, bam, refs, reference, 512)
    assert want.count(b"\n") > 1000 and tot[2] > 10_000 and tot[3] == 0
    base = run_exe("--meth", p(".u.cpg"), "--meth-window", "500", "--meth-regions-out", p(".u.reg"), bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    out = run_exe("--mbias", p(".m.tsv"), "--meth", p(".m.cpg"), "--meth-window", "500", "--meth-regions-out", p(".m.reg"), bam, fa, p(".m.bcf"), p(".m.json"),
                  "S9")
    assert rd(p(".m.tsv")) == want and rd(p(".u.reg")).count(b"\n") > 50
    for a, b in ((".m.bcf", ".u.bcf"), (".m.json", ".u.json"), (".m.cpg", ".u.cpg"), (".m.reg", ".u.reg")):
        assert rd(p(a)) == rd(p(b)), (a, b)
    assert out == base + stdout_line(tot)
    assert mbias.read_table(want).tobytes() == mbias.read_table(p(".m.tsv")).tobytes()
    # --mbias-cycles: a table of 40 cycles, the rest in the overflow total; -O b and the text format beside it
    want40, tot40 = file_table(caller, bam, refs, reference, 40)
    base = run_exe("-O", "b", "--format", "vcf", bam, fa, p(".bv.vcf.gz"), p(".bv.json"), "S9")
    out = run_exe("-O", "b", "--format", "vcf", "--mbias", p(".c.tsv"), "--mbias-cycles", "40", bam, fa, p(".c.vcf.gz"), p(".c.json"), "S9")
    assert rd(p(".c.tsv")) == want40 and tot40[3] > 0 and out == base + stdout_line(tot40) and rd(p(".c.vcf.gz")) == rd(p(".bv.vcf.gz"))
    # pipeline.run(mbias_path=...) writes the same file
    out = p(".pipe")
    s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, mbias_path=out + ".tsv", mbias_params={"n_cycles": 40})
    assert rd(out + ".tsv") == want40 and s["mbias_totals"] == tot40
    # refused where --meth-regions is: sharded runs, the host paths; bad values
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), mbias_path=p(".no.tsv"))
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, mbias_path=p(".no.tsv"), shard_rank=0, shard_world=2)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, mbias_params={"n_cycles": 40})
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, mbias_path=p(".no.tsv"), mbias_params={"n_cycles": 1025})
    for args, env in ((["--rank", "0", "--world", "2"], None), (["--merge", "2"], None), ([], {"BAM2BCF_HOST_READER": "1"}), ([], {"BAM2BCF_HOST_PREP": "1"}),
                      ([], {"BAM2BCF_HOST_BCF": "1"})):
        r = run_exe(*args, "--mbias", p(".no.tsv"), bam, fa, p(".no"), p(".no.json"), env=env, ok=False)
        assert r.returncode == 2 and "--mbias" in r.stderr
    for args in (["--mbias-cycles", "40"], ["--mbias", p(".no.tsv"), "--mbias-cycles", "0"], ["--mbias", p(".no.tsv"), "--mbias-cycles", "1025"],
                 ["--mbias", p(".no.tsv"), "--mbias-cycles", "x"]):
        r = run_exe(*args, bam, fa, p(".no"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--mbias" in r.stderr
    assert not os.path.exists(p(".no.tsv"))
