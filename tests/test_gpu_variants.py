"""The variant-only call set on the device (csrc/variantsdev.hip: bsc_var_select_kernel, the scan, bsc_var_pack_kernel) — the rule of
include/bscall_amd.h (VARIANT, PARAMS, SELECTED, TOTALS, STREAM):

  1. bsc_variants_sites_device against the host form (csrc/variants.c) and the Python form (bs_call_amd/variants.py) on random record
     bytes: every size around a tile, every selection pattern, with and without the emit-byte array, the thresholds, guard bytes, a room
     one short, the refusal; once more on a one-CU grid
  2. its packed output and device count feed both encoders: their streams equal the host encoders' over the host form's selection
  3. bsc_block_variants_kept behind both _keep calls, against tests/variants_ref.py's selection of the block's FULL stream (which reads
     the stream's own bytes and calls nothing of the library), with its index entries against tests/csi_ref.py; what the context keeps
     beside it is untouched
  4. bam2bcf --variants and pipeline.run(variants_path=) file to file"""
import ctypes as C
import gzip
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import csi_ref
import variants_ref as VR
from bs_call_amd import _lib, pipeline, variants, vcf
from bs_call_amd.abi import VCF_REC
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.dbsnp import DbSnpIndex
from variants_cases import PARAMS, random_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
PAD = 0xEE
GUARD = 2  # records of guard bytes behind the room


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
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def run_sites(caller, recs, par, emit=None, max_recs=None, keep=False):
    """bsc_variants_sites_device over the records split into the two per-position arrays.  Returns (records VCF_REC[min(count, room)],
    count, totals) after checking the guard bytes behind the count and behind the room."""
    n = len(recs)
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 128)
    d_core = dev(raw[:, :64]) if n else torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_aux = dev(raw[:, 64:]) if n else torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_emit = dev(np.asarray(emit, np.uint8)) if emit is not None and n else None
    room = n if max_recs is None else max_recs
    d_recs = torch.full(((room + GUARD) * 128,), PAD, dtype=torch.uint8, device="cuda")
    d_n = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    d_tot = torch.full((10,), 77, dtype=torch.int64, device="cuda")
    caller.variants_sites_device(d_core.data_ptr(), d_aux.data_ptr(), d_emit.data_ptr() if d_emit is not None else None, n, d_recs.data_ptr(), room,
                                 d_n.data_ptr(), d_tot.data_ptr(), params=par)
    torch.cuda.synchronize()
    count = int(d_n.cpu().numpy().view(np.uint64)[0])
    tot = tuple(int(v) for v in d_tot.cpu().numpy().view(np.uint64))
    out = d_recs.cpu().numpy()
    stored = min(count, room)
    assert (out[stored * 128 :] == PAD).all(), "bytes behind the count or behind the room were written"
    if keep:
        return d_recs, d_n, out[: stored * 128].view(VCF_REC), count, tot
    return out[: stored * 128].view(VCF_REC), count, tot


def host_form(recs, par, emit=None):
    """bsc_variants_select_recs; the per-position gate is applied to a copy's core.emit (the bytes of a selected record are untouched)."""
    L = _lib.load()
    src = np.ascontiguousarray(recs).copy()
    if emit is not None and len(src):
        src.view(np.uint8).reshape(-1, 128)[np.asarray(emit) == 0, 4] = 0
    out = np.zeros(max(len(src), 1), VCF_REC)
    n_out, tot = C.c_uint64(0), (C.c_uint64 * 10)()
    p = _lib.VarParams(**par)
    assert L.bsc_variants_select_recs(src.ctypes.data if len(src) else None, len(src), C.byref(p), out.ctypes.data, len(src), C.byref(n_out), tot) == 0
    return out[: n_out.value], tuple(int(v) for v in tot)


def check_sites(caller, n, seed):
    rng = np.random.default_rng(seed)
    n_sel = 0
    for present in ("some", "none", "all", "first", "last") if n else ("some",):
        x0 = 2**32 - n if present == "some" and n else 1 + int(rng.integers(0, 1 << 20))  # positions up to 2^32 - 1
        recs = random_records(rng, n, present, x0=x0)
        if n and present == "some":
            assert int(recs["core"]["pos"][-1]) == 2**32 - 1
        gates = [None, np.ones(n, np.uint8), rng.choice([0, 1, 1, 7], n).astype(np.uint8)]  # no array; all set; a 0 over emitted records
        for emit in gates:
            for par in PARAMS:
                idx = variants.select(recs, par, emit)
                want = recs[idx]
                got, count, tot = run_sites(caller, recs, par, emit)
                h_recs, h_tot = host_form(recs, par, emit)
                assert count == len(idx) == len(h_recs), (n, present, par)
                assert got.tobytes() == want.tobytes() == h_recs.tobytes(), (n, present, par)
                assert tot == variants.totals(want) == h_tot, (n, present, par)
                n_sel += count
        if present == "all":
            assert run_sites(caller, recs, {})[1] == n
        if present in ("first", "last"):
            assert run_sites(caller, recs, {})[1] == (n + 63) // 64
        if present == "none":
            assert run_sites(caller, recs, {})[1:] == (0, (0,) * 10)
        if present == "some" and n:
            emit = gates[2]
            hidden = (emit == 0) & (recs["core"]["emit"] != 0) & (recs.view(np.uint8).reshape(-1, 128)[:, 12] != 0)
            assert n < 64 or hidden.any()  # records only the emit byte keeps out
            # a room one short: the full count, the totals, the first records, nothing beyond the room
            idx = variants.select(recs, {}, emit)
            if len(idx):
                got, count, tot = run_sites(caller, recs, {}, emit, max_recs=len(idx) - 1)
                assert count == len(idx) and got.tobytes() == recs[idx[:-1]].tobytes() and tot == variants.totals(recs[idx])
                got, count, _ = run_sites(caller, recs, {}, emit, max_recs=0)
                assert count == len(idx) and len(got) == 0
    return n_sel


# ---- 1. the selection against the host form and the Python rule -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 4113])
def test_sites_device_equals_the_host_form_and_the_python_rule(caller, n):
    n_sel = check_sites(caller, n, 7000 + n)
    if n == 4113:
        assert n_sel > 10_000
        recs = random_records(np.random.default_rng(1), n)
        sel = recs[variants.select(recs)]
        assert n // 5 < len(sel) < n // 2 and (sel["core"]["gt"] > 9).any()
        assert (~np.isin(sel.view(np.uint8).reshape(-1, 128)[:, 12], list(b"ACGT"))).any()


def test_sites_device_on_a_one_cu_grid(one_cu, caller):
    n = 20_003  # 313 tiles over a grid of 8 workgroups of 4 waves: nine full rounds and a ragged tenth
    assert check_sites(one_cu, n, 7777) > 10_000
    recs = random_records(np.random.default_rng(3), n)
    a, b = run_sites(one_cu, recs, {}), run_sites(caller, recs, {})
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]  # the output does not depend on the grid


def test_refusals_leave_the_context_usable(caller):
    recs = random_records(np.random.default_rng(5), 300)
    with pytest.raises(B.BscError, match="reserved"):
        run_sites(caller, recs, {"reserved": 1})
    L, h = caller._L, caller._h
    p = _lib.VarParams()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert L.bsc_variants_sites_device(h, t.data_ptr(), t.data_ptr(), None, 1, None, t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), None) == -1
    assert L.bsc_variants_sites_device(h, None, None, None, 1, C.byref(p), t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), None) == -1
    assert L.bsc_variants_sites_device(h, t.data_ptr() + 8, t.data_ptr(), None, 1, C.byref(p), t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), None) == -1
    assert b"aligned" in L.bsc_last_error()
    assert L.bsc_variants_sites_device(h, t.data_ptr(), t.data_ptr(), None, 1, C.byref(p), None, 1, t.data_ptr(), t.data_ptr(), None) == -1
    nb, nr = C.c_uint64(5), C.c_uint64(5)
    bad = _lib.VarParams(reserved=7)
    assert L.bsc_block_variants_kept(h, C.byref(bad), 1 << 16, C.byref(nb), C.byref(nr), None) == -1 and b"reserved" in L.bsc_last_error()
    assert (nb.value, nr.value) == (0, 0)
    got, count, tot = run_sites(caller, recs, {})
    idx = variants.select(recs)
    assert count == len(idx) > 50 and got.tobytes() == recs[idx].tobytes() and tot == variants.totals(recs[idx])


# ---- 2. the packed output feeds both encoders -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 4113])
def test_packed_output_feeds_both_encoders(caller, n):
    rng = np.random.default_rng(7100 + n)
    recs = random_records(rng, n)
    raw = recs.view(np.uint8).reshape(-1, 128)
    raw[:, 5] %= 10  # records both encoders write: gt 0 .. 9, n_gl 0 .. 6
    raw[:, 10] %= 7
    L = caller._L
    for par in ({}, {"min_phred": 60, "pass_only": 1}):
        d_recs, d_n, got, count, _ = run_sites(caller, recs, par, keep=True)
        sel, _ = host_form(recs, par)
        assert count == len(sel) > 0 and got.tobytes() == sel.tobytes()
        room = n  # max_recs: the records' room, more than the count — the device count limits the encoders
        cap = 1024 * len(sel)
        d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
        d_tot = torch.zeros(3, dtype=torch.int64, device="cuda")
        caller.bcf_block_device(d_recs.data_ptr(), d_n.data_ptr(), room, 3, d_out.data_ptr(), cap, d_tot.data_ptr())
        torch.cuda.synchronize()
        tot = [int(v) for v in d_tot.cpu()]
        want = vcf.bcf_block(sel, 3)
        assert tot == [len(want), 0, len(sel)] and d_out.cpu().numpy()[: tot[0]].tobytes() == want
        d_out.fill_(PAD)
        caller.vcf_text_block_device(d_recs.data_ptr(), d_n.data_ptr(), room, b"chr7", d_out.data_ptr(), cap, d_tot.data_ptr())
        torch.cuda.synchronize()
        tot = [int(v) for v in d_tot.cpu()]
        buf = C.create_string_buffer(2048)
        lines = []
        for i in range(len(sel)):
            k = L.bsc_vcf_format_rec(sel.ctypes.data + 128 * i, b"chr7", None, buf, 2048)
            assert k > 0
            lines.append(buf.raw[:k] + b"\n")
        want = b"".join(lines)
        assert tot == [len(want), 0, len(sel)] and d_out.cpu().numpy()[: tot[0]].tobytes() == want
        assert (d_out.cpu().numpy()[tot[0] :] == PAD).all()


# ---- 3. the block entry behind both _keep calls ---------------------------------------------------------------------------------------------
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
    """A BAM of four contigs.  chrA: 6 000 positions at ~40x, a heterozygous site every 300 and, every 487 positions, an A or a T of the
    reference that the sample carries as the other of the two on both chromosomes (a homozygous ALT: bisulfite leaves A and T alone); a
    dbSNP index over it that lists random sites and half of the heterozygous ones.  chrT: 60 positions (a block shorter than a tile, no
    variant).  chrG: 30 000 positions in several blocks with gaps between the reads.  chrB: 3 000 positions at ~40x, a heterozygous site
    every 250."""
    import dbsnp_crafted as K

    d = tmp_path_factory.mktemp("variant_files")
    rng = np.random.default_rng(4712)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8), "chrB": rng.integers(1, 5, 3_000).astype(np.uint8)}
    sample = reference["chrA"].copy()
    for p in range(486, 6_000, 487):
        if sample[p] in (1, 4):
            sample[p] = 5 - sample[p]
    recs = (W.wgbs_records(rng, sample, 0, 1_200, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50, err=0.0)
            + W.wgbs_records(rng, reference["chrG"], 2, 60) + W.wgbs_records(rng, reference["chrB"], 3, 600, het_every=250))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    sites = {p: (p, n, f, q) for p, n, f, q in K.random_sites(6_000, 40, 33)}
    for k in range(600, 6_000, 600):
        sites[k] = (k, "77%d" % k, False, 0)
    idx = K.write(d / "variants.idx", {"chrA": [sites[p] for p in sorted(sites)]})
    return d, bam, fa, refs, reference, idx


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


def csi_want(stream, fmt, min_shift):
    starts = [e[2] for e in csi_ref.entries_of(stream, fmt, 0)] if stream else []
    # entries_of(.., 0) cuts at every change of position: the records' starts where no two share a position (one contig, one record each)
    return csi_ref.entries_of(stream, fmt, min_shift, sync=[0] + starts[64::64] + [len(stream)])


BLOCK_PARAMS = [{}, {"min_phred": 30, "pass_only": 1}, {"known_only": 1}]


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference, idx = small
    L, h = caller._L, caller._h
    n_blocks = n_short = n_empty = n_with = n_sel = n_known = n_het = n_hom = 0
    with DbSnpIndex(idx) as db, DeviceBamReader(caller, bam, threads=2) as rd:
        cur = -1
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            x, y = int(blk.x), int(blk.y)
            if tid != cur:
                cur = tid
                db.load_contig(name)
            ref = block_reference(codes, x, y)
            flags, names = db.flags(x, y - x + 1), db.names(x, y - x + 1)
            known = set((x + np.nonzero(flags)[0]).tolist())
            kw = dict(reg_stop=len(codes), dbsnp=flags, names=names)
            n_short += y - x + 1 < 64
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, keep=True, **kw)
            ent0, r0 = caller.block_csi_kept(14)
            table0 = caller.block_meth_kept(name)
            blk_sel = 0
            for par in BLOCK_PARAMS:
                want, w_rec, w_tot = VR.select(bcf0, False, par, known)
                got, g_rec, g_tot = caller.block_variants_kept(par)
                assert got == want and g_rec == w_rec and g_tot == w_tot, (name, x, par)
                for min_shift in (14, 6):
                    ent, r = caller.block_variants_csi_kept(min_shift)
                    assert [tuple(int(v) for v in e) for e in ent] == csi_want(want, "bcf", min_shift) and r == w_rec
                if not par:
                    blk_sel = w_rec
                    n_known += w_tot[5]
                    n_het += w_tot[3]
                    n_hom += w_tot[0] - w_tot[3]
            n_empty += blk_sel == 0
            n_with += blk_sel > 0
            n_sel += blk_sel
            # a room one short, then the exact room; a read past the end
            full, _, tot = caller.block_variants_kept()
            nb, nr, t10 = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 10)()
            ok = _lib.VarParams()
            if full:
                assert L.bsc_block_variants_kept(h, C.byref(ok), len(full) - 1, C.byref(nb), C.byref(nr), t10) == -1
                assert nb.value == len(full) and b"dev_cap" in L.bsc_last_error() and tuple(int(v) for v in t10) == tot
                out = np.zeros(8, np.uint8)
                assert L.bsc_variants_stream_read(h, 0, 1, out.ctypes.data) == -1  # a refused call left no stream
            assert L.bsc_block_variants_kept(h, C.byref(ok), max(len(full), 1), C.byref(nb), C.byref(nr), None) == 0
            assert (nb.value, nr.value) == (len(full), tot[0])
            assert caller.variants_stream_read(0, len(full)) == full
            out = np.zeros(len(full) + 8, np.uint8)
            assert L.bsc_variants_stream_read(h, 1, len(full), out.ctypes.data) == -1 and b"beyond" in L.bsc_last_error()
            if len(full) > 40:
                assert caller.variants_stream_read(17, 23) == full[17:40]
            # what the context keeps beside it is untouched
            assert kept_stream(caller, len(bcf0)) == bcf0
            ent1, r1 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() and r0 == r1 == n_rec
            assert caller.block_meth_kept(name) == table0
            assert caller.block_variants_kept()[0] == full  # ... and behind the table call
            # behind the text encoder's keep call: the lines of the same records
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, **kw)
            assert n_txt == n_rec
            for par in BLOCK_PARAMS:
                want, w_rec, w_tot = VR.select(text, True, par, known)
                got, g_rec, g_tot = caller.block_variants_kept(par)
                assert got == want and g_rec == w_rec and g_tot == w_tot, (name, x, par)
                assert g_tot == VR.select(bcf0, False, par, known)[2]
                ent, r = caller.block_variants_csi_kept(14)
                assert [tuple(int(v) for v in e) for e in ent] == csi_want(want, "vcf", 14) and r == w_rec
            assert kept_stream(caller, len(text)) == text
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, **kw)
            assert L.bsc_block_variants_kept(h, C.byref(ok), 1 << 20, C.byref(nb), C.byref(nr), None) == -1
            assert b"no single block" in L.bsc_last_error() and nb.value == 0
            n_blocks += 1
    assert n_blocks > 4 and n_short >= 1 and n_empty >= 1, (n_blocks, n_short, n_empty)
    assert n_sel >= 10 and n_with >= 2 and n_het >= 1 and n_hom >= 1 and n_known >= 1, (n_sel, n_with, n_het, n_hom, n_known)


def test_a_detached_variant_stream_goes_through_the_device_writer(caller, small):
    _, bam, _, refs, reference, _ = small
    L, h = caller._L, caller._h
    with DeviceBamReader(caller, bam, threads=2) as rd:
        blk = next(iter(rd.device_blocks()))
        name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
        ref = block_reference(codes, int(blk.x), int(blk.y))
        caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
        full, n_rec, _ = caller.block_variants_kept()
        assert n_rec > 0
        p, nb = C.c_void_p(), C.c_uint64()
        assert L.bsc_variants_stream_detach(h, C.byref(p), C.byref(nb)) == 0 and nb.value == len(full) and p.value
        p2, nb2 = C.c_void_p(), C.c_uint64(9)
        assert L.bsc_variants_stream_detach(h, C.byref(p2), C.byref(nb2)) == -1 and not p2.value and nb2.value == 0  # once
        z = caller.bgzf()
        z.write_device(p.value, len(full))
        comp = z.take() + z.close()
        assert gzip.decompress(comp) == full and comp.endswith(vcf.BGZF_EOF)
        assert L.bsc_detached_free(h, p) == 0
        assert caller.block_variants_kept()[0] == full  # the next call takes a buffer again


# ---- 4. file to file ----------------------------------------------------------------------------------------------------------------------
def run_exe(*args, env=None, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout
    return r


def split_file(data, text):
    """(header bytes, records bytes) of an uncompressed BCF or VCF file"""
    if text:
        at = data.index(b"\n", 0 if data.startswith(b"#CHROM") else data.index(b"\n#CHROM") + 1) + 1
        return data[:at], data[at:]
    (lt,) = struct.unpack_from("<I", data, 5)
    return data[: 9 + lt], data[9 + lt :]


def file_select(records, text, refs, par=None, known=None):
    """variants_ref's selection of a whole file's records, contig by contig (known: contig name -> positions)"""
    recs = (VR.text_records if text else VR.bcf_records)(records)
    groups = []
    for beg, end, _ in recs:
        key = records[beg:end].split(b"\t", 1)[0].decode() if text else refs[struct.unpack_from("<i", records, beg + 8)[0]][0]
        if groups and groups[-1][0] == key:
            groups[-1][2] = end
        else:
            groups.append([key, beg, end])
    out, tot = [], np.zeros(10, np.int64)
    for key, beg, end in groups:
        b, _, t = VR.select(records[beg:end], text, par, (known or {}).get(key, ()))
        out.append(b)
        tot += np.array(t)
    return b"".join(out), tuple(int(v) for v in tot)


def stdout_line(t):
    return "%d variant records written (snp %d, multi %d, het %d, pass %d, known %d, ts %d, tv %d)\n" % (t[0], t[1], t[2], t[3], t[4], t[5], t[7], t[8])


def test_bam2bcf_variants_and_pipeline(small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference, idx = small
    p = lambda s: str(d / ("f" + s))
    rd = lambda path: open(path, "rb").read()
    # -O u: the main file's header, then the selection of the main file's records; everything else as without the switch
    base = run_exe("--meth", p(".u.bed"), bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    head, records = split_file(rd(p(".u.bcf")), False)
    want, tot = file_select(records, False, refs)
    assert tot[0] >= 10 and tot[3] >= 1 and tot[0] > tot[3] and tot[7] >= 1 and tot[8] >= 1, tot
    out = run_exe("--variants", p(".uv.var.bcf"), "--meth", p(".uv.bed"), bam, fa, p(".uv.bcf"), p(".uv.json"), "S9")
    assert rd(p(".uv.var.bcf")) == head + want
    assert rd(p(".uv.bcf")) == rd(p(".u.bcf")) and rd(p(".uv.json")) == rd(p(".u.json")) and rd(p(".uv.bed")) == rd(p(".u.bed"))
    assert out == base + stdout_line(tot)
    # the thresholds
    par = {"min_phred": 30, "pass_only": 1}
    want_t, tot_t = file_select(records, False, refs, par)
    out = run_exe("--variants", p(".t.var.bcf"), "--variants-min-qual", "30", "--variants-pass", bam, fa, p(".t.bcf"), p(".t.json"), "S9")
    assert rd(p(".t.var.bcf")) == head + want_t and 0 < tot_t[0] < tot[0] and out.endswith(stdout_line(tot_t))
    # -O b --index -D, with the dbSNP switch: BCF and text; the main file, its .csi, the report and the table are those of the run without
    with DbSnpIndex(idx) as db:
        db.load_contig("chrA")
        known = {"chrA": set((1 + np.nonzero(db.flags(1, 6_000))[0]).tolist())}
    for text in (False, True):
        fmt = ["--format", "vcf"] if text else []
        ext = ".vcf.gz" if text else ".bcf"
        opts = fmt + ["-O", "b", "--index", "-D", idx, "--meth", p(".b%d.bed.gz" % text)]
        base = run_exe(*opts, bam, fa, p(".b%d" % text + ext), p(".b%d.json" % text), "S9")
        head_b, records_b = split_file(csi_ref.inflate(rd(p(".b%d" % text + ext))), text)
        for k, (sw, par_k) in enumerate((([], {}), (["--variants-known"], {"known_only": 1}))):
            var = p(".bv%d%d.var" % (text, k) + ext)
            opts_v = fmt + ["-O", "b", "--index", "-D", idx, "--meth", p(".bv%d.bed.gz" % text)]
            out = run_exe(*opts_v, "--variants", var, *sw, bam, fa, p(".bv%d" % text + ext), p(".bv%d.json" % text), "S9")
            want_b, tot_b = file_select(records_b, text, refs, par_k, known)
            blob = rd(var)
            assert blob.endswith(vcf.BGZF_EOF) and csi_ref.inflate(blob) == head_b + want_b, (text, sw)
            assert out == base + stdout_line(tot_b) and tot_b[5] >= 1
            assert not k or 0 < tot_b[0] == tot_b[5]
            for a, b in ((".bv%d" % text + ext, ".b%d" % text + ext), (".bv%d" % text + ext + ".csi", ".b%d" % text + ext + ".csi"),
                         (".bv%d.json" % text, ".b%d.json" % text), (".bv%d.bed.gz" % text, ".b%d.bed.gz" % text)):
                assert rd(p(a)) == rd(p(b)), (a, b)
            # the variant file's own index: tests/csi_ref.py's, and a fetch through it equals a linear scan
            csi = rd(var + ".csi")
            assert csi.endswith(vcf.BGZF_EOF) and gzip.decompress(csi) == csi_ref.build(blob, 14)
            parsed = csi_ref.parse(blob)
            ix = vcf.read_csi(var + ".csi")
            n_hit = 0
            for cname, a, b in csi_ref.sweep(refs[:1] + refs[3:], 14, np.random.default_rng(5), n_random=60):
                got = vcf.fetch(var, cname, a, b, index=ix)
                assert got == csi_ref.linear(parsed, cname, a, b), (cname, a, b)
                n_hit += bool(got)
            assert n_hit >= 3
    # pipeline.run(variants_path=...) writes the same file, for either format, compressed or not
    for text in (False, True):
        for compressed in (False, True):
            out = p(".pipe%d%d" % (text, compressed))
            s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, text=text, compressed=compressed,
                             variants_path=out + ".var", variants_params={"min_phred": 30, "pass_only": 1})
            got = rd(out + ".var")
            got = csi_ref.inflate(got) if compressed else got
            head_p, records_p = split_file(csi_ref.inflate(rd(out)) if compressed else rd(out), text)
            want_p, tot_p = file_select(records_p, text, refs, par)
            assert got == head_p + want_p and s["variant_records"] == tot_p[0] and s["variant_totals"] == tot_p
            if not text:
                assert want_p == want_t and tot_p == tot_t
    # refused where --meth is: sharded runs, the host paths; no file is left behind
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), variants_path=p(".no.var"))
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, variants_path=p(".no.var"), shard_rank=0, shard_world=2)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, variants_params={"pass_only": 1})
    for args, env in ((["--rank", "0", "--world", "2"], None), ([], {"BAM2BCF_HOST_READER": "1"}), ([], {"BAM2BCF_HOST_BCF": "1"})):
        r = run_exe(*args, "--variants", p(".no.var"), bam, fa, p(".no"), p(".no.json"), env=env, ok=False)
        assert r.returncode == 2 and "--variants" in r.stderr
    for args in (["--variants-pass"], ["--variants-min-qual", "3"], ["--variants", p(".no.var"), "--variants-min-qual", "x"]):
        r = run_exe(*args, bam, fa, p(".no"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--variants" in r.stderr
    assert not os.path.exists(p(".no")) and not os.path.exists(p(".no.var")) and not os.path.exists(p(".no.json"))
