"""The dbSNP index kept on the device (bsc_dbsnp_attach; csrc/dbsnpdev.hip, csrc/dbsnpdev_core.h): the flags and the names table the kernels
make in HBM against the host reader's (DbSnpIndex.flags / .names, csrc/dbsnp.c) and the Python restatement's masks (oracle/py_dbsnp.py); the
four bsc_block_*_rawdev* entries with the contig attached and NULL arrays against the same calls with the host arrays; the attachment's life
cycle; pipeline.run(dbsnp_device=True) and bam2bcf -D file to file.  Indexes: tests/dbsnp_crafted.py, written by tools/make_dbsnp_index.py."""
import ctypes as C
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import bs_call_amd as B
import dbsnp_crafted as K
from bs_call_amd import _lib, pipeline
from bs_call_amd import dbsnp as D
from bs_call_amd.abi import PREP_PARAMS, PREP_STATS, SITE_STATS, SITE_STATS_INT_WORDS, VCF_REC
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import BscError
from bs_call_amd.dbsnp import DbSnpIndex
from oracle import py_dbsnp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
X0S = (1, 2, 63, 64, 65, 4097)
NS = (0, 1, 2, 63, 64, 65, 1000)


@pytest.fixture(scope="module")
def caller():
    c = B.SiteCaller()
    yield c
    c.close()


@pytest.fixture(scope="module")
def indexes(tmp_path_factory):
    """[(index file, contig, its sites)]: the crafted index's two contigs and a random 300 k-position contig at spacings 3 and 300"""
    d = tmp_path_factory.mktemp("dbsnp_dev")
    crafted = K.crafted_contigs()
    rnd = {"r3": K.random_sites(300_000, 3, 21), "r300": K.random_sites(300_000, 300, 22)}
    pc, pr = K.write(d / "crafted.idx", crafted), K.write(d / "random.idx", rnd)
    return [(pc, "chrA", crafted["chrA"]), (pc, "chrB", crafted["chrB"]), (pr, "r3", rnd["r3"]), (pr, "r300", rnd["r300"])]


@pytest.fixture(scope="module")
def loaded(indexes):
    """per contig: the open index with the contig loaded, the last site, `whole` (a range from 1 that covers every site and 200 positions
    more) and the host reader's flags of every position a test's range can reach — computed once, shared by the tests"""
    out = []
    for path, name, sites in indexes:
        db = DbSnpIndex(path)
        assert db.load_contig(name) == len(sites)
        last = max(s[0] for s in sites)
        whole = last + 200
        out.append((db, path, name, sites, last, whole, db.flags(1, max(last, max(X0S)) + whole)))
    yield out
    for db, *_ in out:
        db.close()


def _oracle_flags(path, name, n):
    """rs_found of positions 1 .. n from the masks of the Python restatement of the reference's reader"""
    ref = py_dbsnp.Index(path)
    ref.load_contig(name)
    want = np.zeros(n + 64, dtype=np.uint8)
    for b, (mask, fq, _entries, _buf) in ref.bins.items():
        for bit in range(64):
            x = b * 64 + bit
            if (mask >> bit) & 1 and 1 <= x <= n:
                want[x - 1] = 3 if (fq >> bit) & 1 else 1
    return want[:n]


def test_flags_device_equals_the_host_reader_and_the_oracle(caller, loaded):
    import torch

    for db, path, name, sites, last, whole, want in loaded:
        assert (want == _oracle_flags(path, name, len(want))).all(), name
        assert int((want != 0).sum()) == len(sites)
        caller.dbsnp_attach(db)
        d_want = torch.from_numpy(want).cuda()
        pad = 64
        buf = torch.empty(whole + 2 * pad + 64, dtype=torch.uint8, device="cuda")
        base = (-buf.data_ptr()) % 16 + pad  # buf[base] lies on a 16-byte boundary, `pad` guard bytes in front of it
        for x0 in X0S + (last,):
            for n in NS + (whole,):
                for o in range(18):
                    region = buf[: base + o + n + pad]
                    region.fill_(0xAA)
                    caller.dbsnp_flags_device(x0, n, buf.data_ptr() + base + o, C.c_void_p(torch.cuda.current_stream().cuda_stream))
                    exp = torch.full_like(region, 0xAA)  # the guard bytes in front and behind stay as they were
                    exp[base + o : base + o + n] = d_want[x0 - 1 : x0 - 1 + n]
                    assert torch.equal(region, exp), (name, x0, n, o)
        got = D.flags_device(caller, 1, whole)
        assert torch.equal(got, d_want[:whole])
    caller.dbsnp_detach()


def test_names_device_equals_the_host_reader(caller, loaded):
    import torch

    for db, path, name, sites, last, whole, want in loaded:
        caller.dbsnp_attach(db)
        for x0 in X0S + (last,):
            for n in NS + (whole,):
                pos, off, by = db.names(x0, n)
                assert caller.dbsnp_count(x0, n) == (len(pos), len(by)), (name, x0, n)
                d_pos, d_off, d_by = D.names_device(caller, x0, n)
                if n == 0:  # n = 0 does nothing: nothing is written, not even off[0]
                    assert len(d_pos) == 0 and len(d_by) == 0
                    continue
                torch.cuda.synchronize()
                assert (d_pos.cpu().numpy().view(np.uint32) == pos).all() and (d_off.cpu().numpy().view(np.uint32) == off).all(), (name, x0, n)
                assert d_by.cpu().numpy().tobytes() == by, (name, x0, n)
        if name == "r3":
            k, nb = caller.dbsnp_count(1, whole)
            assert k == len(sites) > 50_000  # several workgroups of 256 lanes
            d_pos = torch.zeros(k, dtype=torch.int32, device="cuda")
            d_off = torch.zeros(k + 1, dtype=torch.int32, device="cuda")
            d_by = torch.full((nb + 16,), 0xAA, dtype=torch.uint8, device="cuda")
            for cap_names, cap_bytes in ((k - 1, nb), (k, nb - 1), (0, 0)):
                with pytest.raises(BscError) as ei:
                    caller.dbsnp_names_device(1, whole, d_pos.data_ptr(), d_off.data_ptr(), d_by.data_ptr(), cap_names, cap_bytes)
                assert ei.value.code == -1 and "names" in str(ei.value)
                caller.dbsnp_names_device(1, whole, d_pos.data_ptr(), d_off.data_ptr(), d_by.data_ptr(), k, nb)  # a good call follows every refusal
                torch.cuda.synchronize()
                pos, off, by = db.names(1, whole)
                assert (d_pos.cpu().numpy().view(np.uint32) == pos).all() and (d_off.cpu().numpy().view(np.uint32) == off).all()
                assert d_by[:nb].cpu().numpy().tobytes() == by and bool((d_by[nb:] == 0xAA).all())
    caller.dbsnp_detach()


def test_argument_rules(caller, loaded):
    import torch

    db = loaded[0][0]
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    caller.dbsnp_detach()
    for call in (lambda: caller.dbsnp_count(1, 10), lambda: caller.dbsnp_flags_device(1, 10, buf.data_ptr()),
                 lambda: caller.dbsnp_names_device(1, 10, buf.data_ptr(), buf.data_ptr() + 1024, buf.data_ptr() + 2048, 10, 100)):
        with pytest.raises(BscError) as ei:
            call()
        assert ei.value.code == -1 and "attach" in str(ei.value)
    caller.dbsnp_attach(db)
    for x0, n in ((0, 5), (0xFFFFFFFF, 2), (0xFFFFFFF0, 0x11)):
        with pytest.raises(BscError):
            caller.dbsnp_count(x0, n)
        with pytest.raises(BscError):
            caller.dbsnp_flags_device(x0, n, buf.data_ptr())
    assert caller.dbsnp_count(0xFFFFFFFF, 1) == (0, 0) and caller.dbsnp_count(0xFFFFFFF0, 0x10) == (0, 0)
    caller.dbsnp_flags_device(0xFFFFFFF0, 0x10, buf.data_ptr())
    caller.dbsnp_flags_device(5, 0, None)  # n = 0: valid, nothing done
    torch.cuda.synchronize()
    assert not bool(buf.any())
    caller.dbsnp_detach()


# ---- the block entries ----------------------------------------------------------------------------------------------------------------------
def _write_bam(tmp, seed=9):
    """two contigs of WGBS pairs (the generators of tests/test_gpu_bamdev.py's files), a FASTA of them, and an index that has chrA — one site
    per 5 bp — and chrB, which the BAM lacks, but not chrZ"""
    spec = importlib.util.spec_from_file_location("make_bam_dbsnp_dev", os.path.join(ROOT, "tools", "make_bam.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    rng = np.random.default_rng(seed)
    reference = {"chrA": rng.integers(1, 5, 20_000).astype(np.uint8), "chrZ": rng.integers(1, 5, 9_000).astype(np.uint8)}
    reference["chrA"][6_000:6_200] = 0
    refs = [(k, len(v)) for k, v in reference.items()]
    recs = W.wgbs_records(rng, reference["chrA"], 0, 1200, het_every=300) + W.wgbs_records(rng, reference["chrZ"], 1, 400)
    bam, fa = str(tmp / "in.bam"), str(tmp / "ref.fa")
    W.write_bam(bam, refs, recs)
    with open(fa, "w") as f:
        for name, codes in reference.items():
            f.write(">%s\n" % name)
            s = "".join("NACGT"[c] for c in codes)
            for o in range(0, len(s), 60):
                f.write(s[o : o + 60] + "\n")
    idx = K.write(tmp / "dense.idx", {"chrA": K.random_sites(20_000, 5, 31), "chrB": K.random_sites(5_000, 50, 32)})
    return bam, fa, idx, reference


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return _write_bam(tmp_path_factory.mktemp("dbsnp_blocks"))


def _raw_args(blk, ref, par):
    return (blk.d_tpl, blk.nr, blk.d_seq, blk.seq_bytes, blk.d_misms, blk.n_misms, blk.ins_pad, par.ctypes.data_as(C.c_void_p), int(blk.x), int(blk.y),
            ref.ctypes.data_as(C.c_void_p))


def _records_rawdev(c, blk, ref, reg_stop, flags):
    n = int(blk.y) - int(blk.x) + 1
    par = np.zeros(1, dtype=PREP_PARAMS)
    par["min_qual"][0] = 20
    p = _lib.VcfParams(0, 1, reg_stop)
    out = np.zeros(n, dtype=VCF_REC)
    cnt, st = C.c_uint64(0), np.zeros(1, dtype=PREP_STATS)
    rc = c._L.bsc_block_records_rawdev(c._h, *_raw_args(blk, ref, par), None if flags is None else flags.ctypes.data_as(C.c_void_p), C.byref(p), 1,
                                       out.ctypes.data_as(C.c_void_p), n, C.byref(cnt), st.ctypes.data_as(C.c_void_p), None)
    assert rc == 0, c._L.bsc_last_error()
    return out[: cnt.value].copy()


def _bcf_rawdev_keep(c, blk, ref, reg_stop, rid, flags, names, dev_cap=None):
    """(stream, records, the status of the first call): bsc_block_bcf_rawdev_keep, bsc_block_bcf_again when dev_cap was too small, bsc_bcf_stream_read"""
    n = int(blk.y) - int(blk.x) + 1
    par = np.zeros(1, dtype=PREP_PARAMS)
    par["min_qual"][0] = 20
    p = _lib.VcfParams(0, 1, reg_stop)
    ids = _lib.BcfIds()
    c._L.bsc_bcf_default_ids(C.byref(ids))
    nm, keep = c._bcf_names(names)
    cap = 64 + 192 * n if dev_cap is None else dev_cap
    nb, nr, st = C.c_uint64(0), C.c_uint64(0), np.zeros(1, dtype=PREP_STATS)
    first = c._L.bsc_block_bcf_rawdev_keep(c._h, *_raw_args(blk, ref, par), None if flags is None else flags.ctypes.data_as(C.c_void_p), C.byref(p), 1, rid,
                                           C.byref(ids), None if nm is None else C.addressof(nm), cap, C.byref(nb), C.byref(nr), st.ctypes.data_as(C.c_void_p), None)
    rc = first
    if rc == -1 and nb.value > cap:
        rc = c._L.bsc_block_bcf_again(c._h, None, int(nb.value), C.byref(nb), C.byref(nr))
    assert rc == 0, c._L.bsc_last_error()
    del keep
    out = np.empty(max(int(nb.value), 1), dtype=np.uint8)
    assert c._L.bsc_bcf_stream_read(c._h, 0, nb.value, out.ctypes.data_as(C.c_void_p)) == 0
    c.synchronize()
    return out[: nb.value].tobytes(), nr.value, first


def _same_stats(a, b):
    """Every counter equal; the two methylation profiles — sums of doubles the device adds in arrival order, so two runs of the SAME call differ
    in the last bits — to the 1e-12 tests/test_gpu_chain.py holds them to against the oracle."""
    ia = np.frombuffer(a.tobytes(), dtype=np.uint64)[:SITE_STATS_INT_WORDS]
    ib = np.frombuffer(b.tobytes(), dtype=np.uint64)[:SITE_STATS_INT_WORDS]
    assert (ia == ib).all(), [f for f in SITE_STATS.names if a[f].dtype.kind == "u" and not (a[f] == b[f]).all()]
    for f in ("CpG_ref_meth", "CpG_nonref_meth"):
        np.testing.assert_allclose(a[f], b[f], rtol=1e-12, atol=1e-12)


def _stats(c):
    s = c.site_stats().copy()
    c.reset_site_stats()
    return s


def test_block_entries_with_the_contig_attached(caller, files):
    from bs_call_amd.bam import block_reference

    bam, fa, idx, reference = files
    c = caller
    c.dbsnp_detach()
    c.reset_site_stats()
    n_id = n_forced = n_blocks = 0
    with DbSnpIndex(idx) as db, DeviceBamReader(c, bam, threads=2) as rd:
        refs = rd.refs
        cur = -1
        for blk in rd.device_blocks():
            tid, x, y = int(blk.tid), int(blk.x), int(blk.y)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            if tid != cur:
                cur = tid
                db.load_contig(name)
            ref = block_reference(codes, x, y)
            flags, names = db.flags(x, y - x + 1), db.names(x, y - x + 1)
            kw = dict(reg_stop=len(codes), with_stats=True)
            # the host arrays, nothing attached: what every call must reproduce
            want = {}
            want["bcf"] = c.block_bcf_rawdev(blk, ref, tid, names=names, dbsnp=flags, **kw)[:2] + (_stats(c),)
            want["keep"] = _bcf_rawdev_keep(c, blk, ref, len(codes), tid, flags, names)[:2] + (_stats(c),)
            want["vcf"] = c.block_vcf_rawdev(blk, ref, name, names=names, dbsnp=flags, **kw)[:2] + (_stats(c),)
            want["rec"] = (_records_rawdev(c, blk, ref, len(codes), flags), _stats(c))
            assert want["bcf"][0] == want["keep"][0]
            # attached, NULL for both
            c.dbsnp_attach(db)
            got = {}
            got["bcf"] = c.block_bcf_rawdev(blk, ref, tid, **kw)[:2] + (_stats(c),)
            got["keep"] = _bcf_rawdev_keep(c, blk, ref, len(codes), tid, None, None)[:2] + (_stats(c),)
            got["vcf"] = c.block_vcf_rawdev(blk, ref, name, **kw)[:2] + (_stats(c),)
            got["rec"] = (_records_rawdev(c, blk, ref, len(codes), None), _stats(c))
            for k in ("bcf", "keep", "vcf"):
                assert got[k][0] == want[k][0] and got[k][1] == want[k][1], (k, name, x)
                _same_stats(got[k][2], want[k][2])
            assert got["rec"][0].tobytes() == want["rec"][0].tobytes(), (name, x)
            _same_stats(got["rec"][1], want["rec"][1])
            # a dev_cap too small: the block is refused, bsc_block_bcf_again encodes with the same attached table
            small, n_small, first = _bcf_rawdev_keep(c, blk, ref, len(codes), tid, None, None, dev_cap=4096)
            assert (first == -1) == (len(want["keep"][0]) > 4096) and small == want["keep"][0] and n_small == want["keep"][1]
            _stats(c)
            # one of the two passed while attached: the host array wins, the other comes from the attachment
            zero = np.zeros_like(flags)
            a = c.block_bcf_rawdev(blk, ref, tid, dbsnp=zero, names=(names[0][:0], names[1][:1], b""), **kw)
            b = c.block_bcf_rawdev(blk, ref, tid, dbsnp=flags, **kw)
            c.dbsnp_detach()
            plain = c.block_bcf_rawdev(blk, ref, tid, **kw)
            none = c.block_bcf_rawdev(blk, ref, tid, dbsnp=zero, **kw)
            _stats(c)
            assert a[:2] == none[:2] == plain[:2] and b[:2] == want["bcf"][:2]
            recs = want["rec"][0]
            core = recs["core"]
            n_id += int((recs["rs_found"] != 0).sum())
            n_forced += int((((core["gt"] == 0) & (core["ref_code"] == 1)) | ((core["gt"] == 9) & (core["ref_code"] == 4))).sum())
            if name == "chrA":
                assert int(want["rec"][1]["dbSNP_sites"][0]) == int((recs["rs_found"] != 0).sum())
                assert want["bcf"][0] != plain[0]
            else:  # chrZ: the index lacks it — attached empty, the bytes of a run without an index
                assert want["bcf"][0] == plain[0] and not flags.any()
            n_blocks += 1
    assert n_blocks >= 2 and n_id > 0 and n_forced > 0, (n_blocks, n_id, n_forced)


def test_lifecycle(caller, files):
    from bs_call_amd.bam import block_reference

    bam, fa, idx, reference = files
    c = caller
    c.dbsnp_detach()
    with DbSnpIndex(idx) as db, DeviceBamReader(c, bam, threads=2) as rd:
        refs = rd.refs
        blk = next(iter(rd.device_blocks()))
        tid, x, y = int(blk.tid), int(blk.x), int(blk.y)
        name, codes = refs[tid][0], reference[refs[tid][0]]
        assert name == "chrA"
        ref = block_reference(codes, x, y)
        run = lambda **kw: c.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), **kw)[:2]
        plain = run()
        want = {}
        for ctg in ("chrA", "chrB", "chrZ"):
            n = db.load_contig(ctg)
            want[ctg] = run(dbsnp=db.flags(x, y - x + 1), names=db.names(x, y - x + 1))
            assert (n == 0) == (ctg == "chrZ")
        assert want["chrA"] != want["chrB"] != plain and want["chrZ"] == plain
        db.load_contig("chrA")
        assert c.dbsnp_attach(db) == db.load_contig("chrA")
        db.load_contig("chrB")  # the attachment is a snapshot: loading another contig into db does not change it
        assert run() == want["chrA"]
        assert c.dbsnp_attach(db) == db.load_contig("chrB")  # replaces A
        assert run() == want["chrB"]
        db.load_contig("chrZ")  # a contig the index lacks attaches empty
        assert c.dbsnp_attach(db) == 0 and c.dbsnp_count(1, 20_000) == (0, 0)
        assert run() == plain
        db.load_contig("chrA")
        c.dbsnp_attach(db)
        assert run() == want["chrA"]
        c.dbsnp_detach()
        assert run() == plain
        c.dbsnp_detach()  # twice is fine
    with DbSnpIndex(idx) as db, B.SiteCaller() as c2:  # bsc_destroy frees an attachment left behind
        db.load_contig("chrA")
        c2.dbsnp_attach(db)


def test_a_refused_attach_leaves_nothing_attached(caller, tmp_path):
    ctgs = K.crafted_contigs()
    ctgs["chrBad"] = [(70, "11", False, 0), (64 * 9 + 17, "12345", False, len(K.PREFIXES))]  # an explicit prefix index one behind the last prefix
    idx = K.write(tmp_path / "bad.idx", ctgs)
    with DbSnpIndex(idx) as db:
        db.load_contig("chrA")
        assert caller.dbsnp_attach(db) == len(ctgs["chrA"]) and caller.dbsnp_count(1, 300)[0] > 100
        db.load_contig("chrBad")
        with pytest.raises(BscError) as ei:
            caller.dbsnp_attach(db)
        assert ei.value.code == -1 and "position %d names prefix" % (64 * 9 + 17) in str(ei.value)
        with pytest.raises(BscError) as ei:  # not chrA's entries under the next contig's blocks
            caller.dbsnp_count(1, 300)
        assert "attach" in str(ei.value)
        db.load_contig("chrB")
        assert caller.dbsnp_attach(db) == len(ctgs["chrB"])
    caller.dbsnp_detach()


# ---- file to file ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_and_bam2bcf(tmp_path, caller, files):
    from bs_call_amd.bam import fasta_contig

    bam, fa, idx, reference = files
    ref2 = {name: fasta_contig(fa, name) for name in reference}
    kw = dict(sample="S7", date=(1, 1, 2000), compressed=False, benchmark_mode=True, device_reader=True)
    out = {}
    with DbSnpIndex(idx) as db:
        for what, more in (("host", dict()), ("dev", dict(dbsnp_device=True)), ("host_txt", dict(text=True)), ("dev_txt", dict(text=True, dbsnp_device=True))):
            p, r = str(tmp_path / (what + ".out")), str(tmp_path / (what + ".json"))
            res = pipeline.run(bam, ref2, p, report_path=r, dbsnp=db, **kw, **more)
            out[what] = (open(p, "rb").read(), open(r).read(), res)
        p = str(tmp_path / "none.out")
        pipeline.run(bam, ref2, p, **kw)
        assert open(p, "rb").read() != out["host"][0]  # the index matters on this input
        with pytest.raises(ValueError):
            pipeline.run(bam, ref2, p, dbsnp=db, dbsnp_device=True, sample="S7", compressed=False)
        # a supplied caller comes back with nothing attached
        pipeline.run(bam, ref2, p, dbsnp=db, dbsnp_device=True, caller=caller, **kw)
        assert open(p, "rb").read() == out["host"][0]
        with pytest.raises(BscError):
            caller.dbsnp_count(1, 1)
    assert out["dev"][0] == out["host"][0] and out["dev"][1] == out["host"][1] and out["dev"][2]["contigs"] == ["chrA", "chrZ"]
    assert out["dev_txt"][0] == out["host_txt"][0] and out["dev_txt"][1] == out["host_txt"][1]
    assert b"\trs" in out["dev_txt"][0] or b"\tss" in out["dev_txt"][0]
    # bam2bcf -D: the same bytes under the benchmark-mode header, -O b decoded, --format vcf
    assert os.path.exists(EXE), "run `make demo`"
    for args, want in ((("-D", idx), out["host"][0]), (("-O", "b", "-D" + idx), out["host"][0]), (("--format", "vcf", "-D", idx), out["host_txt"][0]),
                       (("-D", idx, "-O", "b", "--format", "vcf"), out["host_txt"][0])):
        o, r = str(tmp_path / "c.out"), str(tmp_path / "c.json")
        pr = subprocess.run([EXE, *args, bam, fa, o, r, "S7"], capture_output=True, text=True, timeout=300)
        assert pr.returncode == 0, pr.stderr + pr.stdout
        got = open(o, "rb").read()
        if "b" in args or "-O" in args:
            got = gzip.decompress(got)
        assert got == want, args
        assert open(r).read() == out["host"][1], args
        assert pr.stdout.strip() == "%d blocks, %d records written" % (out["host"][2]["blocks"], out["host"][2]["records"])
