"""The CSI index on the device: bsc_csi_scan_device (csrc/csidev.hip) over synthetic streams against a Python walk; bsc_block_csi_kept behind
a kept text block; the index beside a device BGZF writer with a record that starts exactly at a member boundary; and bam2bcf -O b --index
file to file, for BCF and for VCF text: the data file's bytes are those of the run without --index, the inflated .csi equals
tests/csi_ref.py's, and vcf.fetch equals a linear scan over random ranges and every window edge."""
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
import test_bcf as TB
from bs_call_amd import _lib, vcf
from bs_call_amd.abi import VCF_REC
from bs_call_amd.caller import CSI_BCF, CSI_ENTRY, CSI_VCF, CsiIndex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
M = 0xFF00
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
FMT = {"bcf": CSI_BCF, "vcf": CSI_VCF}


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def _recs(rng, positions):
    recs = np.zeros(len(positions), dtype=VCF_REC)
    for i, p in enumerate(positions):
        recs[i] = TB._random_rec(rng)
        recs[i]["core"]["pos"] = p
        recs[i]["core"]["emit"] = 1
    return recs


@pytest.fixture(scope="module")
def streams():
    """{"bcf" | "vcf": bytes, "n": records, "recs": VCF_REC[]}: nearly 3 000 records of one contig: dense stretches (a 64-position tile holds tens of records), gaps, and a record
    at 0-based 2^k - 1 and 2^k for every k the contig has."""
    rng = np.random.default_rng(20261020)
    edges = [e for k in range(5, 19) for e in ((1 << k), (1 << k) + 1)]  # 1-based
    pos = set(edges) | {1} | set(int(v) for v in rng.integers(1, 3000, 2200)) | set(int(v) for v in rng.integers(3000, 300_000, 1400))
    recs = _recs(rng, sorted(pos))
    assert 2500 < len(recs) <= 4000
    return {"n": len(recs), "bcf": vcf.bcf_block(recs, 3), "vcf": ("\n".join(vcf.format_records_c(recs, "chrS")) + "\n").encode(), "recs": recs}


def _tile_sync(stream, fmt):
    """The offsets an encoder leaves: the first record at or behind every multiple of 64 positions (equal neighbours: an empty tile)."""
    ent = csi_ref.entries_of(stream, fmt, 6)  # one run per 64-position window
    n_tiles = ent[-1][0] + 1
    off, k = [], 0
    for t in range(n_tiles):
        while k < len(ent) and ent[k][0] < t:
            k += 1
        off.append(ent[k][2] if k < len(ent) else len(stream))
    return off + [len(stream)]


def _scan(caller, fmt, stream, sync, min_shift, cap=None):
    """(entries as tuples, entries there are, records, error bits); checks that nothing behind the capacity was written."""
    L = caller._L
    d_s = torch.frombuffer(bytearray(stream) if stream else bytearray(1), dtype=torch.uint8).to("cuda")
    d_y = torch.tensor(sync, dtype=torch.int64, device="cuda") if sync is not None else None
    n_sync = len(sync) - 1 if sync is not None else 0
    if cap is None:
        cap = len(csi_ref.entries_of(stream, fmt, min_shift, sync=sync)) + 3
    d_e = torch.full((2 * cap + 16,), -1, dtype=torch.int64, device="cuda")
    d_t = torch.full((3,), 77, dtype=torch.int64, device="cuda")
    rc = L.bsc_csi_scan_device(caller._h, FMT[fmt], C.c_void_p(d_s.data_ptr()), len(stream), C.c_void_p(d_y.data_ptr()) if d_y is not None else None, n_sync,
                               min_shift, C.c_void_p(d_e.data_ptr()), cap, C.c_void_p(d_t.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.bsc_last_error()
    torch.cuda.synchronize()
    tot = [int(v) for v in d_t.cpu().numpy()]
    e = d_e.cpu().numpy()
    n = min(tot[0], cap)
    assert (e[2 * n :] == -1).all(), "entries behind the count / the capacity were written"
    return [tuple(int(v) for v in r) for r in e[: 2 * n].view(CSI_ENTRY)], tot[0], tot[1], tot[2]


@pytest.mark.parametrize("fmt", ["bcf", "vcf"])
@pytest.mark.parametrize("min_shift", [5, 6, 7, 14])
def test_scan_by_tile_offsets(caller, streams, fmt, min_shift):
    s, N = streams[fmt], streams["n"]
    sync = _tile_sync(s, fmt)
    assert len(sync) > 1024 and any(a == b for a, b in zip(sync, sync[1:]))  # several workgroups; empty tiles
    want = csi_ref.entries_of(s, fmt, min_shift, sync=sync)
    assert _scan(caller, fmt, s, sync, min_shift) == (want, len(want), N, 0)
    if min_shift == 14:  # a run that spans three intervals and more comes out as adjacent entries, one per interval that holds a record of it
        run = [w for w, _, _ in want[:6]]
        assert run == [0] * 6 and len(csi_ref.merged(want)) < len(want) // 10
    if min_shift == 5:  # windows smaller than a tile: more than one entry inside an interval
        assert len(want) > len([1 for a, b in zip(sync, sync[1:]) if a != b])


@pytest.mark.parametrize("fmt", ["bcf", "vcf"])
def test_scan_intervals_and_capacity(caller, streams, fmt):
    s, N = streams[fmt], streams["n"]
    starts = [e[2] for e in csi_ref.entries_of(s, fmt, 0)]
    rng = np.random.default_rng(8)
    cuts = sorted(int(v) for v in rng.choice(starts[1:], 37, replace=False))
    sync = [0, 0, 0] + cuts[:20] + [cuts[20]] * 3 + cuts[21:] + [len(s)] * 4  # empty intervals at the start, in the middle, at the end
    want = csi_ref.entries_of(s, fmt, 7, sync=sync)
    assert _scan(caller, fmt, s, sync, 7) == (want, len(want), N, 0)
    one = csi_ref.entries_of(s, fmt, 7)
    assert _scan(caller, fmt, s, None, 7) == (one, len(one), N, 0)  # d_sync = NULL: one lane walks the stream
    assert _scan(caller, fmt, s, [0, len(s)], 7) == (one, len(one), N, 0)
    assert _scan(caller, fmt, s, sync, 7, cap=len(want) - 1) == (want[:-1], len(want), N, 0)  # one too small: the count needed, none beyond
    assert _scan(caller, fmt, s, sync, 7, cap=0) == ([], len(want), N, 0)
    first = s[: starts[1]]
    w0 = csi_ref.entries_of(first, fmt, 14)
    assert len(w0) == 1 and _scan(caller, fmt, first, None, 14) == (w0, 1, 1, 0) and _scan(caller, fmt, first, [0, 0, len(first), len(first)], 14) == (w0, 1, 1, 0)
    assert _scan(caller, fmt, b"", None, 14) == ([], 0, 0, 0) and _scan(caller, fmt, b"", [0], 14) == ([], 0, 0, 0) and _scan(caller, fmt, b"", [0, 0, 0], 14) == ([], 0, 0, 0)


def test_scan_text_names_and_positions(caller, streams):
    recs = streams["recs"][:40].copy()
    recs["core"]["pos"][:3] = (1, 2, 9)
    recs["core"]["pos"][3:] = np.arange(100_000_000, 100_000_000 + 37 * 7_000_000, 7_000_000)[:37]  # 9 digits
    for name in ("c", "N" * 255):
        s = ("\n".join(vcf.format_records_c(recs, name)) + "\n").encode()
        assert s.startswith(name.encode() + b"\t1\t") and b"\t345000000\t" in s
        for min_shift in (6, 14):
            want = csi_ref.entries_of(s, "vcf", min_shift)
            assert _scan(caller, "vcf", s, None, min_shift) == (want, len(want), 40, 0)
            starts = [e[2] for e in csi_ref.entries_of(s, "vcf", 0)]
            sync = [0] + starts[1::3] + [len(s)]
            want = csi_ref.entries_of(s, "vcf", min_shift, sync=sync)
            assert _scan(caller, "vcf", s, sync, min_shift) == (want, len(want), 40, 0)


def test_scan_refuses_a_damaged_stream(caller, streams):
    s = streams["bcf"]
    starts = [e[2] for e in csi_ref.entries_of(s, "bcf", 0)]
    sync = [0] + starts[100::100] + [len(s)]
    k = starts[1234]  # in interval 12
    bad = s[:k] + struct.pack("<I", 0x7FFFFFF0) + s[k + 4 :]  # l_shared: the record would end far behind the stream
    ent, n, recs, err = _scan(caller, "bcf", bad, sync, 14, cap=4000)
    want = csi_ref.entries_of(s, "bcf", 14, sync=sync)
    assert err == 1 and recs == streams["n"] - (starts.index(sync[13]) - 1234)  # the walk of that interval stops there, the others are whole
    assert ent[:12] == want[:12] and n <= len(want)
    bad = s[: starts[7]] + s[starts[5] : starts[6]] + s[starts[8] :]  # a position that goes backwards
    assert _scan(caller, "bcf", bad, None, 14, cap=4000)[3] == 2
    assert _scan(caller, "bcf", s[:-3], sync[:-1] + [len(s) - 3], 14, cap=4000)[3] == 1  # the stream ends inside its last record
    assert _scan(caller, "bcf", s, [0, starts[9], starts[5], len(s)], 14, cap=4000)[3] & 8 and _scan(caller, "bcf", s, [0, len(s) + 64], 14, cap=4000)[3] == 8
    t = streams["vcf"]
    assert _scan(caller, "vcf", t[:-1], None, 14, cap=4000)[3] == 1 and _scan(caller, "vcf", t[:50] + b"\n" + t[50:], None, 14, cap=4000)[3] == 4


def test_scan_argument_errors(caller):
    L = caller._L
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, st = C.c_void_p(d.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.bsc_csi_scan_device(None, 0, p, 8, None, 0, 14, p, 1, p, st) == -1
    assert L.bsc_csi_scan_device(caller._h, 2, p, 8, None, 0, 14, p, 1, p, st) == -1
    assert L.bsc_csi_scan_device(caller._h, 0, p, 8, None, 0, 32, p, 1, p, st) == -1 and L.bsc_csi_scan_device(caller._h, 0, p, 8, None, 0, -1, p, 1, p, st) == -1
    assert L.bsc_csi_scan_device(caller._h, 0, None, 8, None, 0, 14, p, 1, p, st) == -1 and L.bsc_csi_scan_device(caller._h, 0, p, 8, None, 0, 14, None, 1, p, st) == -1
    assert L.bsc_csi_scan_device(caller._h, 0, p, 8, None, 0, 14, p, 1, None, st) == -1 and L.bsc_csi_scan_device(caller._h, 0, p, 8, p, 0, 14, p, 1, p, st) == -1
    e, n, r = C.c_void_p(), C.c_uint64(), C.c_uint64()
    with B.SiteCaller() as fresh:
        assert L.bsc_block_csi_kept(fresh._h, 14, C.byref(e), C.byref(n), C.byref(r)) == -1 and b"no stream on the device" in L.bsc_last_error()
    assert L.bsc_block_csi_kept(None, 14, C.byref(e), C.byref(n), C.byref(r)) == -1
    torch.cuda.synchronize()


def test_index_beside_a_device_writer_with_a_record_at_a_member_boundary(caller, streams):
    """The host-written prefix is padded so that the first record starts at u = 0xFF00 exactly; the second block starts inside a member."""
    contigs = [("chrS", 300_000), ("chrT", 1_000), ("c", 300_000)]
    header = vcf.header_text(contigs, "S1", benchmark_mode=True)
    pad = M - (9 + len(header.encode()) + 1)
    filler = "##pad=" + "x" * (pad - 7) + "\n"
    header = header.replace("#CHROM", filler + "#CHROM")
    head = b"BCF\x02\x02" + struct.pack("<I", len(header.encode()) + 1) + header.encode() + b"\0"
    assert len(head) == M
    recs = streams["recs"]
    blocks = [(0, vcf.bcf_block(recs[:1700], 0)), (0, vcf.bcf_block(recs[1700:], 0)), (2, vcf.bcf_block(recs[:900], 2))]
    z = caller.bgzf()
    z.write(head)
    assert z.tell() == (M, 1)
    parts = []
    with CsiIndex(z, CSI_BCF, contigs, 14) as ix:
        L = caller._L
        h2 = C.c_void_p()
        assert L.bsc_csi_open(z._h, 0, 14, 0, None, None, C.byref(h2)) == -1 and b"an index already" in L.bsc_last_error()
        for tid, s in blocks:
            t = torch.frombuffer(bytearray(s), dtype=torch.uint8).to("cuda")
            starts = [e[2] for e in csi_ref.entries_of(s, "bcf", 0)]
            sync = [0] + starts[64::64] + [len(s)]
            d_sync = torch.tensor(sync, dtype=torch.int64, device="cuda")  # (kept alive across the call)
            ent, n, _, err = caller.csi_scan_device(CSI_BCF, t.data_ptr(), len(s), d_sync.data_ptr(), len(sync) - 1, 14)
            assert err == 0 and n == len(ent) == len(csi_ref.entries_of(s, "bcf", 14, sync=sync))
            ix.add(tid, ent, len(s))
            z.write_device(t.data_ptr(), len(s))
            parts.append(z.take())
        with pytest.raises(B.BscError, match="not closed yet"):
            ix.finish()
        total, n_members = z.tell()
        assert total == M + sum(len(s) for _, s in blocks) and n_members == total // M
        h_z = z._h
        parts.append(z.close())
        blob = b"".join(parts)
        names, lens = (C.c_char_p * 1)(b"chrS"), (C.c_uint32 * 1)(300_000)
        assert L.bsc_csi_open(h_z, 0, 14, 1, names, lens, C.byref(h2)) == -1 and b"not an open BGZF writer" in L.bsc_last_error()  # a closed writer
        assert L.bsc_bgzf_tell(h_z, None, None) == -1
        with pytest.raises(B.BscError, match="writer is closed"):
            ix.add(2, np.zeros(0, CSI_ENTRY), 0)
        csi = ix.finish()
    assert csi_ref.inflate(blob) == head + b"".join(s for _, s in blocks)
    want = csi_ref.build(blob, 14)
    assert gzip.decompress(csi) == want
    first_voff = struct.unpack_from("<Q", want, 16 + 4 + 4 + 4)[0]  # contig 0, bin 0: loffset
    assert first_voff & 0xFFFF == 0 and first_voff >> 16 == csi_ref.member_sizes(blob)[0]  # the first byte of member 1


def test_kept_text_block(caller, tmp_path):
    """bsc_block_csi_kept behind bsc_block_vcf_rawdev_keep: the entries of the kept stream by the encoder's own tile offsets."""
    from bs_call_amd.bam import block_reference
    from bs_call_amd.bamdev import DeviceBamReader

    rng = np.random.default_rng(9)
    codes = rng.integers(1, 5, 40_000).astype(np.uint8)
    bam = str(tmp_path / "k.bam")
    W.write_bam(bam, [("chrK", len(codes))], W.wgbs_records(rng, codes, 0, 3_000, het_every=300))
    n = 0
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            x, y = int(blk.x), int(blk.y)
            text, n_rec, _ = caller.block_vcf_rawdev(blk, block_reference(codes, x, y), "chrK", reg_stop=len(codes))
            for min_shift in (14, 9):
                ent, records = caller.block_csi_kept(min_shift)
                got = [tuple(int(v) for v in e) for e in ent]
                assert records == n_rec and csi_ref.merged(got) == csi_ref.entries_of(text, "vcf", min_shift)
                assert [e[2] for e in got] == sorted(set(e[2] for e in got)) and sum(e[1] for e in got) == n_rec
            n += n_rec
    assert n > 10_000


# ---- file to file -------------------------------------------------------------------------------------------------------------------------
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
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("csi_files")
    out = {}
    rng = np.random.default_rng(77)
    reference = {"chrA": rng.integers(1, 5, 60_000).astype(np.uint8)}
    out["one"] = _fixture_files(d, reference, W.wgbs_records(rng, reference["chrA"], 0, 12_000, het_every=400), "one")
    rng = np.random.default_rng(78)
    reference = {"chrA": rng.integers(1, 5, 200_000).astype(np.uint8), "chrB": rng.integers(1, 5, 9_000).astype(np.uint8),
                 "chrC": rng.integers(1, 5, 5_000).astype(np.uint8), "chrD": rng.integers(1, 5, 150_000).astype(np.uint8)}
    reference["chrB"][4_000:4_250] = 0
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 400, het_every=300) + W.wgbs_records(rng, reference["chrB"], 1, 400)
            + W.wgbs_records(rng, reference["chrD"], 3, 300))
    out["many"] = _fixture_files(d, reference, recs, "many")
    rng = np.random.default_rng(79)  # a header longer than a member: 1 500 contigs, records on three of them
    reference = {"contig_with_a_long_name_%04d" % i: rng.integers(1, 5, 400).astype(np.uint8) for i in range(1500)}
    names = list(reference)
    for i in (0, 700, 1499):
        reference[names[i]] = rng.integers(1, 5, 20_000 + i).astype(np.uint8)
    recs = sum((W.wgbs_records(rng, reference[names[i]], i, 300, het_every=300) for i in (0, 700, 1499)), [])
    out["wide"] = _fixture_files(d, reference, recs, "wide")
    return d, out


@pytest.mark.parametrize("fmt", ["bcf", "vcf"])
@pytest.mark.parametrize("name", ["one", "many", "wide"])
def test_bam2bcf_index(inputs, name, fmt):
    assert os.path.exists(EXE), "run `make demo`"
    d, files = inputs
    bam, fa, refs = files[name]
    opts = ["-O", "b"] + (["--format", "vcf"] if fmt == "vcf" else [])
    plain, idx = str(d / ("%s.%s.plain" % (name, fmt))), str(d / ("%s.%s.indexed" % (name, fmt)))
    r0 = subprocess.run([EXE] + opts + [bam, fa, plain, plain + ".json", "S9"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and not os.path.exists(plain + ".csi"), r0.stderr + r0.stdout
    r1 = subprocess.run([EXE] + opts + ["--index", bam, fa, idx, idx + ".json", "S9"], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr + r1.stdout
    blob = open(idx, "rb").read()
    assert blob == open(plain, "rb").read() and open(idx + ".json").read() == open(plain + ".json").read() and r1.stdout == r0.stdout
    csi = open(idx + ".csi", "rb").read()
    assert csi.endswith(vcf.BGZF_EOF)
    want = csi_ref.build(blob, 14)
    assert gzip.decompress(csi) == want
    parsed = csi_ref.parse(blob)
    data, names, recs = parsed
    blocks = int(r0.stdout.split()[0])
    assert names == [n for n, _ in refs] and len(recs) == int(r0.stdout.split()[2]) > 1000
    if name == "one":
        assert blocks == 1 and len(data) > 3 * M
    if name == "many":  # a window of 16 384 positions holds several blocks: its bin's one chunk spans them; one contig has no record
        assert blocks > 20 and not any(t == 2 for t, *_ in recs)
    if name == "wide":  # no record lies in member 0
        assert recs[0][2] > M
    ix = vcf.read_csi(idx + ".csi")
    assert ix["min_shift"] == 14 and len(ix["refs"]) == len(refs) and (ix["names"] == names) == (fmt == "vcf")
    rng = np.random.default_rng(5)
    used = sorted(set(t for t, *_ in recs))
    some = [refs[t] for t in used] + [r for r in refs if refs.index(r) not in used][:1]
    n_hit = 0
    for cname, a, b in csi_ref.sweep(some, 14, rng):
        got = vcf.fetch(idx, cname, a, b, index=ix)
        assert got == csi_ref.linear(parsed, cname, a, b), (cname, a, b)
        n_hit += bool(got)
    assert n_hit > 50
