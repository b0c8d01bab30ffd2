"""VCF text on the device (csrc/vcftextdev.hip, vcftext_emit.h, fmtg_dev.h): the number formatter against the C library's "%g" value by
value, the encoder against the host formatter (bsc_vcf_format_rec) and against a formatter written in plain Python here, both input forms,
capacity and errors, the stream through the BGZF writer, bam2bcf --format vcf and pipeline.run(text=True)."""
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
from bs_call_amd import _lib, pipeline, vcf
from bs_call_amd.abi import VCF_REC
from oracle import py_bcf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
M = 0xFF00
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
GT = ["AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT"]


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


# ---- 1. the number formatter ----------------------------------------------------------------------------------------------------------
def py_g(bits):
    """printf("%g") of the float with these bits, glibc's spelling of NaNs."""
    if (bits >> 23) & 255 == 255 and bits & 0x7FFFFF:
        return b"-nan" if bits >> 31 else b"nan"
    return ("%g" % struct.unpack("<f", struct.pack("<I", bits))[0]).encode()


def host_slots(bits):
    L = _lib.load()
    out = np.zeros((len(bits), 16), dtype=np.uint8)
    assert L.bsc_fmt_g(bits.ctypes.data, len(bits), out.ctypes.data) == 0
    return out


def device_slots(caller, bits):
    d_v = dev(bits)
    d_o = torch.zeros(len(bits) * 16, dtype=torch.uint8, device="cuda")
    caller.fmt_g_device(d_v.data_ptr(), len(bits), d_o.data_ptr())
    torch.cuda.synchronize()
    return d_o.cpu().numpy().reshape(-1, 16)


def compare_slots(caller, bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    got, want = device_slots(caller, bits), host_slots(bits)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(hex(int(bits[i])), bytes(want[i]), bytes(got[i])) for i in bad[:5]]
    return got


def test_fmt_g_sweep_every_exponent_both_signs(caller):
    """2^26 patterns: for each of the 512 sign / exponent fields 2^17 seeded mantissas (with the all-zeros and all-ones ones)."""
    rng = np.random.default_rng(7001)
    for chunk in range(8):
        se = np.arange(chunk * 64, chunk * 64 + 64, dtype=np.uint32)
        man = rng.integers(0, 1 << 23, (64, 1 << 17), dtype=np.uint64).astype(np.uint32)
        man[:, 0], man[:, 1], man[:, 2] = 0, 0x7FFFFF, 1
        compare_slots(caller, (se[:, None] << np.uint32(23) | man).reshape(-1))


def test_fmt_g_ties_switches_and_specials(caller):
    k = np.arange(100000, 1000000, dtype=np.float64)
    ties = np.concatenate([k + 0.5, 10 * k + 5]).astype(np.float32)
    assert (ties.astype(np.float64) == np.concatenate([k + 0.5, 10 * k + 5])).all()  # exact in float: real ties
    near = []
    for e in range(-45, 39):
        p = np.float32(10.0 ** e) if -45 <= e <= 38 else None
        for v in (p, np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(-np.inf))):
            near.append(v)
    for s in (1e-4, 1e6, 1e5, 999999.5, 9.999995e-5):
        p = np.float32(s)
        q = p
        for _ in range(4):
            q = np.nextafter(q, np.float32(np.inf))
            near.append(q)
        q = p
        for _ in range(4):
            q = np.nextafter(q, np.float32(-np.inf))
            near.append(q)
        near.append(p)
    special = np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 1, 0x80000001, 0x007FFFFF, 0x00800000,
                        0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)
    pos = np.concatenate([ties.view(np.uint32), np.array(near, dtype=np.float32).view(np.uint32), special])
    bits = np.concatenate([pos, pos ^ np.uint32(0x80000000)])
    got = compare_slots(caller, bits)
    text = {float(v): bytes(s[: s[15]]) for v, s in zip(bits[:5].view(np.float32), got[:5])}
    assert text[100000.5] == b"100000" and text[100001.5] == b"100002"
    one = compare_slots(caller, np.array([100000.5, 100001.5, 1000005.0, 1000015.0, 999999.5], dtype=np.float32).view(np.uint32))
    assert [bytes(s[: s[15]]) for s in one] == [b"100000", b"100002", b"1e+06", b"1.00002e+06", b"1e+06"]


def test_fmt_g_wave_shapes_and_python(caller):
    """Waves that are uniform, that hold one odd lane, that mix the fast path (1e-12 .. 1e6) with the slow ones; a 2^17 finite sample also
    against Python's %g."""
    rng = np.random.default_rng(7002)
    fast = (-rng.random(1 << 15) * 10.0 ** rng.integers(-4, 5, 1 << 15)).astype(np.float32).view(np.uint32)
    slow = rng.integers(0, 1 << 32, 1 << 15, dtype=np.uint64).astype(np.uint32)
    uniform = np.repeat(np.concatenate([fast[:256], slow[:256]]), 64)
    odd = np.repeat(fast[:512], 64)
    odd[17::64] = slow[:512]
    odd2 = np.repeat(slow[512:1024], 64)
    odd2[63::64] = fast[512:1024]
    mixed = np.stack([fast, slow], axis=1).reshape(-1)
    compare_slots(caller, np.concatenate([uniform, odd, odd2, mixed]))
    sample = np.concatenate([fast, slow, rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])
    got = compare_slots(caller, sample)
    for b, s in zip(sample.tolist(), got):
        assert bytes(s[: s[15]]) == py_g(b), hex(b)


# ---- 2. records ---------------------------------------------------------------------------------------------------------------------------
def c5(b):
    return b.split(b"\0")[0]


def py_line(raw, contig, name=None):
    """The line of one 128-byte record, in plain Python (csrc/vcf_format.c read once more)."""
    (pos, emit, gt, _rc, gt_enc, flt, phred, n_gl, cg, alt, cx_ref, cx_gt, fs, qd, dp, *rest) = struct.unpack("<I8B2s5s5siII6II8I8Bii2B14x", raw)
    gl, counts, qual, mq = rest[:6], rest[7:15], rest[15:23], rest[23]
    if not emit:
        return b""
    g = GT[gt] if gt < 10 else GT[0]
    het = g[0] != g[1]
    f = [contig, b"%d" % pos, name if name else b".", bytes([cx_ref[2]])]
    f.append((bytes([alt[0]]) + (b"," + bytes([alt[1]]) if alt[1] else b"")) if alt[0] else b".")
    f += [b"%d" % phred, b"PASS" if flt == 0 else (b"mac1" if flt & 128 else b"fail"), b"CX=" + c5(cx_ref)]
    amq = [q for q, c in zip(qual, counts) if c > 0]
    f.append(b"GT:FT:DP:MQ:GQ:QD:GL:MC8" + (b":AMQ" if amq else b"") + b":CS:CG:CX" + (b":FS" if het else b""))
    ft = next((nm for i, nm in enumerate((b"q20", b"qd2", b"fs60", b"mq40")) if flt >> i & 1), b"PASS")
    s = [b"%d/%d" % ((gt_enc >> 5) - 1, ((gt_enc & 15) >> 1) - 1), ft, b"%d" % dp, b"%d" % mq, b"%d" % phred, b"%d" % qd,
         b",".join(py_g(v) for v in gl[: min(n_gl, 6)]), b",".join(b"%d" % c for c in counts)]
    if amq:
        s.append(b",".join(b"%d" % q for q in amq))
    s += [((b"+" if "C" in g else b"") + (b"-" if "G" in g else b"")) or b"NA", bytes([cg]), c5(cx_gt)]
    if het:
        s.append(b"%d" % fs)
    return b"\t".join(f) + b"\t" + b":".join(s) + b"\n"


def host_lines(recs, contig, ids=None):
    L = _lib.load()
    buf = C.create_string_buffer(2048)
    out, base = [], recs.ctypes.data
    for i in range(len(recs)):
        n = L.bsc_vcf_format_rec(base + 128 * i, contig, None if ids is None else ids.get(i), buf, 2048)
        assert n >= 0
        out.append(buf.raw[:n] + b"\n" if n else b"")
    return out


def random_records(rng, n):
    """Every field over its whole type, with the shapes that matter mixed in."""
    raw = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    recs = raw.view(VCF_REC).reshape(-1)
    mode = rng.integers(0, 1 << 16, n)
    core = recs["core"]
    core["emit"] = np.where(mode & 1, 1, core["emit"])
    core["gt"] = np.where(mode & 2, core["gt"] % 10, core["gt"])
    core["n_gl"] = np.where(mode & 4, core["n_gl"] % 7, core["n_gl"])
    recs["counts"][(mode & 8) != 0] = 0
    small = (mode & 16) != 0
    recs["counts"][small] = rng.integers(0, 3, (int(small.sum()), 8)) * rng.integers(0, 90, (int(small.sum()), 8))
    recs["counts"][(mode & 32 != 0) & (mode & 64 != 0)] = 0xFFFFFFFF
    core["flt"] = np.where(mode & 128, 0, core["flt"])
    real = (mode & 256) != 0
    gl = core["gl"]
    gl[real] = (-rng.random((int(real.sum()), 6)) * 10.0 ** rng.integers(-4, 5, (int(real.sum()), 6))).astype(np.float32)
    gl[real & (mode & 512 != 0), 0] = 0.0
    core["gl"] = gl
    # runs of positions without a record, longer than a tile
    for s in range(100, n - 200, 1500):
        core["emit"][s : s + 150] = 0
    recs["core"] = core
    return recs


def names_table(rng, recs, lens=(0, 1, 5, 63, 64, 90)):
    """A table for about a third of the flagged records (and some positions no record has); ids: record index -> the name a host %s prints."""
    flagged = [i for i in range(len(recs)) if recs["rs_found"][i] and recs["core"]["emit"][i]]
    pick = {}
    for i in flagged[::3]:
        pick.setdefault(int(recs["core"]["pos"][i]), None)
    for p in rng.integers(0, 1 << 32, 50):
        pick.setdefault(int(p), None)
    pos = np.array(sorted(pick), dtype=np.uint32)
    off, by = [0], b""
    for k, p in enumerate(pos):
        l = lens[k % len(lens)]
        nm = bytes(rng.integers(97, 123, l, dtype=np.uint8))
        pick[int(p)] = nm[:63]
        by += nm
        off.append(len(by))
    ids = {i: pick[int(recs["core"]["pos"][i])] for i in range(len(recs)) if recs["rs_found"][i] and pick.get(int(recs["core"]["pos"][i]))}
    return (pos, np.array(off, dtype=np.uint32), by), ids


def encode_packed(caller, recs, contig, names=None, cap=None, n=None):
    d_recs = dev(recs) if len(recs) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_n = torch.tensor([len(recs) if n is None else n], dtype=torch.int64, device="cuda")
    cap = max(16, 700 * len(recs)) if cap is None else cap
    d_out = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(3, dtype=torch.int64, device="cuda")
    caller.vcf_text_block_device(d_recs.data_ptr(), d_n.data_ptr(), len(recs), contig, d_out.data_ptr(), cap, d_tot.data_ptr(), names=names)
    torch.cuda.synchronize()
    tot = [int(v) for v in d_tot.cpu()]
    out = d_out.cpu().numpy()
    assert (out[cap:] == 0xEE).all()  # nothing behind the room given
    return out[:cap], tot


@pytest.mark.parametrize("n,contig,with_names", [(0, b"c", False), (1, b"c", False), (63, b"chr1", True), (64, b"chr1", False), (65, b"7", True),
                                                 (5000, b"x" * 255, True), (300_000, b"chr12", True), (20_000, b"chrUn_KI270742v1", False)])
def test_packed_records_equal_the_host_lines(caller, n, contig, with_names):
    rng = np.random.default_rng(9000 + n)
    recs = random_records(rng, n) if n else np.zeros(0, dtype=VCF_REC)
    names, ids = names_table(rng, recs) if with_names and n else (None, None)
    out, tot = encode_packed(caller, recs, contig, names=names)
    want = host_lines(recs, contig, ids)
    stream = b"".join(want)
    assert tot[0] == len(stream) and tot[2] == sum(1 for w in want if w)
    assert tot[1] == int(((recs["core"]["emit"] != 0) & ((recs["core"]["gt"] > 9) | (recs["core"]["n_gl"] > 6))).sum())
    assert out[: tot[0]].tobytes() == stream
    if with_names and n:
        assert any(len(v) == 63 for v in ids.values()) and any(len(v) == 1 for v in ids.values())
    k = min(n, 3000)  # the plain-Python formatter on a part (it is slow)
    raw = recs.view(np.uint8).reshape(-1, 128)
    for i in range(k):
        assert py_line(raw[i].tobytes(), contig, None if ids is None else ids.get(i)) == want[i], i


def test_count_on_the_device_limits_the_records(caller):
    recs = random_records(np.random.default_rng(9100), 1000)
    out, tot = encode_packed(caller, recs, b"c", n=333)
    want = b"".join(host_lines(recs[:333], b"c"))
    assert tot[0] == len(want) and out[: tot[0]].tobytes() == want


# ---- 3. the per-position form behind the chain ---------------------------------------------------------------------------------------------
def test_tiles_of_the_longest_lines_go_out_in_four_parts(caller):
    """the wave's image is 12 KB: 32 lines of ~640 bytes do not fit it, 16 do — four parts of 16 lanes.  Every field at its widest: a 255-byte
    contig name, ten-digit positions, 63-byte names, six likelihoods of twelve characters, counts beyond 32 767, all four filter bits, two
    ALT alleles, a heterozygous call's FS; a stretch of short lines in between, so that the parts of one tile differ in what they hold."""
    n, contig = 200, b"k" * 255
    recs = np.zeros(n, dtype=VCF_REC)
    core = recs["core"]
    core["pos"] = 4_000_000_000 + 7 * np.arange(n, dtype=np.uint32)
    core["emit"] = 1
    core["gt"] = 1            # heterozygous: FS is written
    core["gt_enc"] = 0x24
    core["flt"] = 15          # q20 qd2 fs60 mq40
    core["phred"] = 255
    core["n_gl"] = 6
    core["cg"] = b"H"
    core["alt"] = b"CT"
    core["cx_ref"] = b"ACGTA"
    core["cx_gt"] = b"HHCGH"
    core["fs"] = -2_000_000_000
    core["qd"] = 4_000_000_000
    core["dp"] = 4_000_000_000
    core["gl"] = np.float32(-1.23457e-05)  # "-1.23457e-05"
    recs["core"] = core
    recs["mq"] = -2_000_000_000
    recs["counts"] = 4_000_000_000 + np.arange(8, dtype=np.uint32)
    recs["qual"] = 243
    recs["rs_found"] = 1
    short = slice(85, 115)
    recs["counts"][short] = 5
    recs["core"]["n_gl"][short] = 1
    recs["core"]["dp"][short] = 7
    recs["rs_found"][short] = 0
    rng = np.random.default_rng(4343)
    pos = recs["core"]["pos"].astype(np.uint32)  # every record listed: the longest name the encoder keeps, and longer ones (cut at 63)
    nm = [b"rs" + bytes(rng.choice(list(b"0123456789"), int(rng.integers(61, 90))).tolist()) for _ in pos]
    off = np.concatenate([[0], np.cumsum([len(x) for x in nm])]).astype(np.uint32)
    ids = {i: nm[i][:63] for i in range(n) if recs["rs_found"][i]}
    want = host_lines(recs, contig, ids)
    sizes = np.array([len(w) for w in want])
    assert sizes.max() <= 665 and sizes[:32].sum() > 12288 and sizes[:16].sum() <= 12288
    assert sizes[short].max() < 500 < sizes[:85].min()
    out, tot = encode_packed(caller, recs, contig, names=(pos, off, b"".join(nm)))
    assert tot == [int(sizes.sum()), 0, n] and out[: tot[0]].tobytes() == b"".join(want)


@pytest.fixture(scope="module")
def synth():
    seed = 424242
    tpl, seq = B.synth_reads_host(seed, 5_000, 220_000, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    return tpl, seq, x, y, B.synth_ref_host(seed, x, y - x + 3)


@pytest.mark.parametrize("kw", [{}, {"all_positions": True}, {"reg_start": 60_000, "reg_stop": 150_000}, {"dbsnp": True}])
def test_sites_form_on_the_chain_s_arrays(caller, synth, kw):
    tpl, seq, x, y, ref = synth
    n = y - x + 1
    kw = dict(kw)
    flags = None
    if kw.pop("dbsnp", False):
        flags = (np.random.default_rng(5).integers(0, 40, n) == 0).astype(np.uint8) * 3
    recs = caller.block_records(tpl, seq, x, y, ref, dbsnp=flags, **kw)
    names = ids = None
    if flags is not None:
        names, ids = names_table(np.random.default_rng(6), recs, lens=(4, 9, 63, 70))
        assert ids
    want = b"".join(host_lines(recs, b"chrS", ids))
    d_tpl, d_seq, d_ref = dev(tpl), dev(seq), dev(ref)
    d_db = None if flags is None else dev(flags)
    d_core = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_aux = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    caller.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core.data_ptr(), d_aux.data_ptr(),
                              d_dbsnp=None if d_db is None else d_db.data_ptr(), **kw)
    cap = len(want) + 4096
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(3, dtype=torch.int64, device="cuda")
    caller.vcf_text_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chrS", d_out.data_ptr(), cap, d_tot.data_ptr(), names=names)
    torch.cuda.synchronize()
    tot = [int(v) for v in d_tot.cpu()]
    assert tot == [len(want), 0, len(recs)] and len(recs) > 10_000
    assert d_out.cpu().numpy()[: tot[0]].tobytes() == want
    packed, tot2 = encode_packed(caller, recs, b"chrS", names=names)
    assert tot2[0] == len(want) and packed[: tot2[0]].tobytes() == want


# ---- 4. capacity and errors ---------------------------------------------------------------------------------------------------------------
def test_a_stream_longer_than_the_room_is_cut_at_a_tile(caller):
    recs = random_records(np.random.default_rng(9200), 4000)
    lines = host_lines(recs, b"chr3")
    full = b"".join(lines)
    cap = (len(full) // 2) & ~15
    out, tot = encode_packed(caller, recs, b"chr3", cap=cap)
    assert tot[0] == len(full) and tot[2] == sum(1 for w in lines if w)
    tiles = [sum(len(w) for w in lines[t : t + 64]) for t in range(0, len(lines), 64)]
    fit, at = 0, 0
    for t in tiles:  # every tile that fits whole is written, where it belongs
        if at + t <= cap:
            assert out[at : at + t].tobytes() == full[at : at + t]
            fit += 1
        at += t
    assert 0 < fit < len(tiles)


def test_errors_leave_the_context_usable(caller):
    L, h = caller._L, caller._h
    recs = random_records(np.random.default_rng(9300), 200)
    d_recs, d_n = dev(recs), torch.tensor([200], dtype=torch.int64, device="cuda")
    d_out = torch.zeros(200 * 700, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(3, dtype=torch.int64, device="cuda")
    A = (d_recs.data_ptr(), d_n.data_ptr(), 200)
    Z = (None, d_out.data_ptr(), d_out.numel(), d_tot.data_ptr(), None)
    want = b"".join(host_lines(recs, b"c"))
    few = np.array([1.5, -0.25, 1e10, 3e-7], dtype=np.float32).view(np.uint32)

    def refused(rc):
        """The call answered BSC_ERR_ARG, and the context works: both encoders' next good call gives the right bytes."""
        assert rc == -1
        out, tot = encode_packed(caller, recs, b"c")
        assert out[: tot[0]].tobytes() == want
        compare_slots(caller, few)

    for contig in (b"", b"a\tb", b"a\nb", b"y" * 256, None):
        refused(L.bsc_vcf_text_block_device(h, *A, contig, *Z))
        refused(L.bsc_vcf_text_sites_device(h, d_recs.data_ptr(), d_recs.data_ptr(), 100, contig, *Z))
    rc = L.bsc_vcf_text_block_device(h, *A, b"c", None, d_out.data_ptr() + 8, 1000, d_tot.data_ptr(), None)
    assert b"aligned" in L.bsc_last_error()
    refused(rc)
    refused(L.bsc_vcf_text_block_device(h, *A, b"c", None, None, 1000, d_tot.data_ptr(), None))
    refused(L.bsc_vcf_text_block_device(h, *A, b"c", None, d_out.data_ptr(), 1000, None, None))
    refused(L.bsc_vcf_text_block_device(h, None, d_n.data_ptr(), 200, b"c", *Z))
    refused(L.bsc_vcf_text_block_device(h, d_recs.data_ptr(), None, 200, b"c", *Z))
    refused(L.bsc_vcf_text_block_device(None, *A, b"c", *Z))
    refused(L.bsc_vcf_text_sites_device(h, None, d_recs.data_ptr(), 100, b"c", *Z))
    refused(L.bsc_fmt_g_device(h, None, 4, d_out.data_ptr(), None))
    refused(L.bsc_fmt_g_device(h, d_recs.data_ptr(), 4, d_out.data_ptr() + 4, None))
    refused(L.bsc_fmt_g_device(None, d_recs.data_ptr(), 4, d_out.data_ptr(), None))
    nb, nr = C.c_uint64(0), C.c_uint64(0)
    refused(L.bsc_block_vcf_rawdev_keep(h, None, 0, None, 0, None, 0, 0, None, 1, 10, None, None, None, 0, b"c", None, 100, C.byref(nb), C.byref(nr), None,
                                        None))
    refused(L.bsc_block_vcf_rawdev_keep(h, None, 0, None, 0, None, 0, 0, None, 1, 10, None, None, None, 0, b"", None, 100, C.byref(nb), C.byref(nr), None,
                                        None))


# ---- 5. through BGZF ------------------------------------------------------------------------------------------------------------------------
def test_a_text_stream_through_the_device_bgzf_writer(caller):
    recs = random_records(np.random.default_rng(9400), 8000)
    recs["core"]["emit"] = 1
    want = b"".join(host_lines(recs, b"chr5"))
    assert len(want) > 8 * M
    d_recs, d_n = dev(recs), torch.tensor([len(recs)], dtype=torch.int64, device="cuda")
    d_out = torch.zeros(len(want) + 64, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(3, dtype=torch.int64, device="cuda")
    caller.vcf_text_block_device(d_recs.data_ptr(), d_n.data_ptr(), len(recs), b"chr5", d_out.data_ptr(), len(want) + 64, d_tot.data_ptr())
    torch.cuda.synchronize()
    z, parts, at = caller.bgzf(), [], 0
    for k in (1, M - 1, 17, 3 * M + 5, 100_000):
        z.write_device(d_out.data_ptr() + at, k)
        at += k
        parts.append(z.take())
    z.write_device(d_out.data_ptr() + at, len(want) - at)
    parts.append(z.close())
    blob = b"".join(parts)
    assert gzip.decompress(blob) == want
    at, sizes = 0, []
    while at < len(blob):
        bsize = struct.unpack("<H", blob[at + 16 : at + 18])[0] + 1
        sizes.append(struct.unpack("<I", blob[at + bsize - 4 : at + bsize])[0])
        at += bsize
    assert sizes[-1] == 0 and all(s == M for s in sizes[:-2]) and 0 < sizes[-2] <= M


# ---- 6. bam2bcf --format vcf, 7. pipeline.run(text=True) ---------------------------------------------------------------------------------------
def _fixture_files(tmp_path, reference, recs, name):
    refs = [(k, len(v)) for k, v in reference.items()]
    bam, fa = str(tmp_path / (name + ".bam")), str(tmp_path / (name + ".fa"))
    W.write_bam(bam, refs, recs)
    with open(fa, "w") as f:
        for nm, codes in reference.items():
            f.write(">%s\n" % nm)
            s = "".join("NACGT"[c] for c in codes)
            for o in range(0, len(s), 60):
                f.write(s[o : o + 60] + "\n")
    return bam, fa


def line_of_bcf(d, contigs):
    """A decoded BCF record as its text line: the tie between the two formats that does not go through the library's formatter."""
    fmt, s = d["fmt"], []
    for k in d["fmt_order"]:
        v = fmt[k]
        if k == "GT":
            s.append(b"%d/%d" % ((v[0] >> 1) - 1, (v[1] >> 1) - 1))
        elif k == "GL":
            s.append(b",".join(("%g" % x).encode() for x in v))
        elif isinstance(v, (bytes, bytearray)):
            s.append(bytes(v).split(b"\0")[0])  # FT is "q20\0;qd2\0"-style: the text shows what stands before the first NUL
        else:
            s.append(b",".join(b"%d" % x for x in v))
    f = [contigs[d["rid"]].encode(), b"%d" % d["pos"], bytes(d["id"]) or b".", bytes(d["alleles"][0]),
         b",".join(bytes(a) for a in d["alleles"][1:]) or b".", b"%d" % int(d["qual"]), d["filter"][0].encode(), b"CX=" + bytes(d["info"]["CX"]).split(b"\0")[0],
         b":".join(k.encode() for k in d["fmt_order"])]
    return b"\t".join(f) + b"\t" + b":".join(s) + b"\n"


def bcf_lines(blob, contigs):
    assert blob[:5] == b"BCF\2\2"
    (lt,) = struct.unpack_from("<I", blob, 5)
    header, at, out = blob[9 : 9 + lt - 1], 9 + lt, []
    while at < len(blob):
        ls, li = struct.unpack_from("<II", blob, at)
        out.append(line_of_bcf(py_bcf.decode_record(blob[at : at + 8 + ls + li]), contigs))
        at += 8 + ls + li
    return header, out


def run_exe(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


def check_bam2bcf(tmp_path, reference, recs, name):
    assert os.path.exists(EXE), "run `make demo`"
    bam, fa = _fixture_files(tmp_path, reference, recs, name)
    p = lambda s: str(tmp_path / (name + s))
    before = run_exe(bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    plain_bcf = open(p(".u.bcf"), "rb").read()
    out_v = run_exe("--format", "vcf", bam, fa, p(".vcf"), p(".v.json"), "S9")
    out_z = run_exe("--format", "vcf", "-O", "b", bam, fa, p(".vcf.gz"), p(".z.json"), "S9")
    assert out_v == before and out_z == before and open(p(".v.json")).read() == open(p(".u.json")).read() == open(p(".z.json")).read()
    text = open(p(".vcf"), "rb").read()
    header, lines = bcf_lines(plain_bcf, list(reference))
    assert text == header + b"".join(lines)
    assert header.startswith(b"##fileformat=VCFv4.2\n") and header.endswith(b"\tFORMAT\tS9\n")
    comp = open(p(".vcf.gz"), "rb").read()
    assert comp.endswith(vcf.BGZF_EOF) and gzip.decompress(comp) == text
    run_exe(bam, fa, p(".u2.bcf"), p(".u2.json"), "S9")
    assert open(p(".u2.bcf"), "rb").read() == plain_bcf
    return int(before.split()[0]), text, bam


def test_bam2bcf_text_one_contig_one_block(tmp_path, caller):
    rng = np.random.default_rng(77)
    reference = {"chrA": rng.integers(1, 5, 60_000).astype(np.uint8)}
    recs = W.wgbs_records(rng, reference["chrA"], 0, 12_000, het_every=400)
    blocks, text, bam = check_bam2bcf(tmp_path, reference, recs, "one")
    assert blocks == 1 and len(text) > 3 * M
    # the same lines from the library's host formatter, on the packed records of the same block
    from bs_call_amd.bam import block_reference
    from bs_call_amd.bamdev import DeviceBamReader

    with DeviceBamReader(caller, bam) as rd:
        (blk,) = [(int(b.x), int(b.y), *rd.fetch(b)) for b in rd.device_blocks()]
    x, y, raw, seq, ms = blk
    precs, _ = caller.block_records_raw(raw, seq, ms, x, y, block_reference(reference["chrA"], x, y), reg_stop=60_000)
    lines = host_lines(precs, b"chrA")
    body = b"".join(lines)
    head = text[: len(text) - len(body)]
    assert len(lines) > 1000 and text == head + body and head.startswith(b"##fileformat=") and head.endswith(b"\tFORMAT\tS9\n")
    # pipeline.run(text=True) writes the same file
    for compressed in (False, True):
        out = str(tmp_path / ("pipe%d" % compressed))
        pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, text=True, compressed=compressed)
        got = open(out, "rb").read()
        if compressed:
            at, sizes = 0, []
            while at < len(got):
                bsize = struct.unpack("<H", got[at + 16 : at + 18])[0] + 1
                sizes.append(struct.unpack("<I", got[at + bsize - 4 : at + bsize])[0])
                at += bsize
            assert all(s == M for s in sizes[:-2]) and sizes[-1] == 0
            got = gzip.decompress(got)
        assert got == text
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, str(tmp_path / "no"), device_reader=True, text=True, shard_rank=0, shard_world=2)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, str(tmp_path / "no"), text=True)
    assert not os.path.exists(tmp_path / "no")


def test_bam2bcf_text_many_contigs_many_blocks(tmp_path):
    rng = np.random.default_rng(78)
    reference = {"chrA": rng.integers(1, 5, 200_000).astype(np.uint8), "chrB": rng.integers(1, 5, 9_000).astype(np.uint8),
                 "chrC": rng.integers(1, 5, 5_000).astype(np.uint8), "chrD": rng.integers(1, 5, 150_000).astype(np.uint8)}
    reference["chrB"][4_000:4_250] = 0
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 400, het_every=300) + W.wgbs_records(rng, reference["chrB"], 1, 400)
            + W.wgbs_records(rng, reference["chrD"], 3, 300))
    blocks, text, _ = check_bam2bcf(tmp_path, reference, recs, "many")
    assert blocks > 20 and len(text) > M


def test_block_entry_too_little_room_then_again_gives_the_text(caller, tmp_path):
    """bsc_block_vcf_rawdev_keep with too little room answers like the BCF form; bsc_block_bcf_again then runs the TEXT encoder."""
    from bs_call_amd.bam import block_reference
    from bs_call_amd.bamdev import DeviceBamReader

    rng = np.random.default_rng(79)
    reference = {"chrA": rng.integers(1, 5, 60_000).astype(np.uint8)}
    recs = W.wgbs_records(rng, reference["chrA"], 0, 12_000, het_every=400)
    bam, _ = _fixture_files(tmp_path, reference, recs, "again")
    with DeviceBamReader(caller, bam) as rd:
        for blk in rd.device_blocks():
            ref = block_reference(reference["chrA"], int(blk.x), int(blk.y))
            full, n_rec, _ = caller.block_vcf_rawdev(blk, ref, "chrA", reg_stop=60_000)
            from bs_call_amd.abi import PREP_PARAMS, PREP_STATS

            par = np.zeros(1, dtype=PREP_PARAMS)
            par["min_qual"][0] = 20
            vp = _lib.VcfParams(0, 1, 60_000)
            st = np.zeros(1, dtype=PREP_STATS)
            nb, nr = C.c_uint64(0), C.c_uint64(0)
            rc = caller._L.bsc_block_vcf_rawdev_keep(caller._h, blk.d_tpl, blk.nr, blk.d_seq, blk.seq_bytes, blk.d_misms, blk.n_misms, blk.ins_pad,
                                                     par.ctypes.data, int(blk.x), int(blk.y), ref.ctypes.data, None, C.byref(vp), 0, b"chrA", None, 4096,
                                                     C.byref(nb), C.byref(nr), st.ctypes.data, None)
            assert rc == -1 and nb.value == len(full)  # BSC_ERR_ARG and the room needed
            assert b"bsc_block_vcf" in caller._L.bsc_last_error() and b"out_cap is 4096" in caller._L.bsc_last_error()
            nb, nr = C.c_uint64(0), C.c_uint64(0)
            assert caller._L.bsc_block_bcf_again(caller._h, None, len(full) + 64, C.byref(nb), C.byref(nr)) == 0
            assert nb.value == len(full) and nr.value == n_rec
            out = np.zeros(len(full), np.uint8)
            assert caller._L.bsc_bcf_stream_read(caller._h, 0, len(full), out.ctypes.data) == 0
            caller.synchronize()
            assert out.tobytes() == full and full.startswith(b"chrA\t") and full.count(b"\n") == n_rec
            small, n2, _ = caller.block_vcf_rawdev(blk, ref, "chrA", reg_stop=60_000)  # default room, grown by itself when needed
            assert small == full and n2 == n_rec
            break
