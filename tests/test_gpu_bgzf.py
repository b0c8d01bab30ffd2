"""BGZF on the device (csrc/bgzfdev.hip, bsc_bgzf_*): members cut at every 0xFF00 bytes of the logical stream, each a valid gzip member
with the 'BC' field, its CRC-32 and ISIZE; decoded by zlib, by gzip over the whole file and by the library's own inflater; the same
members as the host writer (vcf.write_bcf), the same bytes however the writes are split, a ratio next to zlib level 1, and bam2bcf -O b."""
import ctypes as C
import gzip
import importlib.util
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import bs_call_amd as B
from bs_call_amd import _lib, vcf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
M = 0xFF00
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)


def members(blob):
    """[(bsize, deflate payload, crc, isize)] of a BGZF file; checks every header and that the file ends with the EOF marker."""
    assert blob.endswith(vcf.BGZF_EOF)
    out, at = [], 0
    while at < len(blob):
        hdr = blob[at : at + 18]
        assert hdr[:4] == b"\x1f\x8b\x08\x04" and hdr[10:16] == b"\x06\x00BC\x02\x00", hdr
        bsize = struct.unpack("<H", hdr[16:18])[0] + 1
        assert at + bsize <= len(blob) and bsize <= 65536
        crc, isize = struct.unpack("<II", blob[at + bsize - 8 : at + bsize])
        out.append((bsize, blob[at + 18 : at + bsize - 8], crc, isize))
        at += bsize
    assert at == len(blob) and out[-1][0] == 28 and out[-1][3] == 0
    return out[:-1]


def inflate_own(payload, n):
    L = _lib.load()
    out = np.zeros(max(n, 1), np.uint8)
    src = np.frombuffer(payload, np.uint8) if payload else np.zeros(1, np.uint8)
    rc = L.bsc_inflate_raw(src.ctypes.data_as(C.c_void_p), len(payload), out.ctypes.data_as(C.c_void_p), n)
    assert rc == 0
    return out[:n].tobytes()


def check_bgzf(blob, data):
    """Decode `blob` three ways and check it against `data` and the format contract."""
    ms = members(blob)
    assert len(ms) == (len(data) + M - 1) // M
    for k, (bsize, payload, crc, isize) in enumerate(ms):
        want = data[k * M : (k + 1) * M]
        assert isize == len(want) and crc == zlib.crc32(want)
        assert zlib.decompress(payload, -15) == want
        assert inflate_own(payload, isize) == want
    assert gzip.GzipFile(fileobj=io.BytesIO(blob)).read() == data
    return ms


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


@pytest.fixture(scope="module")
def bcf_stream(caller):
    """A real BCF record stream from the device encoder: 30x synthetic reads, ~10+ MB."""
    seed = 424242
    tpl, seq = B.synth_reads_host(seed, 5_000, 220_000, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    ref = B.synth_ref_host(seed, x, y - x + 3)
    blob, n = caller.block_bcf(tpl, seq, x, y, ref, 0)
    assert n > 50_000
    return bytes(blob)


def dev_compress(caller, data, pieces=None, device=None, take_every=1):
    """Compress through the writer: `pieces` lengths (the rest in one write); device[i] True sends piece i from a device tensor."""
    z = caller.bgzf()
    parts, at = [], 0
    pieces = list(pieces or []) + [len(data) - sum(pieces or [])]
    keep = []
    for i, k in enumerate(pieces):
        chunk = data[at : at + k]
        at += k
        if device is not None and device[i % len(device)] and k:
            t = torch.frombuffer(bytearray(chunk), dtype=torch.uint8).to("cuda")
            torch.cuda.synchronize()
            z.write_device(t.data_ptr(), k)
            keep.append(t)
        else:
            z.write(chunk)
        if i % take_every == 0:
            parts.append(z.take())
    parts.append(z.close())
    return b"".join(parts)


CRAFTED = {
    "empty": b"",
    "one": b"\x07",
    "m-1": bytes(np.random.default_rng(1).integers(0, 4, M - 1, dtype=np.uint8) + 65),
    "m": bytes(np.random.default_rng(2).integers(0, 4, M, dtype=np.uint8) + 65),
    "m+1": bytes(np.random.default_rng(3).integers(0, 4, M + 1, dtype=np.uint8) + 65),
    "3m": bytes(np.random.default_rng(4).integers(0, 16, 3 * M, dtype=np.uint8) + 48),
    "zeros": bytes(1_000_000),
    "random": np.random.default_rng(5).integers(0, 256, 1_000_000, dtype=np.uint8).tobytes(),
    "period3": b"abc" * 333_333,
    # byte k (k < 22) fib(k + 1) times, shuffled: an unlimited Huffman code would be 21 bits deep — the 15-bit limit at work
    "skewed": np.random.default_rng(6).permutation(np.repeat(np.arange(22, dtype=np.uint8), [int(round(1.618034 ** (k + 1) / 5 ** 0.5)) for k in range(22)])).tobytes(),
    "text": b"".join(b"chr1\t%d\t.\tA\tC\t%d\tPASS\tDP=%d\n" % (i, i % 97, i % 31) for i in range(40_000)),
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_round_trip_on_crafted_streams(caller, name):
    data = CRAFTED[name]
    blob = dev_compress(caller, data)
    ms = check_bgzf(blob, data)
    if name == "empty":
        assert blob == vcf.BGZF_EOF
    if name == "random":
        assert all(b <= 65536 for b, *_ in ms)
        assert all(p[0] & 7 == 1 for _, p, _, _ in ms)  # stored
    if name in ("zeros", "period3"):
        assert all(p[0] & 7 == 5 for _, p, _, _ in ms)  # final, dynamic Huffman
        assert len(blob) < len(data) // 50


def test_round_trip_on_a_device_bcf_stream(caller, bcf_stream):
    t = torch.frombuffer(bytearray(bcf_stream), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    z = caller.bgzf()
    z.write_device(t.data_ptr(), len(bcf_stream))
    blob = z.take() + z.close()
    ms = check_bgzf(blob, bcf_stream)
    assert all(p[0] & 7 == 5 for _, p, _, _ in ms)


def test_same_members_as_the_host_writer(caller, bcf_stream, tmp_path):
    header = vcf.header_text([("chrS", 300_000)], "S1", benchmark_mode=True)
    pu, pc = str(tmp_path / "u.bcf"), str(tmp_path / "c.bcf")
    vcf.write_bcf(pu, header, [bcf_stream[:1_000_003], bcf_stream[1_000_003:]], compressed=False)
    vcf.write_bcf(pc, header, [bcf_stream], compressed=True)
    data = open(pu, "rb").read()
    host = members(open(pc, "rb").read())
    dev = check_bgzf(dev_compress(caller, data), data)
    assert len(dev) == len(host)
    assert [(c, i) for _, _, c, i in dev] == [(c, i) for _, _, c, i in host]


def test_split_independence_and_determinism(caller, bcf_stream):
    data = bcf_stream[:3_000_000] + CRAFTED["zeros"][:100_000] + CRAFTED["random"][:200_000] + b"abc" * 50_000
    whole = dev_compress(caller, data)
    assert dev_compress(caller, data) == whole
    rng = np.random.default_rng(11)
    for trial in range(3):
        pieces = []
        left = len(data)
        while left > 0:
            k = int(rng.choice([0, 1, 2, int(rng.integers(3, 300)), int(rng.integers(300, 70_000)), int(rng.integers(70_000, 400_000))]))
            k = min(k, left)
            pieces.append(k)
            left -= k
        got = dev_compress(caller, data, pieces, device=[bool(v) for v in rng.integers(0, 2, 7)], take_every=int(rng.integers(1, 4)))
        assert got == whole, trial
    check_bgzf(whole, data)


def test_ratio_next_to_zlib_level_1(caller, bcf_stream):
    data = bcf_stream
    assert len(data) >= 10_000_000
    blob = dev_compress(caller, data)
    check_bgzf(blob, data)
    z1 = 28
    for k in range(0, len(data), M):
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += 18 + len(co.compress(data[k : k + M]) + co.flush()) + 8
    print("ratio: device %.3f, zlib 1 %.3f" % (len(data) / len(blob), len(data) / z1))
    assert len(blob) <= 1.05 * z1, (len(data) / len(blob), len(data) / z1)


def test_errors(caller):
    L = _lib.load()
    h = C.c_void_p()
    assert L.bsc_bgzf_open(None, C.byref(h)) == -1
    assert L.bsc_bgzf_open(caller._h, None) == -1
    assert L.bsc_bgzf_write(None, b"x", 1) == -1
    assert L.bsc_bgzf_write_device(None, None, 0) == -1
    d, n = C.c_void_p(), C.c_uint64()
    assert L.bsc_bgzf_take(None, C.byref(d), C.byref(n)) == -1
    assert L.bsc_bgzf_close(None, C.byref(d), C.byref(n)) == -1
    assert L.bsc_bgzf_open(caller._h, C.byref(h)) == 0
    assert L.bsc_bgzf_write(h, None, 5) == -1
    assert L.bsc_bgzf_write_device(h, None, 5) == -1
    assert L.bsc_bgzf_take(h, None, C.byref(n)) == -1
    assert L.bsc_bgzf_write(h, b"abc", 3) == 0
    assert L.bsc_bgzf_close(h, C.byref(d), C.byref(n)) == 0
    out = np.zeros(n.value, np.uint8)
    assert L.bsc_detached_read(caller._h, d, 0, n.value, out.ctypes.data_as(C.c_void_p)) == 0
    assert L.bsc_detached_wait(caller._h) == 0
    assert L.bsc_detached_free(caller._h, d) == 0
    assert gzip.decompress(out.tobytes()) == b"abc"
    assert L.bsc_bgzf_write(h, b"abc", 3) == -1  # after close
    assert b"not an open BGZF writer" in L.bsc_last_error()
    assert L.bsc_bgzf_write_device(h, None, 0) == -1
    assert L.bsc_bgzf_take(h, C.byref(d), C.byref(n)) == -1
    assert L.bsc_bgzf_close(h, C.byref(d), C.byref(n)) == -1


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


def _run_both(tmp_path, bam, fa, name):
    out_u, rep_u = str(tmp_path / (name + ".u.bcf")), str(tmp_path / (name + ".u.json"))
    out_b, rep_b = str(tmp_path / (name + ".b.bcf")), str(tmp_path / (name + ".b.json"))
    r = subprocess.run([EXE, bam, fa, out_u, rep_u, "S9"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    rb = subprocess.run([EXE, "-O", "b", bam, fa, out_b, rep_b, "S9"], capture_output=True, text=True, timeout=300)
    assert rb.returncode == 0, rb.stderr + rb.stdout
    plain, comp = open(out_u, "rb").read(), open(out_b, "rb").read()
    check_bgzf(comp, plain)
    assert open(rep_b).read() == open(rep_u).read() and rb.stdout == r.stdout
    ru = subprocess.run([EXE, "-O", "u", bam, fa, str(tmp_path / (name + ".u2.bcf")), str(tmp_path / (name + ".u2.json")), "S9"], capture_output=True,
                        text=True, timeout=300)
    assert ru.returncode == 0 and open(tmp_path / (name + ".u2.bcf"), "rb").read() == plain
    return int(r.stdout.split()[0]), len(plain)


def test_bam2bcf_compressed_one_contig_one_block(tmp_path):
    assert os.path.exists(EXE), "run `make demo`"
    rng = np.random.default_rng(77)
    reference = {"chrA": rng.integers(1, 5, 60_000).astype(np.uint8)}
    recs = W.wgbs_records(rng, reference["chrA"], 0, 12_000, het_every=400)
    bam, fa = _fixture_files(tmp_path, reference, recs, "one")
    blocks, n = _run_both(tmp_path, bam, fa, "one")
    assert blocks == 1 and n > 3 * M


def test_bam2bcf_compressed_many_contigs_many_blocks(tmp_path):
    assert os.path.exists(EXE), "run `make demo`"
    rng = np.random.default_rng(78)
    reference = {"chrA": rng.integers(1, 5, 200_000).astype(np.uint8), "chrB": rng.integers(1, 5, 9_000).astype(np.uint8),
                 "chrC": rng.integers(1, 5, 5_000).astype(np.uint8), "chrD": rng.integers(1, 5, 150_000).astype(np.uint8)}
    reference["chrB"][4_000:4_250] = 0
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 400, het_every=300) + W.wgbs_records(rng, reference["chrB"], 1, 400)
            + W.wgbs_records(rng, reference["chrD"], 3, 300))
    bam, fa = _fixture_files(tmp_path, reference, recs, "many")
    blocks, n = _run_both(tmp_path, bam, fa, "many")
    assert blocks > 20 and n > M
