"""The CSI index without a GPU: bsc_csi_add / bsc_csi_finish fed with entries and member sizes computed in Python from files the host
writers wrote (vcf.write_bcf / write_vcf), against tests/csi_ref.py's index of the same file; vcf.read_csi / csi_chunks / fetch against a
linear scan; the record walk of the device scan (csrc/csidev_core.h) as a stand-alone host program under AddressSanitizer +
UndefinedBehaviorSanitizer over crafted and damaged streams; the error returns."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import csi_ref
import test_bcf as TB
from bs_call_amd import _lib, vcf
from bs_call_amd.abi import VCF_REC
from bs_call_amd.caller import CSI_BCF, CSI_ENTRY, CSI_VCF, BscError, CsiIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTIGS = [("chrA", 200_000), ("chrEmpty", 5_000), ("c", 70_000), ("chrLast", 40_000)]
M = 0xFF00


def _recs(rng, positions):
    recs = np.zeros(len(positions), dtype=VCF_REC)
    for i, p in enumerate(positions):
        recs[i] = TB._random_rec(rng)
        recs[i]["core"]["pos"] = p
        recs[i]["core"]["emit"] = 1
    return recs


def _positions(rng, length, n):
    """1-based positions: random ones, and every window edge of min_shift 14 and 7 nearby (0-based 2^k - 1 and 2^k)."""
    edges = [e for k in (7, 14, 15, 16, 17) for e in ((1 << k), (1 << k) + 1) if e <= length]
    pos = set(int(v) for v in rng.integers(1, length + 1, n)) | set(edges) | {1, length}
    return sorted(pos)


@pytest.fixture(scope="module")
def blocks():
    """[(tid, VCF_REC[])] in file order: several blocks a contig, cut at arbitrary records — so inside windows —, one contig without records."""
    rng = np.random.default_rng(20261019)
    out = []
    for tid, (_, ln) in enumerate(CONTIGS):
        if tid == 1:
            continue
        recs = _recs(rng, _positions(rng, ln, 2000 if tid == 0 else 300))
        cuts = [0] + sorted(int(v) for v in rng.choice(np.arange(1, len(recs)), 3, replace=False)) + [len(recs)]
        out += [(tid, recs[a:b]) for a, b in zip(cuts, cuts[1:])]
    return out


@pytest.fixture(scope="module")
def files(blocks, tmp_path_factory):
    """{"bcf" | "vcf": (path, blob, header bytes, [(tid, block stream)])}"""
    d = tmp_path_factory.mktemp("csi_host")
    header = vcf.header_text(CONTIGS, "S1", benchmark_mode=True)
    out = {}
    streams = [(tid, vcf.bcf_block(r, tid)) for tid, r in blocks]
    p = str(d / "f.bcf")
    vcf.write_bcf(p, header, [s for _, s in streams], compressed=True)
    out["bcf"] = (p, open(p, "rb").read(), 9 + len(header.encode()) + 1, streams)
    lines = [(tid, vcf.format_records_c(r, CONTIGS[tid][0])) for tid, r in blocks]
    p = str(d / "f.vcf.gz")
    vcf.write_vcf(p, header, [l for _, l in lines], bgzip=True)
    out["vcf"] = (p, open(p, "rb").read(), len(header.encode()), [(tid, ("\n".join(l) + "\n").encode()) for tid, l in lines])
    return out


def _index_bytes(fmt, blob, header_bytes, streams, min_shift, rng):
    """The .csi bytes bsc_csi_* make of Python-computed entries (cut at random record starts, as the scan's intervals cut them) and sizes."""
    pieces = 0
    with CsiIndex(None, CSI_BCF if fmt == "bcf" else CSI_VCF, CONTIGS, min_shift, header_bytes) as ix:
        for tid, s in streams:
            starts = [e[2] for e in csi_ref.entries_of(s, fmt, 0)]  # min_shift 0: (nearly) every record starts a run
            cuts = [int(v) for v in rng.choice(starts, min(len(starts), 7), replace=False)]
            ent = csi_ref.entries_of(s, fmt, min_shift, sync=cuts)
            pieces += len(ent) - len(csi_ref.merged(ent))
            ix.add(tid, np.array(ent, dtype=CSI_ENTRY), len(s))
        assert pieces > 0 or min_shift < 14  # some runs do come in pieces
        ix.members(csi_ref.member_sizes(blob))
        return ix.finish()


@pytest.mark.parametrize("fmt", ["bcf", "vcf"])
@pytest.mark.parametrize("min_shift", [14, 5])
def test_finish_equals_the_python_index(files, fmt, min_shift):
    _, blob, header_bytes, streams = files[fmt]
    assert csi_ref.inflate(blob)[header_bytes:] == b"".join(s for _, s in streams)
    csi = _index_bytes(fmt, blob, header_bytes, streams, min_shift, np.random.default_rng(3))
    assert csi.endswith(vcf.BGZF_EOF) and all(len(d) == M for _, d in csi_ref.members(csi)[:-2])
    want = csi_ref.build(blob, min_shift)
    assert gzip.decompress(csi) == want
    assert len(want) > (M if min_shift == 5 else 200)  # at min_shift 5 the index itself spans more than one member


@pytest.mark.parametrize("fmt", ["bcf", "vcf"])
def test_fetch_equals_the_linear_scan(files, fmt):
    path, blob, header_bytes, streams = files[fmt]
    rng = np.random.default_rng(4)
    with open(path + ".csi", "wb") as f:
        f.write(_index_bytes(fmt, blob, header_bytes, streams, 14, rng))
    ix = vcf.read_csi(path + ".csi")
    assert ix["min_shift"] == 14 and ix["depth"] == csi_ref.depth_of(14, [l for _, l in CONTIGS]) and len(ix["refs"]) == len(CONTIGS)
    assert ix["refs"][1] == {} and (ix["names"] == [n for n, _ in CONTIGS]) == (fmt == "vcf")
    parsed = csi_ref.parse(blob)
    n_hit = 0
    for name, a, b in csi_ref.sweep(CONTIGS, 14, rng) + [("nope", 0, 10), ("chrEmpty", 0, 5000)]:
        got = vcf.fetch(path, name, a, b, index=ix)
        assert got == csi_ref.linear(parsed, name, a, b), (name, a, b)
        n_hit += bool(got)
    assert n_hit > 100
    assert vcf.fetch(path, 2, 0, 70_000) == csi_ref.linear(parsed, "c", 0, 70_000)  # by contig number, index from path + ".csi"
    # a query reads its chunks, not the file: the chunks of one window are a small part of it
    ch = vcf.csi_chunks(ix, 0, 3 << 14, 4 << 14)
    assert len(ch) == 1 and (ch[0][1] >> 16) - (ch[0][0] >> 16) < len(blob) // 4


def test_reg2bins_and_chunk_rules():
    assert vcf.csi_reg2bins(0, 1, 14, 2) == [0, 1, 9] and vcf.csi_reg2bins(0, 1 << 20, 14, 2) == [0] + list(range(1, 9)) + list(range(9, 73))
    assert vcf.csi_reg2bins((1 << 14) - 1, (1 << 14) + 1, 14, 1) == [0, 1, 2] and vcf.csi_reg2bins(5, 5, 14, 1) == []
    ix = {"min_shift": 14, "depth": 1, "refs": [{1: (100, [(100, 200)]), 3: (300, [(300, 400)]), 4: (400, [(400, 500)]), 0: (50, [(50, 350)]), 10: (0, [(100, 500), (5, 0)])}]}
    assert vcf.csi_chunks(ix, 0, 0, 1 << 14) == [(50, 350)]  # the leaf's loffset 100 keeps the parent's chunk; the two overlap: merged
    assert vcf.csi_chunks(ix, 0, 1 << 14, 2 << 14) == [(50, 350)]  # leaf 2 is missing: the previous sibling's loffset, 100
    assert vcf.csi_chunks(ix, 0, 2 << 14, 4 << 14) == [(50, 500)]  # loffset 300: the parent's chunk (it ends at 350) stays, overlapping and adjacent chunks merge
    assert vcf.csi_chunks(ix, 0, 3 << 14, 4 << 14) == [(400, 500)]  # loffset 400 drops the parent's chunk
    assert vcf.csi_chunks(ix, 1, 0, 100) == [] and vcf.csi_chunks(ix, 0, 9, 9) == []


# ---- the record walk on the CPU, under the sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("csi_walk") / "csi_walk_host")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "bs_call_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csidev", "csi_walk_host.c"), "-o", out], check=True)
    return out


def _walk(exe, tmp_path, fmt, min_shift, stream, sync, cap=1 << 20):
    sp, op = str(tmp_path / "s.bin"), str(tmp_path / "o.txt")
    open(sp, "wb").write(stream)
    if sync is not None:
        open(op, "w").write("".join("%d\n" % v for v in sync))
    p = subprocess.run([exe, fmt, str(min_shift), str(cap), sp, op if sync is not None else "-"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = p.stdout.split("\n")[:-1]
    tail = lines[-1].split()
    return [tuple(int(v) for v in l.split()) for l in lines[:-1]], int(tail[1]), int(tail[3]), int(tail[5])


def _sync_of(stream, fmt, rng, k):
    """k interval boundaries at record starts, with empty intervals at the start, in the middle and at the end."""
    starts = [e[2] for e in csi_ref.entries_of(stream, fmt, 0)]
    cuts = sorted(int(v) for v in rng.choice(starts[1:], min(k, len(starts) - 1), replace=False)) if len(starts) > 1 else []
    mid = cuts[len(cuts) // 2 : len(cuts) // 2 + 1]
    return [0, 0, 0] + cuts[: len(cuts) // 2] + mid + mid + cuts[len(cuts) // 2 :] + [len(stream)] * 3


@pytest.mark.parametrize("fmt", ["bcf", "vcf"])
def test_walk_of_whole_streams(exe, files, tmp_path, fmt):
    rng = np.random.default_rng(6)
    stream = files[fmt][3][0][1]
    n_rec = len(csi_ref.entries_of(stream, fmt, 0))
    for min_shift in (5, 6, 7, 14):
        sync = _sync_of(stream, fmt, rng, 40)
        want = csi_ref.entries_of(stream, fmt, min_shift, sync=sync)
        assert _walk(exe, tmp_path, fmt, min_shift, stream, sync) == (want, len(want), n_rec, 0)
    want = csi_ref.entries_of(stream, fmt, 14)
    assert _walk(exe, tmp_path, fmt, 14, stream, None) == (want, len(want), n_rec, 0)
    assert len(want) >= 2
    assert _walk(exe, tmp_path, fmt, 14, stream, None, cap=len(want) - 1) == (want[:-1], len(want), n_rec, 0)  # one too small
    assert _walk(exe, tmp_path, fmt, 14, b"", [0, 0]) == ([], 0, 0, 0) and _walk(exe, tmp_path, fmt, 14, b"", None) == ([], 0, 0, 0)


def test_walk_of_damaged_streams(exe, files, tmp_path):
    stream = files["bcf"][3][0][1]
    starts = [e[2] for e in csi_ref.entries_of(stream, "bcf", 0)]
    k = starts[5]
    for bad_shared in (0xFFFFFFF0, 5, struct.unpack_from("<I", stream, k)[0] + 1):  # beyond the stream, below the fixed fields, off by one at the end
        cut = stream[: starts[6]] if bad_shared < 1000 and bad_shared > 5 else stream
        s = cut[:k] + struct.pack("<I", bad_shared) + cut[k + 4 :]
        ent, n, recs, err = _walk(exe, tmp_path, "bcf", 14, s, None)
        assert err == 1 and recs == 5 and ent == csi_ref.entries_of(stream[:k], "bcf", 14)
    assert _walk(exe, tmp_path, "bcf", 14, stream[: starts[6] - 1], None)[2:] == (5, 1)  # the stream ends inside a record
    assert _walk(exe, tmp_path, "bcf", 14, stream[:20], None)[2:] == (0, 1)
    back = stream[starts[3] : starts[4]] + stream[starts[1] : starts[2]]
    assert _walk(exe, tmp_path, "bcf", 14, back, None)[2:] == (1, 2)  # a position that goes backwards
    assert _walk(exe, tmp_path, "bcf", 14, stream, [0, starts[3], starts[2], len(stream)])[3] & 8  # offsets that descend
    assert _walk(exe, tmp_path, "bcf", 14, stream, [0, len(stream) + 1])[3] == 8
    text = files["vcf"][3][0][1]
    assert _walk(exe, tmp_path, "vcf", 14, text[:-1], None)[3] == 1  # no newline at the end
    for bad, err in ((b"chrA 12 . A\n", 4), (b"chrA\tx12\t.\n", 4), (b"chrA\t0\t.\n", 4), (b"chrA\t4294967296\t.\n", 4), (b"chrA\t123456789012\t.\n", 4), (b"\n", 4),
                     (b"chrA\t12", 1), (b"chrA", 1), (b"chrA\t12\n", 4)):
        assert _walk(exe, tmp_path, "vcf", 14, text + bad + (text if err == 4 else b""), None)[3] == err, bad  # (1: the stream ends inside the line)
    ok = b"c\t1\t.\n" + b"c\t999999999\t.\tA\n" + b"c\t4294967295\t.\n"
    assert _walk(exe, tmp_path, "vcf", 14, ok, None) == ([(0, 1, 0), (999999998 >> 14, 1, 6), (4294967294 >> 14, 1, 22)], 3, 3, 0)
    long_name = b"N" * 255 + b"\t16384\t.\n" + b"N" * 255 + b"\t16385\t.\n"
    assert _walk(exe, tmp_path, "vcf", 14, long_name, None) == ([(0, 1, 0), (1, 1, 264)], 2, 2, 0)


# ---- the error returns ----------------------------------------------------------------------------------------------------------------
def test_errors():
    L = _lib.load()
    names = (C.c_char_p * 2)(b"a", b"b")
    lens = (C.c_uint32 * 2)(100_000, 50_000)
    h = C.c_void_p()
    assert L.bsc_csi_open(None, 0, 14, 2, names, lens, C.byref(h)) == -1 and b"not an open BGZF writer" in L.bsc_last_error()
    assert L.bsc_bgzf_tell(None, None, None) == -1
    assert L.bsc_csi_open_detached(0, 14, 2, names, lens, 100, None) == -1
    assert L.bsc_csi_open_detached(2, 14, 2, names, lens, 100, C.byref(h)) == -1
    assert L.bsc_csi_open_detached(0, 0, 2, names, lens, 100, C.byref(h)) == -1 and L.bsc_csi_open_detached(0, 32, 2, names, lens, 100, C.byref(h)) == -1
    assert L.bsc_csi_open_detached(0, 14, 2, None, lens, 100, C.byref(h)) == -1
    assert L.bsc_csi_add(None, 0, None, 0, 0) == -1 and L.bsc_csi_finish(None, None, 0) == -1 and L.bsc_csi_members(None, None, 0) == -1
    L.bsc_csi_close(None)
    assert L.bsc_csi_open_detached(0, 14, 2, names, lens, 100, C.byref(h)) == 0

    def add(tid, ent, n_bytes):
        e = np.array(ent, dtype=CSI_ENTRY)
        return L.bsc_csi_add(h, tid, e.ctypes.data_as(C.c_void_p) if len(e) else None, len(e), n_bytes)

    assert L.bsc_csi_finish(h, None, 0) == -1 and b"not closed yet" in L.bsc_last_error()  # finish before the file is closed
    assert add(2, [(0, 1, 0)], 50) == -1 and add(-1, [(0, 1, 0)], 50) == -1
    assert add(0, [(0, 1, 0)], 0) == -1 and add(0, [], 50) == -1 and L.bsc_csi_add(h, 0, None, 1, 50) == -1
    assert add(0, [(1, 1, 0), (0, 1, 10)], 50) == -1 and b"out of order" in L.bsc_last_error()  # windows descend
    assert add(0, [(0, 1, 0), (1, 1, 0)], 50) == -1 and add(0, [(0, 1, 4)], 50) == -1 and add(0, [(0, 1, 0), (1, 1, 50)], 50) == -1
    assert add(0, [(0, 0, 0)], 50) == -1 and add(0, [(8, 1, 0)], 50) == -1  # no records; a window beyond the levels (depth 1: 8 windows)
    assert add(0, [(2, 3, 0), (3, 1, 30)], 50) == 0
    assert add(0, [(2, 1, 0)], 50) == -1 and b"out of order" in L.bsc_last_error()  # behind the contig's last window
    assert add(1, [(0, 1, 0)], 20) == 0
    assert add(0, [(5, 1, 0)], 20) == -1 and b"out of order" in L.bsc_last_error()  # contigs descend
    assert add(1, [], 0) == 0
    sizes = (C.c_uint64 * 2)(60, 60)
    assert L.bsc_csi_members(h, sizes, 2) == -1 and L.bsc_csi_members(h, None, 1) == -1  # 170 bytes are one member
    assert L.bsc_csi_members(h, sizes, 1) == 0 and L.bsc_csi_members(h, sizes, 1) == -1
    assert add(1, [(1, 1, 0)], 20) == -1 and b"closed" in L.bsc_last_error()
    need = L.bsc_csi_finish(h, None, 0)
    buf = np.full(need + 8, 0xEE, np.uint8)
    assert need > 28 and L.bsc_csi_finish(h, None, 5) == -1
    assert L.bsc_csi_finish(h, buf.ctypes.data_as(C.c_void_p), need - 1) == need and (buf == 0xEE).all()  # too small: nothing written
    assert L.bsc_csi_finish(h, buf.ctypes.data_as(C.c_void_p), need) == need and (buf[need:] == 0xEE).all()
    raw = gzip.decompress(buf[:need].tobytes())
    v = lambda u: u  # one member at file offset 0: the virtual offset is the offset
    want = (b"CSI\x01" + struct.pack("<iiii", 14, 1, 0, 2)
            + struct.pack("<i", 3) + struct.pack("<IQiQQ", 1 + 2, v(100), 1, v(100), v(130)) + struct.pack("<IQiQQ", 1 + 3, v(130), 1, v(130), v(150))
            + struct.pack("<IQiQQQQ", 10, 0, 2, v(100), v(150), 4, 0)
            + struct.pack("<i", 2) + struct.pack("<IQiQQ", 1, v(150), 1, v(150), v(170)) + struct.pack("<IQiQQQQ", 10, 0, 2, v(150), v(170), 1, 0) + struct.pack("<Q", 0))
    assert raw == want
    L.bsc_csi_close(h)
    assert L.bsc_csi_finish(h, None, 0) == -1 and L.bsc_csi_add(h, 0, None, 0, 0) == -1  # a closed index
    with pytest.raises(BscError):
        CsiIndex(None, 7, CONTIGS)


def test_bam2bcf_refuses_index_without_a_compressed_single_run(tmp_path):
    exe = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
    assert os.path.exists(exe), "run `make demo`"
    args = ["in.bam", "ref.fa", str(tmp_path / "o.bcf"), str(tmp_path / "o.json")]
    env = {k: v for k, v in os.environ.items() if not k.startswith("BAM2BCF_HOST")}
    for opts, extra, word in ((["--index"], {}, "-O b"), (["--index", "-O", "u"], {}, "-O b"), (["-O", "b", "--index", "--rank", "0", "--world", "2"], {}, "--rank"),
                              (["--index", "-O", "b", "--merge", "2"], {}, "--merge"), (["-O", "b", "--index"], {"BAM2BCF_HOST_READER": "1"}, "BAM2BCF_HOST_READER"),
                              (["--format", "vcf", "-O", "b", "--index"], {"BAM2BCF_HOST_BCF": "1"}, "BAM2BCF_HOST")):
        p = subprocess.run([exe] + opts + args, capture_output=True, text=True, timeout=60, env=dict(env, **extra))
        assert p.returncode == 2 and word in p.stderr and not os.path.exists(tmp_path / "o.bcf"), (opts, p.stderr)
