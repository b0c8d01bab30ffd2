"""zlib streams of fixed-stride pieces on the device (csrc/zlibdev.hip: bsc_zlib_pieces_device), the block follow-up that deflates a block's
bigWig sections (bsc_block_bigwig_deflate) and the compressed track file to file (bam2bcf --meth-bigwig-compress,
pipeline.run(bigwig_compress=True)).  The checker is Python's zlib: every stream inflates — with its Adler-32 verified — to its piece.

The (S, sites) grid of the block level runs on dense random records through bsc_bigwig_sites_device and bsc_zlib_pieces_device at stride
24 + 8 S — the call bsc_block_bigwig_deflate makes: the block entry takes its arrays from a reader's block only, whose site count is what
the reads give.  The block entry itself runs on a reader's blocks with S chosen from each block's site count (sites = S - 1, S, S + 1, 2 S + 1).

The ratio (30x synthetic reads, 26 906 sites, S = 1024; measured on an MI355X, 2026-10-19): device 101 657 bytes, zlib level 1 99 343,
Z_HUFFMAN_ONLY 142 461 — 1.023 x level 1, inside the 1.05 the test asserts (profiles/bigwig_z.json has the matcher's knobs row by row)."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

import bs_call_amd as B
from bs_call_amd import bigwig, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from methregions_ref import random_records
from test_gpu_bigwig import EXE, _fixture_files, W, all_sites, kept_stream, run_exe

pytestmark = pytest.mark.gpu
GUARD = 0xA5
M = 0xFF00


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def guarded(n_bytes):
    return torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")


def zpieces(caller, data, piece, src_off=0, out_room=None, sizes_room=None):
    """bsc_zlib_pieces_device over `data` lying src_off bytes behind a 256-byte aligned address.  Returns (streams or None, sizes or None,
    totals): None where the room was too small — that the array is then untouched, and the guard bytes behind every room, are checked here."""
    n = len(data)
    n_pieces = -(-n // piece)
    src = torch.zeros(n + src_off + 16, dtype=torch.uint8, device="cuda")
    if n:
        src[src_off : src_off + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    out_room = n + 11 * n_pieces if out_room is None else out_room
    sizes_room = n_pieces if sizes_room is None else sizes_room
    out, sizes, tot = guarded(out_room), guarded(4 * sizes_room), guarded(16)
    torch.cuda.synchronize()
    caller.zlib_pieces_device(src.data_ptr() + src_off if n else None, n, piece, out.data_ptr() if out_room else None, out_room,
                              sizes.data_ptr() if sizes_room else None, sizes_room, tot.data_ptr())
    torch.cuda.synchronize()
    h_out, h_sizes, h_tot = out.cpu().numpy(), sizes.cpu().numpy(), tot.cpu().numpy()
    totals = [int(v) for v in h_tot[:16].view(np.uint64)]
    assert (h_tot[16:] == GUARD).all() and (h_out[out_room:] == GUARD).all() and (h_sizes[4 * sizes_room :] == GUARD).all(), "written behind a room"
    assert totals[1] == n_pieces
    if n_pieces > sizes_room:
        assert (h_sizes == GUARD).all(), "a room too small is not written at all"
        zs = None
    else:
        zs = h_sizes[: 4 * n_pieces].view(np.uint32).copy()
        assert int(zs.sum()) == totals[0]
    if totals[0] > out_room:
        assert (h_out == GUARD).all(), "a room too small is not written at all"
        return None, zs, totals
    assert (h_out[totals[0] : out_room] == GUARD).all(), "written behind the streams"
    blob = h_out[: totals[0]].tobytes()
    if zs is None:
        return blob, None, totals
    ends = np.cumsum(zs)
    return [blob[int(e - s) : int(e)] for s, e in zip(zs, ends)], zs, totals


def check_streams(streams, data, piece):
    """Every stream is the zlib stream of its piece: header, one final stored or dynamic block, Adler-32 (zlib verifies it), the size limit."""
    assert len(streams) == -(-len(data) // piece)
    kinds = []
    for k, s in enumerate(streams):
        want = data[k * piece : (k + 1) * piece]
        assert s[:2] == b"\x78\x9c" and s[2] & 1 == 1 and (s[2] >> 1) & 3 in (0, 2), (k, s[:3])
        assert len(s) <= len(want) + 11
        assert zlib.decompress(s) == want, k
        assert zlib.decompress(s[2:-4], -15) == want and int.from_bytes(s[-4:], "big") == zlib.adler32(want)
        kinds.append((s[2] >> 1) & 3)
    return kinds


def fib_skewed():
    """The 22-symbol Fibonacci-skewed bytes of tests/test_gpu_bgzf.py: an unlimited Huffman code would be 21 bits deep."""
    return np.random.default_rng(6).permutation(np.repeat(np.arange(22, dtype=np.uint8), [int(round(1.618034 ** (k + 1) / 5 ** 0.5)) for k in range(22)])).tobytes()


def source(name, n):
    if name == "zeros":
        return bytes(n)
    if name == "random":
        return np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8).tobytes()
    if name == "abc":
        return (b"abc" * (n // 3 + 1))[:n]
    if name == "period8":
        return (bytes([1, 2, 3, 4, 0x9A, 0x99, 0x99, 0x42]) * (n // 8 + 1))[:n]
    if name == "skewed":
        s = fib_skewed()
        return (s * (n // len(s) + 1))[:n]
    if name == "ff":
        return b"\xff" * n
    if name == "text":
        return b"".join(b"chr1\t%d\t.\tA\tC\t%d\tPASS\tDP=%d\n" % (i, i % 97, i % 31) for i in range(n // 20 + 1))[:n]
    raise KeyError(name)


SOURCES = ["zeros", "random", "abc", "period8", "skewed", "ff", "text"]
STRIDES = [1, 2, 3, 4, 5, 32, 255, 256, 257, 8216, M - 1, M]


# ---- 1. the pieces round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", STRIDES)
def test_strides_with_every_kind_of_last_piece(caller, piece):
    rng = np.random.default_rng(9000 + piece)
    pool = source("text", 3 * M) if piece % 2 else bytes((rng.integers(0, 4, 3 * M, dtype=np.uint8) * 37 + 11).astype(np.uint8))
    for last in sorted({1, piece, max(piece - 1, 1)}):  # the last piece is 1 byte, is full, is full - 1
        data = pool[: 2 * piece + last]
        for off in ((0, 1, 2, 3) if last == 1 else (piece % 4,)):
            streams, zs, tot = zpieces(caller, data, piece, off)
            check_streams(streams, data, piece)
            assert tot == [sum(len(s) for s in streams), len(streams)] and [len(s) for s in streams] == [int(v) for v in zs]


@pytest.mark.parametrize("name", SOURCES)
def test_sources(caller, name):
    for piece, n in ((8216, 3 * 8216 + 100), (M, M + 77), (40, 40 * 7 + 3)):
        data = source(name, n)
        streams, _, _ = zpieces(caller, data, piece, 1)
        kinds = check_streams(streams, data, piece)
        if name == "random":
            assert all(k == 0 for k in kinds) and [len(s) for s in streams] == [len(data[k * piece : (k + 1) * piece]) + 11 for k in range(len(streams))]
        if name in ("zeros", "abc", "period8", "ff") and piece >= 8216:
            # long matches, as far as a lane-parallel parse lets them run: a match ends with its lane's segment, so a piece costs at least
            # 256 matches.  From the format alone: 256 matches of at most 15 + 5 + 15 + 13 bits (1 536 bytes), the first round's 256
            # positions, which have no earlier round to look into, as literals of at most 15 bits (480 bytes), a header of at most 564
            # bytes: 2 580 bytes, below a third of the smallest piece here
            assert all(k == 2 for k in kinds[:-1]) and all(len(s) < piece // 3 for s in streams[:-1])
        if name in ("skewed", "text") and piece >= 8216:
            assert kinds[0] == 2 and len(streams[0]) < piece


def test_a_full_piece_of_ff_has_the_largest_adler_sums(caller):
    data = b"\xff" * (2 * M)
    streams, _, _ = zpieces(caller, data, M)
    check_streams(streams, data, M)
    assert streams[0] == streams[1] and int.from_bytes(streams[0][-4:], "big") == zlib.adler32(b"\xff" * M)


def test_a_repeat_beyond_the_window_is_no_match(caller):
    """A piece may be longer than DEFLATE's 32 768-byte window: bytes that repeat 40 000 back cannot be a match."""
    first = bytes((np.random.default_rng(9050).integers(0, 16, 40_000, dtype=np.uint8) * 16).astype(np.uint8))
    data = first + first[: M - 40_000]
    streams, _, _ = zpieces(caller, data, M)
    assert check_streams(streams, data, M) == [2] and len(streams[0]) < M * 5 // 8  # 16 symbols: 4 bits a byte, and a header


def test_three_thousand_pieces_a_workgroup_loops(caller):
    rng = np.random.default_rng(9100)
    data = bytes((rng.integers(0, 3, 3000 * 40, dtype=np.uint8) + 65).astype(np.uint8))
    streams, _, tot = zpieces(caller, data, 40, 3)
    check_streams(streams, data, 40)
    assert tot[1] == 3000


# ---- 2. a stream is a function of its piece's bytes alone ----------------------------------------------------------------------------------------
def test_function_of_the_bytes_alone(caller):
    rng = np.random.default_rng(9200)
    for piece in (40, 8216):
        n_p = 3000 if piece == 40 else 9
        mine = source("text", piece) if piece == 40 else source("period8", 4000) + source("text", piece - 4000)
        other = lambda: bytes((rng.integers(0, 5, piece, dtype=np.uint8) * 50).astype(np.uint8))
        first = b"".join([mine] + [other() for _ in range(n_p - 2)] + [mine])
        a, _, _ = zpieces(caller, first, piece, 0)
        assert a[0] == a[n_p - 1]  # at index 0 and at the last index
        for off in (1, 2, 3):  # at every source offset
            b, _, _ = zpieces(caller, first[: 2 * piece], piece, off)
            assert b[0] == a[0] and b[1] == a[1]
        again, _, _ = zpieces(caller, first, piece, 0)  # in two calls
        assert again == a
        second = b"".join([other(), mine, other()])  # with different neighbours
        c, _, _ = zpieces(caller, second, piece, 2)
        assert c[1] == a[0]
        alone, _, _ = zpieces(caller, mine, piece, 0)
        assert alone == [a[0]]
        assert zlib.decompress(a[0]) == mine


# ---- 3. rooms and errors ------------------------------------------------------------------------------------------------------------------------
def test_rooms_one_short_and_errors(caller):
    data = source("text", 5 * 300 + 17)
    streams, zs, tot = zpieces(caller, data, 300)
    check_streams(streams, data, 300)
    exact, _, tot2 = zpieces(caller, data, 300, 0, out_room=tot[0], sizes_room=tot[1])
    assert exact == streams and tot2 == tot
    got, zs1, tot1 = zpieces(caller, data, 300, 0, out_room=tot[0] - 1)  # (that the short array holds nothing is checked inside)
    assert got is None and tot1 == tot and (zs1 == zs).all()
    blob, zs2, tot3 = zpieces(caller, data, 300, 0, sizes_room=tot[1] - 1)
    assert zs2 is None and tot3 == tot and blob == b"".join(streams)
    got, zs0, tot0 = zpieces(caller, data, 300, 0, out_room=0, sizes_room=0)
    assert got is None and zs0 is None and tot0 == tot
    none, _, tot_none = zpieces(caller, b"", 300)  # no byte: no piece
    assert none == [] and tot_none == [0, 0]
    L, h = caller._L, caller._h
    buf, t = guarded(4096), guarded(16)
    f = L.bsc_zlib_pieces_device
    A = (buf.data_ptr(), 1024, buf.data_ptr() + 2048, 16, t.data_ptr(), None)
    assert f(h, buf.data_ptr(), 100, 0, *A) == -1 and b"piece" in L.bsc_last_error()
    assert f(h, buf.data_ptr(), 100, M + 1, *A) == -1 and b"piece" in L.bsc_last_error()
    assert f(None, buf.data_ptr(), 100, 10, *A) == -1
    assert f(h, None, 100, 10, *A) == -1 and b"NULL" in L.bsc_last_error()
    assert f(h, buf.data_ptr(), 100, 10, None, 1024, *A[2:]) == -1 and f(h, buf.data_ptr(), 100, 10, *A[:2], None, 16, *A[4:]) == -1
    assert f(h, buf.data_ptr(), 100, 10, *A[:4], None, None) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all() and (t.cpu().numpy() == GUARD).all()
    streams2, _, _ = zpieces(caller, data, 300)  # the context is usable
    assert streams2 == streams


# ---- 4. the block level -------------------------------------------------------------------------------------------------------------------------
def device_stream(caller, recs, x0, S):
    """bsc_bigwig_sites_device's stream over the records, left on the device: (tensor, bytes)."""
    n = len(recs)
    raw = recs.view(np.uint8).reshape(-1, 128)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to("cuda")
    d_core, d_aux = up(raw[:, :64]), up(raw[:, 64:])
    n_sec = -(-n // S)
    out, sec, zoom, tot = guarded(24 * n_sec + 8 * n), guarded(40 * n_sec), guarded(40 * n), guarded(48)
    caller.bigwig_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, x0, 3, out.data_ptr(), 24 * n_sec + 8 * n, sec.data_ptr(), n_sec, zoom.data_ptr(), n,
                               tot.data_ptr(), None, {"items_per_section": S, "reduction": 64})
    torch.cuda.synchronize()
    nb = int(tot.cpu().numpy()[:8].view(np.uint64)[0])
    return out, out.cpu().numpy()[:nb].tobytes()


@pytest.mark.parametrize("S", [1, 3, 64, 1024, 8157])
def test_sections_of_a_device_stream_at_every_border(caller, S):
    rng = np.random.default_rng(9300 + S)
    piece = 24 + 8 * S
    for count in ((S - 1, S, S + 1) if S == 8157 else (S - 1, S, S + 1, 2 * S + 1)):
        if count == 0:
            continue
        recs = all_sites(random_records(rng, count, 77))
        d_out, raw = device_stream(caller, recs, 77, S)
        assert len(raw) == 24 * -(-count // S) + 8 * count
        n_p = -(-len(raw) // piece)
        out, sizes, tot = guarded(len(raw) + 11 * n_p), guarded(4 * n_p), guarded(16)
        caller.zlib_pieces_device(d_out.data_ptr(), len(raw), piece, out.data_ptr(), len(raw) + 11 * n_p, sizes.data_ptr(), n_p, tot.data_ptr())
        torch.cuda.synchronize()
        zs = sizes.cpu().numpy()[: 4 * n_p].view(np.uint32)
        blob, at = out.cpu().numpy(), 0
        assert [int(v) for v in tot.cpu().numpy()[:16].view(np.uint64)] == [int(zs.sum()), n_p] and n_p == -(-count // S)
        for k in range(n_p):  # stream k inflates to section k
            s = blob[at : at + int(zs[k])].tobytes()
            assert s[:2] == b"\x78\x9c" and zlib.decompress(s) == raw[k * piece : (k + 1) * piece]
            at += int(zs[k])
        assert (blob[at:] == GUARD).all() and (d_out.cpu().numpy()[: len(raw)].tobytes() == raw)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The BAM of three contigs tests/test_gpu_bigwig.py uses: 6 000 positions at ~40x, one of 60 positions, 30 000 covered thinly in several blocks."""
    d = tmp_path_factory.mktemp("bigwig_z_files")
    rng = np.random.default_rng(4711)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50)
            + W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def test_block_entry_deflates_the_kept_block_and_touches_nothing_else(caller, small):
    _, bam, _, refs, reference = small
    par = {"contexts": 1}
    n_blocks, n_streams, cur = 0, 0, None
    with B.SiteCaller() as fresh:  # no bsc_block_bigwig_kept came before it
        with pytest.raises(B.BscError, match="bsc_block_bigwig_kept"):
            fresh.block_bigwig_deflate()
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            ref = block_reference(codes, int(blk.x), int(blk.y))
            if name != cur:
                cur = name
                caller.meth_regions_attach(sorted([(0, len(codes))] + [(s, min(s + 100, len(codes))) for s in range(0, len(codes), 100)]))
            bcf0, _, _ = caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
            table0 = caller.block_meth_kept(name, par)
            ent0 = caller.block_csi_kept(14)[0].tobytes()
            caller.block_meth_regions_kept(par)
            acc0 = caller.meth_regions_read().copy()
            _, sites, _, _ = caller.block_bigwig_kept(tid, par, None)
            if sites == 0:
                assert caller.block_bigwig_deflate()[0] == b"" and len(caller.block_bigwig_deflate()[1]) == 0  # a block with no site: 0 / 0
                continue
            for S in sorted({sites + 1, sites, max(sites - 1, 1), max((sites - 1) // 2, 1), 50}):  # sites = S - 1, S, S + 1, 2 S + 1 (or + 2)
                if S > 8157:
                    continue
                bwp = {"items_per_section": S, "reduction": 128}
                raw, ns, secs, _ = caller.block_bigwig_kept(tid, par, bwp)
                zdata, zs = caller.block_bigwig_deflate()
                assert ns == sites and len(zs) == len(secs) == -(-sites // S) and int(zs.sum()) == len(zdata)
                at = 0
                for k, size in enumerate(int(v) for v in zs):
                    assert zlib.decompress(zdata[at : at + size]) == raw[k * (24 + 8 * S) : (k + 1) * (24 + 8 * S)]
                    at += size
                n_streams += len(zs)
                assert caller.bigwig_stream_read(0, len(raw)) == raw  # the uncompressed stream is still there
                assert caller.bigwig_zstream_read(2, 3) == zdata[2:5]
                with pytest.raises(B.BscError):
                    caller.bigwig_zstream_read(len(zdata), 1)
            # byte-equal before and after: the kept stream, the table, the .csi entries, the region sums
            assert kept_stream(caller, len(bcf0)) == bcf0 and caller.block_meth_kept(name, par) == table0
            assert caller.block_csi_kept(14)[0].tobytes() == ent0 and (caller.meth_regions_read() == acc0).all()
            caller.meth_regions_reset()
            # S = 8158: a section of 65 288 bytes is refused; and so is a deflate behind a kept call that failed
            caller.block_bigwig_kept(tid, par, {"items_per_section": 8158, "reduction": 128})
            with pytest.raises(B.BscError, match="8157"):
                caller.block_bigwig_deflate()
            caller.block_bigwig_kept(tid, par, {"items_per_section": 8157, "reduction": 128})
            assert len(caller.block_bigwig_deflate()[1]) == -(-sites // 8157)
            with pytest.raises(B.BscError):
                caller.block_bigwig_kept(tid, par, {"items_per_section": 0, "reduction": 128})
            with pytest.raises(B.BscError, match="bsc_block_bigwig_kept"):
                caller.block_bigwig_deflate()
            n_blocks += 1
    caller.meth_regions_attach([])
    assert n_blocks > 3 and n_streams > 20


# ---- 5. the ratio -------------------------------------------------------------------------------------------------------------------------------
def test_ratio_next_to_zlib(caller):
    """The sections (S = 1024) of the device's stream for 30x synthetic reads over 220 000 positions: the device's total next to zlib level 1
    and Z_HUFFMAN_ONLY per section.  Hard: no stream above its piece + 11.  Target: the device total <= 1.05 x the level-1 total.

    Measured on an MI355X (2026-10-19): 26 906 sites, 215 896 bytes raw; device 101 657, level 1 99 343, Z_HUFFMAN_ONLY 142 461: 1.0233."""
    seed = 424242
    tpl, seq = B.synth_reads_host(seed, 5_000, 220_000, 30)
    x, y = 4_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    n = y - x + 1
    ref = B.synth_ref_host(seed, x, n + 2)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1)).to("cuda")
    d_tpl, d_seq, d_ref = up(tpl), up(seq), up(ref)
    d_core, d_aux = torch.zeros(n * 64, dtype=torch.uint8, device="cuda"), torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    caller.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core.data_ptr(), d_aux.data_ptr())
    n_sec = n // 1024 + 1
    out, sec, zoom, tot = guarded(24 * n_sec + 8 * n), guarded(40 * n_sec), guarded(40 * (n // 1024 + 2)), guarded(48)
    caller.bigwig_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, x, 0, out.data_ptr(), 24 * n_sec + 8 * n, sec.data_ptr(), n_sec, zoom.data_ptr(),
                               n // 1024 + 2, tot.data_ptr())
    torch.cuda.synchronize()
    nb, sites = (int(v) for v in tot.cpu().numpy()[:16].view(np.uint64))
    assert sites >= 20_000 and nb == 24 * -(-sites // 1024) + 8 * sites
    raw = out.cpu().numpy()[:nb].tobytes()
    piece = 24 + 8 * 1024
    streams, _, totals = zpieces(caller, raw, piece)
    check_streams(streams, raw, piece)
    lvl1 = huff = 0
    for k in range(len(streams)):
        part = raw[k * piece : (k + 1) * piece]
        lvl1 += len(zlib.compress(part, 1))
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        huff += len(co.compress(part) + co.flush())
    print("\nbigwig sections: %d sites, %d bytes raw; device %d, zlib level 1 %d, Z_HUFFMAN_ONLY %d; device / level 1 = %.4f"
          % (sites, nb, totals[0], lvl1, huff, totals[0] / lvl1))
    assert all(len(s) <= len(raw[k * piece : (k + 1) * piece]) + 11 for k, s in enumerate(streams))
    assert totals[0] <= 1.05 * lvl1


# ---- 6. file to file ------------------------------------------------------------------------------------------------------------------------------
def same_track(a, b, refs):
    assert a.header["zoomLevels"] == b.header["zoomLevels"] and a.summary == b.summary and a.chroms == b.chroms and a.section_count == b.section_count
    assert [z[0] for z in a.zooms] == [z[0] for z in b.zooms]
    for name, _ in refs:
        assert a.intervals(name) == b.intervals(name)
        for l in range(len(a.zooms)):
            assert a.zoom_records(l, name) == b.zoom_records(l, name)
    for l in range(len(a.zooms)):
        assert a.zoom_records(l) == b.zoom_records(l)


def test_bam2bcf_meth_bigwig_compress_and_pipeline(caller, small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("z" + s))
    common = ["--meth-bigwig-section", "50", "--meth-bigwig-zoom", "8", bam, fa]
    run_exe("--meth", p(".0.meth"), "--meth-bigwig", p(".0.bw"), *common, p(".0.bcf"), p(".0.json"), "S9")
    run_exe("--meth", p(".1.meth"), "--meth-bigwig", p(".1.bw"), "--meth-bigwig-compress", *common, p(".1.bcf"), p(".1.json"), "S9")
    for ext in (".meth", ".bcf", ".json"):
        assert open(p(".1" + ext), "rb").read() == open(p(".0" + ext), "rb").read(), ext
    plain, comp = bigwig.read(p(".0.bw")), bigwig.read(p(".1.bw"))
    leaves = [hit for at in [comp.header["fullIndexOffset"]] + [z[2] for z in comp.zooms] for hit in comp._rtree_hits(at, None, 0, 0)]
    largest = max(len(zlib.decompress(comp.raw[off : off + size])) for off, size in leaves)
    assert plain.header["uncompressBufSize"] == 0 and comp.header["uncompressBufSize"] == largest >= 24 + 8 * 50
    same_track(plain, comp, refs)
    assert plain.summary["basesCovered"] > 300 and comp.header["zoomLevels"] >= 2
    assert os.path.getsize(p(".1.bw")) < os.path.getsize(p(".0.bw"))
    # pipeline.run agrees with the binary
    s = pipeline.run(bam, reference, p(".p.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, bigwig_path=p(".p.bw"),
                     bigwig_section=50, bigwig_zoom=8, bigwig_compress=True)
    piped = bigwig.read(p(".p.bw"))
    same_track(comp, piped, refs)
    assert piped.header["uncompressBufSize"] == comp.header["uncompressBufSize"] and s["bigwig_sites"] == plain.summary["basesCovered"]
    assert open(p(".p.bw"), "rb").read() == open(p(".1.bw"), "rb").read()  # (the device's streams are a function of the sections' bytes alone)
    # the refusals
    r = run_exe("--meth-bigwig-compress", bam, fa, p(".no.bcf"), p(".no.json"), ok=False)
    assert r.returncode == 2 and "needs --meth-bigwig" in r.stderr
    r = run_exe("--meth-bigwig", p(".no.bw"), "--meth-bigwig-compress", "--meth-bigwig-section", "8158", bam, fa, p(".no.bcf"), p(".no.json"), ok=False)
    assert r.returncode == 2 and "8157" in r.stderr
    r = run_exe("--meth-bigwig", p(".no.bw"), "--meth-bigwig-compress", "--rank", "0", "--world", "2", bam, fa, p(".no.bcf"), p(".no.json"), ok=False)
    assert r.returncode == 2 and "single run" in r.stderr
    for kw in (dict(bigwig_path=None), dict(bigwig_section=8158), dict(device_reader=False)):
        with pytest.raises(ValueError):
            pipeline.run(bam, reference, p(".no"), **dict(dict(device_reader=True, bigwig_path=p(".no.bw"), bigwig_compress=True), **kw))
    assert not os.path.exists(p(".no.bw")) and not os.path.exists(p(".no.bcf")) and not os.path.exists(p(".no"))
    run_exe("--meth-bigwig", p(".8.bw"), "--meth-bigwig-compress", "--meth-bigwig-section", "8157", bam, fa, p(".8.bcf"), p(".8.json"), "S9")
    run_exe("--meth-bigwig", p(".9.bw"), "--meth-bigwig-section", "8157", bam, fa, p(".9.bcf"), p(".9.json"), "S9")
    same_track(bigwig.read(p(".9.bw")), bigwig.read(p(".8.bw")), refs)
