"""The bedMethyl table as bigBed items on the device (csrc/bigbeddev.hip: the bsc_bigbed_*_kernel family): the call's stream of items, the
blocks' and the level-0 windows' summaries and the four totals against the host form (bsc_bigbed_blocks_recs, which
tests/test_bigbed_host.py holds to the rule in two other forms) on dense arrays of random record contents — every array length around a
tile, every block size around its border, block borders on and inside tiles, window borders, positions of 1 to 10 digits up to 2^32 - 1,
counts of 1 to 10 digits, the records that attain the shortest and the longest item, with and without the chain's emit byte, under the
thresholds, with each room one short — and against bsc_meth_sites_device's table on the same arrays.  Then the deflate over ranges of
varying length (csrc/zlibdev.hip: bsc_zlib_ranges_device): Python's zlib checks every stream.  Every comparison is of exact integers or
bytes."""
import ctypes as C
import importlib.util
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import bs_call_amd as B
import methbed_ref as MB
from bs_call_amd import _lib, bigbed, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from methregions_ref import random_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
GUARD = 0xA5
M = 0xFF00


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def guarded(n_bytes):
    """Room of n_bytes on the device with 64 guard bytes behind it, filled with the guard value."""
    return torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")


def rows(a):
    return [tuple(int(v) for v in r) for r in a]


def all_sites(recs):
    """Every record a site under the default parameters."""
    c = recs["core"]
    c["emit"], c["gt"], c["cg"] = 1, np.where(np.arange(len(recs)) % 3 == 0, 7, 4), b"C"
    recs["core"] = c
    recs["counts"] = np.maximum(recs["counts"], 1)
    return recs


def no_sites(recs):
    c = recs["core"]
    c["gt"] = 5
    recs["core"] = c
    return recs


def host_block(recs, chrom_id, par, bbp):
    raw, blk, zoom = bigbed.blocks_recs_host(recs, chrom_id, par, bbp)
    return raw, rows(blk), rows(zoom), [len(raw), int(blk["count"].sum()) if len(blk) else 0, len(blk), len(zoom)]


def unpack(out, blk, zoom, tot, rooms):
    """The device buffers as (bytes, blocks, zoom0, totals); the guard bytes behind every room are checked here."""
    torch.cuda.synchronize()
    totals = [int(v) for v in tot.cpu().numpy().view(np.uint64)[:4]]
    assert (tot.cpu().numpy()[32:] == GUARD).all()
    res = []
    for buf, room, need, item in ((out, rooms[0], totals[0], 1), (blk, 24 * rooms[1], 24 * totals[2], 24), (zoom, 24 * rooms[2], 24 * totals[3], 24)):
        h = buf.cpu().numpy()
        assert (h[room:] == GUARD).all(), "written behind the room given"
        if need > room:
            assert (h == GUARD).all(), "a room too small is not written at all"
            res.append(None)
        else:
            assert (h[need:room] == GUARD).all(), "written behind what was reported"
            res.append(h[:need].tobytes() if item == 1 else rows(np.frombuffer(h[:need].tobytes(), dtype=bigbed.BB_SUM)))
    return res[0], res[1], res[2], totals


def default_rooms(n, bp):
    return (bigbed.ITEM_MAX * n, -(-n // bp["items_per_block"]), n)


def device_block(caller, recs, x0, chrom_id=0, par=None, bbp=None, rooms=None):
    """bsc_bigbed_sites_device over the records' two halves.  rooms: (bytes, blocks, windows); default: what every position a site needs."""
    n = len(recs)
    bp = dict({"items_per_block": 512, "reduction": 1024}, **(bbp or {}))
    rooms = default_rooms(n, bp) if rooms is None else rooms
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    out, blk, zoom, tot = guarded(rooms[0]), guarded(24 * rooms[1]), guarded(24 * rooms[2]), guarded(32)
    caller.bigbed_sites_device(d_core.data_ptr() if n else None, d_aux.data_ptr() if n else None, n, x0, chrom_id, out.data_ptr(), rooms[0], blk.data_ptr(),
                               rooms[1], zoom.data_ptr(), rooms[2], tot.data_ptr(), par, bp)
    return unpack(out, blk, zoom, tot, rooms)


def launch_with_emit(caller, recs, emit, x0, chrom_id=0, par=None, bbp=None):
    """The launcher behind the entry (bsc_dev_launch_bigbed) with the chain's emit byte per position, as a block follow-up would hand it
    over — the public per-position entry has no such array.  The workspaces have guard bytes behind them too.  COUPLING: the argument list
    below restates csrc/bigbeddev.hip's bsc_dev_launch_bigbed by hand, an internal symbol; a change there must be made here too (ctypes would
    not notice).  The emit path is also covered through the public bsc_block_bigbed_kept in the block-entry test."""
    L = caller._L
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.bsc_dev_launch_bigbed.restype = C.c_int
    L.bsc_dev_launch_bigbed.argtypes = [vp, vp, vp, u64, u32, u32, C.POINTER(_lib.MethParams), C.POINTER(_lib.BbParams)] + [vp] * 8 + [C.c_size_t, vp, vp,
                                        vp, u64, vp, u64, vp, u64, vp, C.c_int, vp]
    L.bsc_dev_scan_tmp_bytes_u64.restype = C.c_int
    L.bsc_dev_scan_tmp_bytes_u64.argtypes = [C.c_uint32, C.POINTER(C.c_size_t)]
    n = len(recs)
    n_tiles = (n + 63) // 64
    scan = C.c_size_t(0)
    assert L.bsc_dev_scan_tmp_bytes_u64(n_tiles + 1, C.byref(scan)) == 0
    bpd = dict({"items_per_block": 512, "reduction": 1024}, **(bbp or {}))
    bp = _lib.BbParams(**bpd)
    rooms = default_rooms(n, bpd)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux, d_emit = dev(raw[:, :64]), dev(raw[:, 64:]), dev(emit)
    used = [n] + [8 * (n_tiles + 1)] * 6 + [scan.value, 4 * n, 4 * (n + 1)]  # item_len, cnt, off, tbytes, boff, hcnt, hoff, scan, sites, wbeg
    ws = [guarded(u) for u in used]
    out, blk, zoom, tot = guarded(rooms[0]), guarded(24 * rooms[1]), guarded(24 * rooms[2]), guarded(32)
    torch.cuda.synchronize()
    mp = _lib.MethParams(**(par or {}))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc = L.bsc_dev_launch_bigbed(d_core.data_ptr(), d_aux.data_ptr(), d_emit.data_ptr(), n, x0, chrom_id, C.byref(mp), C.byref(bp), *[w.data_ptr() for w in ws[:8]],
                                 scan.value, ws[8].data_ptr(), ws[9].data_ptr(), out.data_ptr(), rooms[0], blk.data_ptr(), rooms[1], zoom.data_ptr(), rooms[2],
                                 tot.data_ptr(), cus, None)
    assert rc == 0
    got = unpack(out, blk, zoom, tot, rooms)
    for w, u in zip(ws, used):  # nothing behind the workspaces either
        assert (w.cpu().numpy()[u:] == GUARD).all()
    return got


# ---- 1. array lengths, with and without the emit bytes ----------------------------------------------------------------------------------------
LENGTHS = [1, 63, 64, 65, 127, 128, 129, 64 * 37 + 5]


@pytest.mark.parametrize("n", LENGTHS)
def test_array_lengths_with_and_without_the_emit_bytes(caller, n):
    rng = np.random.default_rng(8000 + n)
    x0, bbp = 1000, {"items_per_block": 5, "reduction": 16}
    recs = random_records(rng, n, x0, wide=True)
    want = host_block(recs, 4, {"contexts": 1}, bbp)
    assert device_block(caller, recs, x0, 4, {"contexts": 1}, bbp) == want
    if n > 64:
        assert want[3][2] > 1 and want[3][3] > 1
    emit = rng.choice([0, 1, 1, 1, 255], n).astype(np.uint8)  # the chain's byte per position: 0 takes a record away, whatever its own bytes say
    gated = recs.copy()
    c = gated["core"]
    c["emit"][emit == 0] = 0
    gated["core"] = c
    want_e = host_block(gated, 4, {"contexts": 1}, bbp)
    assert launch_with_emit(caller, recs, emit, x0, 4, {"contexts": 1}, bbp) == want_e
    py = bigbed.blocks_of_recs(gated, 4, {"contexts": 1}, 5, 16)
    assert want_e[:3] == (py[0], rows(py[1]), rows(py[2]))
    if n >= 64:
        assert want_e != want


# ---- 2. block sizes around their borders; borders on and inside tiles -------------------------------------------------------------------------
@pytest.mark.parametrize("B_items", [1, 3, 64, 65, 512])
def test_block_sizes_and_site_counts(caller, B_items):
    rng = np.random.default_rng(8100 + B_items)
    for count in (B_items - 1, B_items, B_items + 1, 2 * B_items + 1):
        bbp = {"items_per_block": B_items, "reduction": 64}
        # exactly `count` sites: dense (B = 64: a block's border on every tile's border; 65: inside), and thinned (a site every third
        # position, so ranks and positions part ways)
        dense = all_sites(random_records(rng, max(count, 1), 77, wide=True))
        if count == 0:
            dense = no_sites(dense)
        want = host_block(dense, 1, None, bbp)
        assert want[3][1] == count and want[3][2] == -(-count // B_items)
        assert device_block(caller, dense, 77, 1, None, bbp) == want
        thin = all_sites(random_records(rng, 3 * count + 1, 500, wide=True))
        c = thin["core"]
        c["gt"][np.arange(len(thin)) % 3 != 1] = 0
        thin["core"] = c
        want = host_block(thin, 1, None, bbp)
        assert want[3][1] == count
        assert device_block(caller, thin, 500, 1, None, bbp) == want
        if count:
            assert want[1][-1][2] == (count - 1) % B_items + 1 and want[1][0][4] == 0
            assert [b[4] for b in want[1]] == sorted({b[4] for b in want[1]})


# ---- 3. windows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("red", [1, 7, 64, 100, 1024])
def test_reductions_with_borders_on_and_inside_tiles(caller, red):
    rng = np.random.default_rng(8200 + red)
    n = 64 * 37 + 5
    for x0 in (1, 30, 1000):  # x0 = 1: start = index, so a window of 64 or 1024 begins on a tile's border; the others begin inside a tile
        recs = random_records(rng, n, x0, wide=True)
        want = host_block(recs, 2, None, {"reduction": red})
        assert device_block(caller, recs, x0, 2, None, {"reduction": red}) == want
        starts = [z[0] // red for z in want[2]]
        assert starts == sorted(set(starts)) and sum(z[2] for z in want[2]) == want[3][1] > 1000
        if red == 1:
            assert want[3][3] == want[3][1]


# ---- 4. digits: positions of 1 to 10 digits up to 2^32 - 1, counts of 1 to 10 digits, the shortest and the longest item ---------------------------
def test_positions_of_one_to_ten_digits(caller):
    rng = np.random.default_rng(8300)
    n = 140
    for x0 in [1] + [10**d - 70 for d in range(2, 10)] + [2**32 - n]:  # every power of ten is crossed inside the array; the last position is 2^32 - 1
        recs = all_sites(random_records(rng, n, x0, wide=True))
        for bbp in ({"items_per_block": 10, "reduction": 64}, {"items_per_block": 65535, "reduction": 2**32 - 1}):
            want = host_block(recs, 7, None, bbp)
            assert want[3][1] == n
            assert device_block(caller, recs, x0, 7, None, bbp) == want
    assert want[1][-1][1] == 2**32 - 1 and b"\t4294967294\t4294967295\t" in want[0][-100:]


def test_counts_of_one_to_ten_digits_and_the_extreme_items(caller):
    n, x0 = 256, 3
    recs = all_sites(random_records(np.random.default_rng(8400), n, x0))
    vals = [0, 1, 9, 10, 99, 100, 999, 1000, 10**4 - 1, 10**5, 10**6 - 1, 10**7, 10**8 - 1, 10**8, 10**9 - 1, 10**9, 4 * 10**9, 2**32 - 1]
    for i in range(n):
        a, b = vals[i % len(vals)], vals[(i // len(vals) + i) % len(vals)]
        recs["counts"][i] = 0
        recs["counts"][i, 5], recs["counts"][i, 6], recs["counts"][i, 7], recs["counts"][i, 4] = a, a, b, b  # (a = b = 0: no site)
    c = recs["core"]
    c["cg"][1::2] = b"H"
    c["phred"] = np.arange(n) % 256
    # the shortest item: pos <= 9 (index 0 .. 6), a = 0, b = 1 .. 9, GQ <= 9, "CG"; the longest: a = b = 4 * 10^9, GQ 255, a CH? name, at the top
    c["cg"][2], c["phred"][2], c["flt"][2] = b"C", 5, 0
    recs["core"] = c
    recs["counts"][2] = 0
    recs["counts"][2, 5], recs["counts"][2, 6], recs["counts"][2, 7], recs["counts"][2, 4] = 0, 0, 7, 7
    want = host_block(recs, 0, {"contexts": 1}, {"items_per_block": 7, "reduction": 10})
    lens = [12 + len(t) + 1 for _, _, _, t in bigbed.items_of_stream(want[0])]
    assert min(lens) == bigbed.ITEM_MIN and want[3][1] > 200
    assert device_block(caller, recs, x0, 0, {"contexts": 1}, {"items_per_block": 7, "reduction": 10}) == want
    top = all_sites(random_records(np.random.default_rng(8401), 70, 2**32 - 70))
    c = top["core"]
    c["cg"], c["phred"] = b"H", 255
    top["core"] = c
    top["counts"] = 4_000_000_000
    want = host_block(top, 2**32 - 1, {"contexts": 1}, {"items_per_block": 64, "reduction": 1})
    assert len(want[0]) == 70 * bigbed.ITEM_MAX  # a whole tile of the longest items: the wave's image at its fullest
    assert device_block(caller, top, 2**32 - 70, 2**32 - 1, {"contexts": 1}, {"items_per_block": 64, "reduction": 1}) == want


# ---- 5. the thresholds, no site at all, the table ------------------------------------------------------------------------------------------------
def test_thresholds_and_all_contexts(caller):
    rng = np.random.default_rng(8500)
    n, x0 = 1500, 4000
    recs = random_records(rng, n, x0)
    c = recs["core"]  # called neighbours that are bases, so that every name occurs (random bytes give CHN almost always)
    c["cx_gt"] = np.ascontiguousarray(rng.choice(list(b"ACGTN"), (n, 5)).astype(np.uint8)).view("S5").reshape(-1)
    recs["core"] = c
    bbp = {"items_per_block": 100, "reduction": 50}
    plain = device_block(caller, recs, x0, 0, None, bbp)
    assert plain == host_block(recs, 0, None, bbp)
    for par in ({"min_cov": 5}, {"min_phred": 100}, {"pass_only": 1}, {"contexts": 1}, {"contexts": 1, "min_cov": 3, "min_phred": 20, "pass_only": 1}):
        got = device_block(caller, recs, x0, 0, par, bbp)
        assert got == host_block(recs, 0, par, bbp) and got != plain, par
        if par == {"contexts": 1}:
            assert got[3][1] > plain[3][1] and b"CHH\t" in got[0] and b"CHG\t" in got[0] and b"CHN\t" in got[0]
        elif "contexts" not in par:
            assert 0 < got[3][1] < plain[3][1]


def test_no_site_at_all(caller):
    recs = no_sites(random_records(np.random.default_rng(8600), 300, 10))
    assert device_block(caller, recs, 10) == (b"", [], [], [0] * 4) == host_block(recs, 0, None, None)
    assert device_block(caller, recs[:0], 10) == (b"", [], [], [0] * 4)  # no position either


def test_items_rejoined_are_the_table_s_bytes(caller):
    rng = np.random.default_rng(8700)
    n, x0 = 64 * 37 + 5, 1000
    recs = random_records(rng, n, x0, wide=True)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    d_out = torch.zeros(400 * n, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    for par in ({}, {"contexts": 1, "min_cov": 2}):
        caller.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chrW", d_out.data_ptr(), d_out.numel(), d_tot.data_ptr(), params=par)
        torch.cuda.synchronize()
        n_bytes, lines = (int(v) for v in d_tot.cpu().numpy().view(np.uint64)[:2])
        table = d_out[:n_bytes].cpu().numpy().tobytes()
        got = device_block(caller, recs, x0, 3, par)
        assert got[3][1] == lines > 500 and sum(b[2] for b in got[1]) == lines == sum(z[2] for z in got[2])
        assert bigbed.lines_of_stream(got[0], {3: b"chrW"}) == table


# ---- 6. each room one short; errors ------------------------------------------------------------------------------------------------------------
def test_each_room_one_short(caller):
    rng = np.random.default_rng(8800)
    n, x0 = 700, 50
    recs = random_records(rng, n, x0, wide=True)
    bbp = {"items_per_block": 16, "reduction": 32}
    want = host_block(recs, 3, None, bbp)
    exact = (want[3][0], want[3][2], want[3][3])
    assert min(exact) > 10
    assert device_block(caller, recs, x0, 3, None, bbp, rooms=exact) == want  # exactly enough
    for k in range(3):
        rooms = tuple(v - (1 if j == k else 0) for j, v in enumerate(exact))
        got = device_block(caller, recs, x0, 3, None, bbp, rooms=rooms)  # (the guard bytes, and that the short array holds nothing, are checked inside)
        assert got[3] == want[3]  # the needs are reported all the same
        assert got[k] is None and [g for j, g in enumerate(got[:3]) if j != k] == [w for j, w in enumerate(want[:3]) if j != k]
    assert device_block(caller, recs, x0, 3, None, bbp, rooms=(0, 0, 0)) == (None, None, None, want[3])


def test_errors_leave_the_context_usable(caller):
    L, h = caller._L, caller._h
    recs = random_records(np.random.default_rng(8900), 300, 100, wide=True)
    want = host_block(recs, 0, None, None)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    out, tot = guarded(4096), guarded(32)
    ok, bp = _lib.MethParams(), _lib.BbParams()
    A = (d_core.data_ptr(), d_aux.data_ptr(), 300)
    Z = (out.data_ptr(), 0, out.data_ptr(), 0, out.data_ptr(), 0, tot.data_ptr(), None)
    f = L.bsc_bigbed_sites_device
    assert f(h, *A, 0, 0, C.byref(ok), C.byref(bp), *Z) == -1 and b"1-based" in L.bsc_last_error()
    assert f(h, *A, 2**32 - 299, 0, C.byref(ok), C.byref(bp), *Z) == -1 and b"beyond" in L.bsc_last_error()
    assert f(h, *A, 100, 0, None, C.byref(bp), *Z) == -1 and f(h, *A, 100, 0, C.byref(ok), None, *Z) == -1
    assert f(h, *A, 100, 0, C.byref(_lib.MethParams(contexts=2)), C.byref(bp), *Z) == -1
    for bad in (_lib.BbParams(0, 1), _lib.BbParams(65536, 1), _lib.BbParams(1, 0)):
        assert f(h, *A, 100, 0, C.byref(ok), C.byref(bad), *Z) == -1 and b"items_per_block" in L.bsc_last_error()
    assert f(h, d_core.data_ptr() + 8, d_aux.data_ptr(), 299, 100, 0, C.byref(ok), C.byref(bp), *Z) == -1 and b"16-byte" in L.bsc_last_error()
    assert f(h, *A, 100, 0, C.byref(ok), C.byref(bp), out.data_ptr() + 8, 8, *Z[2:]) == -1 and b"16-byte" in L.bsc_last_error()
    assert f(h, *A, 100, 0, C.byref(ok), C.byref(bp), out.data_ptr(), 0, out.data_ptr() + 4, 1, *Z[4:]) == -1 and b"8-byte" in L.bsc_last_error()
    assert f(h, None, d_aux.data_ptr(), 300, 100, 0, C.byref(ok), C.byref(bp), *Z) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all() and (tot.cpu().numpy() == GUARD).all()
    assert device_block(caller, recs, 100) == want


# ---- 7. the deflate over ranges -------------------------------------------------------------------------------------------------------------------
def zranges(caller, data, lens, max_piece, src_off=0, out_room=None, sizes_room=None):
    """bsc_zlib_ranges_device over ranges of `lens` bytes of `data`, back to back, the data lying src_off bytes behind a 256-byte aligned address.  Returns (streams or None, sizes or None, totals, the ranges' bytes): None where the
    room was too small — that the array is then untouched, and the guard bytes behind every room, are checked here."""
    offs = [0]
    for ln in lens:
        offs.append(offs[-1] + ln)
    assert offs[-1] <= len(data)
    pieces = [data[a:b] for a, b in zip(offs, offs[1:])]
    n_p = len(lens)
    src = torch.zeros(len(data) + src_off + 16, dtype=torch.uint8, device="cuda")
    src[src_off : src_off + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    d_offs = dev(np.array(offs, dtype=np.uint64))
    need = sum(lens) + 11 * n_p
    out_room = need if out_room is None else out_room
    sizes_room = n_p if sizes_room is None else sizes_room
    out, sizes, tot = guarded(out_room), guarded(4 * sizes_room), guarded(24)
    torch.cuda.synchronize()
    caller.zlib_ranges_device(src.data_ptr() + src_off, d_offs.data_ptr(), n_p, max_piece, out.data_ptr() if out_room else None, out_room,
                              sizes.data_ptr() if sizes_room else None, sizes_room, tot.data_ptr())
    torch.cuda.synchronize()
    h_out, h_sizes, h_tot = out.cpu().numpy(), sizes.cpu().numpy(), tot.cpu().numpy()
    totals = [int(v) for v in h_tot[:24].view(np.uint64)]
    assert (h_tot[24:] == GUARD).all() and (h_out[out_room:] == GUARD).all() and (h_sizes[4 * sizes_room :] == GUARD).all(), "written behind a room"
    assert totals[1] == n_p and totals[2] == 0
    if n_p > sizes_room:
        assert (h_sizes == GUARD).all(), "a room too small is not written at all"
        zs = None
    else:
        zs = h_sizes[: 4 * n_p].view(np.uint32).copy()
        assert int(zs.sum()) == totals[0]
    if totals[0] > out_room:
        assert (h_out == GUARD).all(), "a room too small is not written at all"
        return None, zs, totals, pieces
    assert (h_out[totals[0] : out_room] == GUARD).all(), "written behind the streams"
    blob = h_out[: totals[0]].tobytes()
    if zs is None:
        return blob, None, totals, pieces
    ends = np.cumsum(zs)
    return [blob[int(e - s) : int(e)] for s, e in zip(zs, ends)], zs, totals, pieces


def check_streams(streams, pieces):
    """Every stream is the zlib stream of its range: header, one final stored or dynamic block, Adler-32 (zlib verifies it), the size limit."""
    assert len(streams) == len(pieces)
    kinds = []
    for k, (s, want) in enumerate(zip(streams, pieces)):
        assert s[:2] == b"\x78\x9c" and s[2] & 1 == 1 and (s[2] >> 1) & 3 in (0, 2), (k, s[:3])
        assert len(s) <= len(want) + 11
        assert zlib.decompress(s) == want, k
        assert zlib.decompress(s[2:-4], -15) == want and int.from_bytes(s[-4:], "big") == zlib.adler32(want)
        kinds.append((s[2] >> 1) & 3)
    return kinds


def item_text(n_bytes, seed=8950):
    """A stream of items as the encoder's host form writes them, n_bytes of it."""
    out, x0 = [], 10_000
    rng = np.random.default_rng(seed)
    while sum(map(len, out)) < n_bytes:
        out.append(bigbed.blocks_recs_host(random_records(rng, 2000, x0), 1, {"contexts": 1}, None)[0])
        x0 += 2000
    return b"".join(out)[:n_bytes]


MIXED = [1, 11, 255, 256, 257, 8216, M - 1, M, 46, 100, 3, M]


@pytest.mark.parametrize("name", ["zeros", "random", "items", "one value"])
def test_ranges_of_mixed_lengths_in_one_call(caller, name):
    n = sum(MIXED)
    data = {"zeros": lambda: bytes(n), "random": lambda: np.random.default_rng(8951).integers(0, 256, n, dtype=np.uint8).tobytes(),
            "items": lambda: item_text(n), "one value": lambda: b"\xff" * n}[name]()
    for off in (0, 1, 2, 3):
        streams, zs, tot, pieces = zranges(caller, data, MIXED, M, off)
        kinds = check_streams(streams, pieces)
        assert tot == [sum(len(s) for s in streams), len(MIXED), 0] and [len(s) for s in streams] == [int(v) for v in zs]
        if name == "random":
            assert all(k == 0 for k in kinds) and [len(s) for s in streams] == [ln + 11 for ln in MIXED]  # stored
        if name in ("zeros", "one value"):
            assert kinds[MIXED.index(M)] == 2 and len(streams[MIXED.index(M)]) < M // 3
        if name == "items":
            assert kinds[MIXED.index(8216)] == 2 and len(streams[MIXED.index(8216)]) < 8216 // 2


def test_three_thousand_ranges_a_workgroup_loops(caller):
    rng = np.random.default_rng(8960)
    lens = [int(v) for v in rng.integers(1, 120, 3000)]
    data = item_text(sum(lens))
    streams, _, tot, pieces = zranges(caller, data, lens, 128, 3)
    check_streams(streams, pieces)
    assert tot[1] == 3000 and tot[0] < sum(lens) + 11 * 3000


def test_equal_length_ranges_give_the_pieces_call_s_bytes(caller):
    for piece, n_p in ((40, 300), (8216, 5), (M, 2)):
        data = item_text(piece * n_p, 8970 + n_p)
        streams, zs, tot, _ = zranges(caller, data, [piece] * n_p, piece, 1)
        src = torch.zeros(len(data) + 17, dtype=torch.uint8, device="cuda")
        src[1 : 1 + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
        out, sizes, t2 = guarded(len(data) + 11 * n_p), guarded(4 * n_p), guarded(16)
        caller.zlib_pieces_device(src.data_ptr() + 1, len(data), piece, out.data_ptr(), len(data) + 11 * n_p, sizes.data_ptr(), n_p, t2.data_ptr())
        torch.cuda.synchronize()
        want_tot = [int(v) for v in t2.cpu().numpy()[:16].view(np.uint64)]
        assert want_tot == tot[:2]
        assert out.cpu().numpy()[: tot[0]].tobytes() == b"".join(streams)
        assert sizes.cpu().numpy()[: 4 * n_p].view(np.uint32).tolist() == [int(v) for v in zs]


def test_ranges_each_room_one_short(caller):
    lens = [300, 46, 100, 2000, 1]
    data = item_text(sum(lens))
    streams, zs, tot, pieces = zranges(caller, data, lens, 2048)
    check_streams(streams, pieces)
    blob, zs2, tot2, _ = zranges(caller, data, lens, 2048, out_room=tot[0], sizes_room=len(lens))  # exactly enough
    assert b"".join(blob) == b"".join(streams) and tot2 == tot
    got = zranges(caller, data, lens, 2048, out_room=tot[0] - 1)
    assert got[0] is None and got[2] == tot and got[1].tolist() == zs.tolist()
    got = zranges(caller, data, lens, 2048, sizes_room=len(lens) - 1)
    assert got[1] is None and got[2] == tot and got[0] == b"".join(streams)
    got = zranges(caller, data, lens, 2048, out_room=0, sizes_room=0)
    assert got[:3] == (None, None, tot)


def test_a_range_of_no_byte_or_too_long_is_refused(caller):
    """A refusal, not a fault: the kernel reads nothing for a range without a byte (size 0) and cuts a range longer than max_piece at
    max_piece bytes — bytes of the range itself —, so every access stays inside the buffers the entry sized for max_piece; the entry
    reports BSC_ERR_ARG from the count.  The guard bytes stay, and the context goes on working."""
    data = item_text(4000)
    src = dev(np.frombuffer(data + bytes(16), dtype=np.uint8))
    for offs, max_piece, bad in (([0, 100, 100, 300], 256, 1), ([0, 100, 357, 400], 256, 1), ([0, 0, 257, 257, 300], 256, 3), ([0, 200, 100, 300], 256, 1)):
        n_p = len(offs) - 1
        d_offs = dev(np.array(offs, dtype=np.uint64))
        out, sizes, tot = guarded(4000 + 11 * n_p), guarded(4 * n_p), guarded(24)
        torch.cuda.synchronize()
        rc = caller._L.bsc_zlib_ranges_device(caller._h, src.data_ptr(), d_offs.data_ptr(), n_p, max_piece, out.data_ptr(), 4000 + 11 * n_p, sizes.data_ptr(),
                                              n_p, tot.data_ptr(), None)
        assert rc == -1 and b"ranges have no byte or more than max_piece" in caller._L.bsc_last_error()
        torch.cuda.synchronize()
        totals = [int(v) for v in tot.cpu().numpy()[:24].view(np.uint64)]
        assert totals[1] == n_p and totals[2] == bad and totals[0] <= sum(min(max(b - a, 0), max_piece) + 11 for a, b in zip(offs, offs[1:]))
        assert (tot.cpu().numpy()[24:] == GUARD).all() and (out.cpu().numpy()[4000 + 11 * n_p :] == GUARD).all() and (sizes.cpu().numpy()[4 * n_p :] == GUARD).all()
    L, h = caller._L, caller._h
    assert L.bsc_zlib_ranges_device(h, src.data_ptr(), d_offs.data_ptr(), 3, 0, out.data_ptr(), 100, sizes.data_ptr(), 3, tot.data_ptr(), None) == -1
    assert L.bsc_zlib_ranges_device(h, src.data_ptr(), d_offs.data_ptr(), 3, M + 1, out.data_ptr(), 100, sizes.data_ptr(), 3, tot.data_ptr(), None) == -1
    assert L.bsc_zlib_ranges_device(h, src.data_ptr(), d_offs.data_ptr() + 4, 3, 256, out.data_ptr(), 100, sizes.data_ptr(), 3, tot.data_ptr(), None) == -1
    assert L.bsc_zlib_ranges_device(h, None, d_offs.data_ptr(), 3, 256, out.data_ptr(), 100, sizes.data_ptr(), 3, tot.data_ptr(), None) == -1
    streams, _, _, pieces = zranges(caller, data, [100, 200, 256], 256)  # the context is usable
    check_streams(streams, pieces)
    t0 = guarded(24)
    caller.zlib_ranges_device(None, None, 0, 256, None, 0, None, 0, t0.data_ptr())  # no piece
    torch.cuda.synchronize()
    assert not t0.cpu().numpy()[:24].any() and (t0.cpu().numpy()[24:] == GUARD).all()


# ---- 8. the block entries -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The BAM of three contigs the methylation-table tests use: 6 000 positions at ~40x, one of 60 positions (a block shorter than a tile),
    and 30 000 positions covered thinly in several blocks."""
    d = tmp_path_factory.mktemp("bigbed_files")
    rng = np.random.default_rng(4711)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50)
            + W.wgbs_records(rng, reference["chrG"], 2, 60))
    refs = [(k, len(v)) for k, v in reference.items()]
    bam = str(d / "small.bam")
    W.write_bam(bam, refs, recs)
    return bam, refs, reference


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


@pytest.mark.parametrize("par", [{"contexts": 1}, {"min_cov": 12, "min_phred": 30, "pass_only": 1}])
def test_block_entries_behind_both_keep_calls(caller, small, par):
    """The block's stream and summaries are the Python rule's over the DECODED BCF of the same block (tests/methbed_ref.py's lines, cut into
    items here), the items re-joined are the block's own table, every block's zlib stream inflates to its bytes, and nothing else the block
    left changes: the kept stream, the table, the index entries, the regions' sums, the bigWig stream and summaries."""
    bam, refs, reference = small
    bbp, bwp = {"items_per_block": 50, "reduction": 128}, {"items_per_section": 50, "reduction": 128}
    n_blocks, seen = 0, 0
    flat = lambda g: (g[0], g[1], rows(g[2]), rows(g[3]))
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            ref = block_reference(codes, int(blk.x), int(blk.y))
            caller.meth_regions_attach([(0, len(codes))])
            # without the calls: the block, its table, its index entries, the regions' sums, its bigWig data
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
            table0 = caller.block_meth_kept(name, par)
            ent0 = caller.block_csi_kept(14)[0].tobytes()
            caller.block_meth_regions_kept(par)
            acc0 = caller.meth_regions_read().copy()
            caller.meth_regions_reset()
            bw0 = caller.block_bigwig_kept(tid, par, bwp)
            bw0 = (bw0[0], bw0[1], bw0[2].tobytes(), bw0[3].tobytes())
            # what the file itself says: the Python rule's lines over the DECODED BCF of the block, cut into items by the ITEM rule
            py_table = MB.of_bcf_stream(bcf0, name.encode(), par)
            assert py_table == table0[0]
            items = []
            for line in py_table.splitlines():
                contig, start, end, rest = line.split(b"\t", 3)
                assert contig == name.encode()
                items.append((int(start), struct.pack("<III", tid, int(start), int(end)) + rest + b"\0"))
            py = bigbed.blocks_of_items(items, 50, 128)
            want = (py[0], len(items), rows(py[1]), rows(py[2]))
            # before anything else is read
            caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
            got = caller.block_bigbed_kept(tid, par, bbp)
            assert flat(got) == want and bigbed.lines_of_stream(got[0], {tid: name.encode()}) == table0[0] and got[1] == table0[1]
            zblob, zs = caller.block_bigbed_deflate()
            offs, at = [b[4] for b in want[2]] + [len(want[0])], 0
            assert len(zs) == len(want[2])
            for k, size in enumerate(int(v) for v in zs):
                assert zlib.decompress(zblob[at : at + size]) == want[0][offs[k] : offs[k + 1]]
                at += size
            assert at == len(zblob)
            assert caller.block_csi_kept(14)[0].tobytes() == ent0 and caller.block_meth_kept(name, par) == table0 and kept_stream(caller, len(bcf0)) == bcf0
            caller.block_meth_regions_kept(par)
            assert (caller.meth_regions_read() == acc0).all()
            caller.meth_regions_reset()
            bw1 = caller.block_bigwig_kept(tid, par, bwp)
            assert (bw1[0], bw1[1], bw1[2].tobytes(), bw1[3].tobytes()) == bw0
            # after them, and twice
            assert flat(caller.block_bigbed_kept(tid, par, bbp)) == want == flat(caller.block_bigbed_kept(tid, par, bbp))
            assert caller.block_bigbed_deflate()[0] == zblob
            assert kept_stream(caller, len(bcf0)) == bcf0 and caller.block_meth_kept(name, par) == table0
            if want[0]:
                assert caller.bigbed_stream_read(8, 16) == want[0][8:24]
            # behind the text encoder's keep call
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, reg_stop=len(codes))
            assert flat(caller.block_bigbed_kept(tid, par, bbp)) == want
            assert kept_stream(caller, len(text)) == text and n_txt == n_rec and caller.block_meth_kept(name, par) == table0
            # B above the cap of a compressed file: the deflate refuses, the plain call does not
            assert flat(caller.block_bigbed_kept(tid, par, dict(bbp, items_per_block=bigbed.Z_ITEMS_MAX + 1)))[:2] == want[:2]
            with pytest.raises(B.BscError):
                caller.block_bigbed_deflate()
            seen += len(items)
            n_blocks += 1
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes))
            with pytest.raises(B.BscError):
                caller.block_bigbed_kept(tid, par, bbp)
            with pytest.raises(B.BscError):
                caller.block_bigbed_deflate()
    caller.meth_regions_attach([])
    assert n_blocks > 3 and seen > (100 if "min_cov" in par else 1000)


def test_deflate_without_a_kept_call_is_refused():
    with B.SiteCaller() as c:
        with pytest.raises(B.BscError):
            c.block_bigbed_deflate()
        with pytest.raises(B.BscError):
            c.block_bigbed_kept(0)
        with pytest.raises(B.BscError):
            c.bigbed_stream_read(0, 8)


# ---- 9. file to file ------------------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")


def run_exe(*args, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_bam2bcf_meth_bigbed_and_pipeline(caller, small, tmp_path):
    assert os.path.exists(EXE), "run `make demo`"
    bam, refs, reference = small
    fa = str(tmp_path / "small.fa")
    with open(fa, "w") as f:
        for nm, codes in reference.items():
            f.write(">%s\n" % nm)
            seq = "".join("NACGT"[c] for c in codes)
            for o in range(0, len(seq), 60):
                f.write(seq[o : o + 60] + "\n")
    p = lambda s: str(tmp_path / ("f" + s))
    common = ["--meth-all", "--meth-min-cov", "2", bam, fa]
    run_exe("--meth", p(".n.bed"), *common, p(".n.bcf"), p(".n.json"), "S9")  # without the switch
    opts = ["--meth-bigbed-items", "50", "--meth-bigbed-zoom", "8"]
    r0 = run_exe("--meth", p(".0.bed"), "--meth-bigbed", p(".0.bb"), *opts, *common, p(".0.bcf"), p(".0.json"), "S9")
    run_exe("--meth", p(".1.bed"), "--meth-bigbed", p(".1.bb"), "--meth-bigbed-compress", *opts, *common, p(".1.bcf"), p(".1.json"), "S9")
    for ext in (".bed", ".bcf", ".json"):  # every other output is what it is without the switch
        assert open(p(".0" + ext), "rb").read() == open(p(".n" + ext), "rb").read() == open(p(".1" + ext), "rb").read(), ext
    table = open(p(".n.bed"), "rb").read()
    assert bigbed.lines(p(".0.bb")) == table == bigbed.lines(p(".1.bb")) and table.count(b"\n") > 500
    assert "%d bedMethyl bigBed items written" % table.count(b"\n") in r0.stdout
    plain, comp = bigbed.read(p(".0.bb")), bigbed.read(p(".1.bb"))
    assert plain.header["uncompressBufSize"] == 0 and comp.header["uncompressBufSize"] in range(50 * bigbed.ITEM_MIN, max(50 * bigbed.ITEM_MAX, 32 * 512) + 1)
    assert plain.item_count == comp.item_count == table.count(b"\n") and plain.items_per_slot == comp.items_per_slot == 50
    assert plain.summary == comp.summary and plain.chroms == comp.chroms == {n: (k, l) for k, (n, l) in enumerate(refs)}
    assert len(plain.zooms) == len(comp.zooms) >= 2 and all(plain.zoom_records(l) == comp.zoom_records(l) for l in range(len(plain.zooms)))
    for name, length in refs:  # both files read the same through their R-trees, and as the table says
        want = [ln.split(b"\t", 3) for ln in table.splitlines() if ln.startswith(name.encode() + b"\t")]
        assert plain.entries(name) == comp.entries(name) == [(int(c[1]), int(c[2]), c[3]) for c in want]
        assert plain.entries(name, length // 3, length // 2) == comp.entries(name, length // 3, length // 2) == [
            (int(c[1]), int(c[2]), c[3]) for c in want if int(c[1]) < length // 2 and length // 3 < int(c[2])]
    assert os.path.getsize(p(".1.bb")) < os.path.getsize(p(".0.bb"))
    # pipeline.run gives the same files
    par = {"contexts": 1, "min_cov": 2}
    for z, ref_file in ((False, p(".0.bb")), (True, p(".1.bb"))):
        s = pipeline.run(bam, reference, p(".p.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, meth_params=par,
                         bigbed_path=p(".p.bb"), bigbed_items=50, bigbed_zoom=8, bigbed_compress=z)
        assert open(p(".p.bb"), "rb").read() == open(ref_file, "rb").read() and s["bigbed_items"] == plain.item_count
    # the refusals
    r = run_exe("--meth-bigbed", p(".no.bb"), "--meth-bigbed-compress", "--meth-bigbed-items", "653", bam, fa, p(".no.bcf"), p(".no.json"), ok=False)
    assert r.returncode == 2 and "652" in r.stderr
    for kw in (dict(bigbed_path=None), dict(bigbed_items=653), dict(device_reader=False), dict(bigbed_items=0, bigbed_compress=False)):
        with pytest.raises(ValueError):
            pipeline.run(bam, reference, p(".no"), **dict(dict(device_reader=True, bigbed_path=p(".no.bb"), bigbed_compress=True), **kw))
    assert not os.path.exists(p(".no.bb")) and not os.path.exists(p(".no.bcf")) and not os.path.exists(p(".no"))


# ---- 10. the ratio on item text ----------------------------------------------------------------------------------------------------------------------
def test_device_bytes_against_zlib_level_1_on_blocks_of_items(caller):
    """Blocks of 512 items of a seeded fixture, the device's streams against Python zlib level 1 over the same blocks.  The bigWig bound (1.05)
    was measured on binary sections; for item text the ratio was measured first (RATIO_MEASURED below) and is printed before it is asserted."""
    rng = np.random.default_rng(8990)
    recs = random_records(rng, 40_000, 100_000)
    data, blk, _ = bigbed.blocks_recs_host(recs, 1, {"contexts": 1}, None)
    offs = [int(b["off"]) for b in blk] + [len(data)]
    lens = [b - a for a, b in zip(offs, offs[1:])]
    assert len(lens) > 30 and max(lens) <= 512 * bigbed.ITEM_MAX <= M
    streams, _, tot, pieces = zranges(caller, data, lens, 512 * bigbed.ITEM_MAX)
    check_streams(streams, pieces)
    ref = sum(len(zlib.compress(p, 1)) for p in pieces)
    ratio = tot[0] / ref
    print("bigbed ratio: device %d bytes, zlib level 1 %d bytes, ratio %.4f, raw %d" % (tot[0], ref, ratio, len(data)))
    assert ratio <= RATIO_MEASURED + 0.03


# Measured on an MI355X on 2026-10-19: device 422 569 bytes, zlib level 1 431 160 bytes over the same 40 blocks (raw 1 209 948): 0.9801.  The
# encoder is deterministic; the margin of 0.03 covers a change of fixture only.
RATIO_MEASURED = 0.9801
