"""The coverage bigWig track on the device, alone and with the level track in one sweep (csrc/bwcovdev.hip: bsc_bwcov_write_kernel /
bsc_bwcov_reduce_kernel over the track mask, behind the tile, heads and windows kernels of csrc/bigwigdev.hip): streams, section and
window summaries and the six totals against the host forms (bsc_bigwig_cov_sections_recs, bsc_bigwig_sections_recs — which
tests/test_bigwig_cov_host.py and tests/test_bigwig_host.py hold to the Python rules) on dense arrays of random record contents: array
lengths around a tile, section sizes around their borders, window borders on and inside tiles, thresholds, positions up to 2^32 - 1, with
and without the chain's emit byte; the value float at every tie; sums of squares beyond 2^64 with the carry in the butterfly; the three
masks against each other and against bsc_bigwig_sites_device; each of the six rooms one short; the same at a one-CU grid; the block entry
behind both _keep calls against the Python rule over the DECODED BCF; and file to file (bam2bcf --cov-bigwig, pipeline.run) against
tests/bigwig_cov_ref.py.  Every comparison is of exact integers or bytes."""
import ctypes as C
import importlib.util
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import bigwig_cov_ref as RC
import bigwig_ref as R
import bs_call_amd as B
import methcpg_ref as MC
import methregions_ref as MR
from bs_call_amd import _lib, bigwig, methbed, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from methregions_ref import random_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cov_bigwig_model", os.path.join(ROOT, "tests", "test_gpu_bigwig.py"))
BW = importlib.util.module_from_spec(spec)  # the level track's test module: its helpers (dev, guarded, all_sites, the fixture files) are reused
spec.loader.exec_module(BW)
GUARD, TOP = BW.GUARD, 2**32 - 1
LEVEL, COV = _lib.BW_LEVEL, _lib.BW_COVERAGE
dev, guarded, all_sites, no_sites = BW.dev, BW.guarded, BW.all_sites, BW.no_sites


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


@pytest.fixture(scope="module")
def one_cu():
    """A context created under BSC_NUM_CUS=1 (bsc_create reads it once): grids of 8 workgroups, 32 waves."""
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


def params(bwp):
    return dict({"items_per_section": 1024, "reduction": 1024}, **(bwp or {}))


def host_tracks(recs, chrom_id, par, bwp, mask):
    """What a call with `mask` must leave: (level (bytes, sections, zoom0) or None, coverage likewise, the six totals)."""
    lv = bigwig.sections_recs_host(recs, chrom_id, par, bwp)
    cv = bigwig.sections_recs_host(recs, chrom_id, par, bwp, track="coverage")
    flat = lambda g: (g[0], R.sum_rows(g[1]), R.sum_rows(g[2]))
    sec = lv[1]
    tot = [len(lv[0]), int(sec["count"].sum()) if len(sec) else 0, len(sec), len(lv[2])]
    tot += [int(sec["sum_m"].sum()), int(sec["sum_m2"].sum())] if mask & LEVEL and len(sec) else [0, 0]
    return flat(lv) if mask & LEVEL else None, flat(cv) if mask & COV else None, tot


def full_rooms(n, bp):
    n_sec = -(-n // bp["items_per_section"])
    return (24 * n_sec + 8 * n, n_sec, n)


class Rooms:
    """The three guarded arrays of one track."""

    def __init__(self, rooms):
        self.rooms = rooms
        self.out, self.sec, self.zoom = guarded(rooms[0]), guarded(40 * rooms[1]), guarded(40 * rooms[2])

    def desc(self):
        return _lib.BwTrackOut(self.out.data_ptr(), self.rooms[0], self.sec.data_ptr(), self.rooms[1], self.zoom.data_ptr(), self.rooms[2])

    def read(self, totals):
        """(bytes, sections, zoom0), None for an array whose room was too small — which must then hold nothing but the guard."""
        res = []
        for buf, room, need, item in ((self.out, self.rooms[0], totals[0], 1), (self.sec, 40 * self.rooms[1], 40 * totals[2], 40),
                                      (self.zoom, 40 * self.rooms[2], 40 * totals[3], 40)):
            h = buf.cpu().numpy()
            assert (h[room:] == GUARD).all(), "written behind the room given"
            if need > room:
                assert (h == GUARD).all(), "a room too small is not written at all"
                res.append(None)
            else:
                res.append(h[:need].tobytes() if item == 1 else R.sum_rows(np.frombuffer(h[:need].tobytes(), dtype=bigwig.BW_SUM)))
        return tuple(res)


def device_tracks(caller, recs, x0, chrom_id=0, par=None, bwp=None, mask=3, rooms_l=None, rooms_c=None, emit=None):
    """bsc_bigwig_tracks_device over the records' two halves (emit given: the launcher behind it, bsc_dev_launch_bigwig_tracks, with the chain's
    byte per position, as the block entry hands it over).  Returns (level, coverage, totals) as host_tracks does."""
    n, bp = len(recs), params(bwp)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    L_ = Rooms(rooms_l or full_rooms(n, bp)) if mask & LEVEL else None
    C_ = Rooms(rooms_c or full_rooms(n, bp)) if mask & COV else None
    tot = guarded(48)
    if emit is None:
        caller.bigwig_tracks_device(d_core.data_ptr() if n else None, d_aux.data_ptr() if n else None, n, x0, chrom_id, mask, L_ and L_.desc(),
                                    C_ and C_.desc(), tot.data_ptr(), par, bp)
    else:
        L = caller._L
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.bsc_dev_launch_bigwig_tracks.restype = C.c_int
        L.bsc_dev_launch_bigwig_tracks.argtypes = [vp, vp, vp, u64, u32, u32, C.POINTER(_lib.MethParams), C.POINTER(_lib.BwParams), u32, vp, vp, vp, vp, vp, vp,
                                                   C.c_size_t, vp, vp, vp, C.POINTER(_lib.BwTrackOut), C.POINTER(_lib.BwTrackOut), vp, C.c_int, vp]
        L.bsc_dev_scan_tmp_bytes_u64.restype = C.c_int
        L.bsc_dev_scan_tmp_bytes_u64.argtypes = [C.c_uint32, C.POINTER(C.c_size_t)]
        n_tiles = (n + 63) // 64
        scan = C.c_size_t(0)
        assert L.bsc_dev_scan_tmp_bytes_u64(n_tiles + 1, C.byref(scan)) == 0
        d_emit = dev(emit)
        d_val = dev((np.arange(1001, dtype=np.float64) / 10.0).astype(np.float32))
        sizes = (8 * (n_tiles + 1),) * 4 + (scan.value, 8 * n, 4 * n, 4 * (n + 1))  # cnt, off, hcnt, hoff, scan, sites, cov, wbeg
        ws = [guarded(s) for s in sizes]
        torch.cuda.synchronize()
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        dl, dc = L_ and L_.desc(), C_ and C_.desc()
        rc = L.bsc_dev_launch_bigwig_tracks(d_core.data_ptr(), d_aux.data_ptr(), d_emit.data_ptr(), n, x0, chrom_id, C.byref(_lib.MethParams(**(par or {}))),
                                            C.byref(_lib.BwParams(**bp)), mask, d_val.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(),
                                            ws[3].data_ptr(), ws[4].data_ptr(), scan.value, ws[5].data_ptr(), ws[6].data_ptr(), ws[7].data_ptr(),
                                            dl and C.byref(dl), dc and C.byref(dc), tot.data_ptr(), cus, None)
        assert rc == 0
        torch.cuda.synchronize()
        for w, used in zip(ws, sizes):  # nothing behind the workspaces either
            assert (w.cpu().numpy()[used:] == GUARD).all()
    torch.cuda.synchronize()
    totals = [int(v) for v in tot.cpu().numpy().view(np.uint64)[:6]]
    assert (tot.cpu().numpy()[48:] == GUARD).all()
    return L_ and L_.read(totals), C_ and C_.read(totals), totals


def same_runs(level, cov):
    """Every start / end / count is equal between the two tracks."""
    assert len(level[0]) == len(cov[0])
    for a, b in ((level[1], cov[1]), (level[2], cov[2])):
        assert [r[:3] for r in a] == [r[:3] for r in b]


# ---- 1. array lengths, with and without the emit bytes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 20_003])
def test_array_lengths_with_and_without_the_emit_bytes(caller, n):
    rng = np.random.default_rng(9000 + n)
    x0, bwp = 1000, {"items_per_section": 5, "reduction": 16}
    recs = random_records(rng, n, x0, wide=True)
    for mask in (COV, 3):
        want = host_tracks(recs, 4, None, bwp, mask)
        assert device_tracks(caller, recs, x0, 4, None, bwp, mask) == want
    same_runs(want[0], want[1])
    assert want[2][2] > 1 and want[2][3] > 1
    emit = rng.choice([0, 1, 1, 1, 255], n).astype(np.uint8)  # the chain's byte per position: 0 takes a record away, whatever its own bytes say
    gated = recs.copy()
    c = gated["core"]
    c["emit"][emit == 0] = 0
    gated["core"] = c
    for mask in (COV, 3):
        want_e = host_tracks(gated, 4, None, bwp, mask)
        assert device_tracks(caller, recs, x0, 4, None, bwp, mask, emit=emit) == want_e
    sites = [(p - 1, min(a + b, TOP)) for p, a, b in MR.sites_of_rec_bytes(recs.tobytes(), None, emit)]
    assert want_e[1] == RC.block_entries(4, sites, 5, 16)  # the Python rule, from the record bytes
    assert want_e != want


# ---- 2. section sizes around their borders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 64, 65])
def test_section_sizes_and_site_counts(caller, S):
    rng = np.random.default_rng(9100 + S)
    for count in (S - 1, S, S + 1, 2 * S + 1):
        bwp = {"items_per_section": S, "reduction": 64}
        dense = all_sites(random_records(rng, max(count, 1), 77, wide=True))
        if count == 0:
            dense = no_sites(dense)
        thin = all_sites(random_records(rng, 3 * count + 1, 500, wide=True))  # a site every third position: ranks and positions part ways
        c = thin["core"]
        c["gt"][np.arange(len(thin)) % 3 != 1] = 0
        thin["core"] = c
        for recs, x0 in ((dense, 77), (thin, 500)):
            want = host_tracks(recs, 1, None, bwp, 3)
            assert want[2][1] == count and want[2][2] == -(-count // S)
            assert device_tracks(caller, recs, x0, 1, None, bwp, 3) == want
            assert device_tracks(caller, recs, x0, 1, None, bwp, COV) == (None, want[1], want[2][:4] + [0, 0])


# ---- 3. windows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("red", [1, 7, 64, 1024])
def test_reductions_with_borders_on_and_inside_tiles(caller, red):
    rng = np.random.default_rng(9200 + red)
    n = 64 * 37 + 5
    for x0 in (1, 30, 1000):  # x0 = 1: start = index, so a window of 64 or 1024 begins on a tile's border; the others begin inside a tile
        recs = random_records(rng, n, x0, wide=True)
        want = host_tracks(recs, 2, None, {"reduction": red}, 3)
        assert device_tracks(caller, recs, x0, 2, None, {"reduction": red}, 3) == want
        starts = [z[0] // red for z in want[1][2]]
        assert starts == sorted(set(starts)) and sum(z[2] for z in want[1][2]) == want[2][1] > 1000
        if red == 64 and x0 == 1:
            assert any(z[0] % 64 == 0 for z in want[1][2])
    assert device_tracks(caller, recs, x0, 2, None, {"reduction": red}, COV)[1] == want[1]


def test_thresholds_and_all_contexts(caller):
    rng = np.random.default_rng(9300)
    n, x0 = 1500, 4000
    recs = random_records(rng, n, x0, wide=True)
    bwp = {"items_per_section": 100, "reduction": 50}
    plain = device_tracks(caller, recs, x0, 0, None, bwp, 3)
    assert plain == host_tracks(recs, 0, None, bwp, 3)
    for par in ({"min_cov": 5}, {"min_phred": 100}, {"pass_only": 1}, {"contexts": 1}, {"contexts": 1, "min_cov": 3, "min_phred": 20, "pass_only": 1},
                {"min_cov": TOP}):  # (the last: a + b is compared in 64 bits, before the saturation)
        got = device_tracks(caller, recs, x0, 0, par, bwp, 3)
        assert got == host_tracks(recs, 0, par, bwp, 3) and got != plain, par
        assert 0 < got[2][1] and (got[2][1] > plain[2][1]) == (par == {"contexts": 1})
    assert device_tracks(caller, no_sites(recs.copy()), x0, 0, None, bwp, 3) == ((b"", [], []), (b"", [], []), [0] * 6)
    assert device_tracks(caller, recs[:0], x0, 0, None, bwp, COV) == (None, (b"", [], []), [0] * 6)  # no position either


def test_positions_up_to_the_top_of_the_range(caller):
    n = 197
    x0 = 2**32 - n  # the last position is 2^32 - 1, the last start 2^32 - 2
    rng = np.random.default_rng(9400)
    for recs in (all_sites(random_records(rng, n, x0, wide=True)), random_records(rng, n, x0, wide=True)):
        for bwp in ({"items_per_section": 10, "reduction": 64}, {"items_per_section": 65535, "reduction": 2**32 - 1}, {"items_per_section": 1, "reduction": 3}):
            want = host_tracks(recs, 7, None, bwp, 3)
            assert device_tracks(caller, recs, x0, 7, None, bwp, 3) == want
    assert want[1][1][-1][1] == 2**32 - 1 or want[2][1] < n


# ---- 4. the float -----------------------------------------------------------------------------------------------------------------------------
SUMS = [1, 2**24 - 1, 2**24, 2**24 + 1, 2**24 + 3, 2**25 + 2, 2**25 + 6, 2**31, 2**32 - 129, 2**32 - 128, 2**32 - 1, 2**32, 2**33 - 2]


def test_the_value_float_at_every_tie(caller):
    n = 3 * len(SUMS) + 70  # the sums at the front, across a tile's border, and once more behind it
    sums = (SUMS * 3 + [5] * 70)[:n]
    sums[64:64 + len(SUMS)] = SUMS
    a = np.array([v // 2 for v in sums], dtype=np.uint64)
    b = np.array([v - v // 2 for v in sums], dtype=np.uint64)
    recs = all_sites(random_records(np.random.default_rng(9500), n, 10), a=a.astype(np.uint32), b=b.astype(np.uint32))
    bwp = {"items_per_section": 40, "reduction": 1}
    want = host_tracks(recs, 0, None, bwp, 3)
    got = device_tracks(caller, recs, 10, 0, None, bwp, 3)
    assert got == want and device_tracks(caller, recs, 10, 0, None, bwp, COV)[1] == want[1]
    c = np.array([min(v, TOP) for v in sums], dtype=np.uint32)
    floats = c.astype(np.float32)  # numpy's u32 -> f32
    stream = got[1][0]
    for i in range(n):
        k, j = divmod(i, 40)
        at = k * (24 + 8 * 40) + 24 + 8 * j
        assert stream[at : at + 8] == np.uint32(9 + i).tobytes() + floats[i].tobytes() == np.uint32(9 + i).tobytes() + RC.f32(int(c[i])), (i, sums[i])
    assert [z[3] for z in got[1][2]] == [int(v) for v in c]  # one window a site: min c = c


# ---- 5. the wide sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [64, 65, 70])
def test_sums_of_squares_beyond_2_64_in_one_section_and_window(caller, count):
    n, x0 = 200, 1025  # starts 1024 .. 1223: one window of 1024, in four tiles; the sites of c = 2^32 - 1 lie across the border of tiles 0 and 1
    recs = random_records(np.random.default_rng(9600 + count), n, x0)
    recs = no_sites(recs)
    c = recs["core"]
    c["gt"][30 : 30 + count] = 4
    c["emit"], c["cg"], c["flt"], c["phred"] = 1, b"C", 0, 99
    recs["core"] = c
    recs["counts"][30 : 30 + count] = TOP  # a = b = 2^32 - 1: a + b saturates
    bwp = {"items_per_section": 128, "reduction": 1024}
    want = host_tracks(recs, 0, None, bwp, 3)
    sq = count * TOP * TOP
    assert want[1][1] == want[1][2] == [(1054, 1054 + count, count, TOP, TOP, sq >> 64, count * TOP, sq % 2**64)] and sq >> 64 == count - 1
    assert device_tracks(caller, recs, x0, 0, None, bwp, 3) == want
    assert device_tracks(caller, recs, x0, 0, None, bwp, COV) == (None, want[1], want[2][:4] + [0, 0])


def test_a_carry_on_the_last_merge_step_alone(caller):
    """64 sites in one section and one window, lane = rank: c = 2^31 (c * c = 2^62) in lanes 0, 1, 32 and 33, c = 1 elsewhere.  Each half of
    the wave adds up to 2^63 + 30 without a carry; the butterfly's last step (lanes 32 apart) gives 2^64 + 60: the one carry."""
    n, x0 = 64, 1
    recs = all_sites(random_records(np.random.default_rng(9700), n, x0), a=0, b=1)
    for i in (0, 1, 32, 33):
        recs["counts"][i] = 2**30  # a = b = 2^30
    bwp = {"items_per_section": 64, "reduction": 1024}
    want = host_tracks(recs, 0, None, bwp, 3)
    assert want[1][1] == want[1][2] == [(0, 64, 64, 1, 2**31, 1, 4 * 2**31 + 60, 60)]
    assert device_tracks(caller, recs, x0, 0, None, bwp, 3) == want
    assert device_tracks(caller, recs, x0, 0, None, bwp, COV) == (None, want[1], want[2][:4] + [0, 0])


# ---- 6. the mask ------------------------------------------------------------------------------------------------------------------------------
def test_masks_against_each_other_and_against_the_level_entry(caller):
    rng = np.random.default_rng(9800)
    n, x0 = 64 * 21 + 9, 300
    recs = random_records(rng, n, x0, wide=True)
    bwp = {"items_per_section": 16, "reduction": 32}
    old = BW.device_block(caller, recs, x0, 5, None, bwp)  # bsc_bigwig_sites_device: (bytes, sections, zoom0, totals)
    m1 = device_tracks(caller, recs, x0, 5, None, bwp, LEVEL)
    m2 = device_tracks(caller, recs, x0, 5, None, bwp, COV)
    m3 = device_tracks(caller, recs, x0, 5, None, bwp, 3)
    assert m1 == (old[:3], None, old[3]) and old[3][4] > 0
    assert m3[0] == m1[0] and m3[1] == m2[1] and m3[2] == m1[2] and m2[2] == m1[2][:4] + [0, 0]
    same_runs(m3[0], m3[1])
    assert m3 == host_tracks(recs, 5, None, bwp, 3)
    # a track of the mask without a descriptor, a mask that is none: refused, nothing written, the context usable
    L, h = caller._L, caller._h
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    room, tot = Rooms(full_rooms(n, params(bwp))), guarded(48)
    d, mp, bp = room.desc(), _lib.MethParams(), _lib.BwParams(16, 32)
    f = lambda mask, lv, cv, x=x0: L.bsc_bigwig_tracks_device(h, d_core.data_ptr(), d_aux.data_ptr(), n, x, 5, C.byref(mp), C.byref(bp), mask, lv, cv, tot.data_ptr(), None)
    for mask, lv, cv in ((1, None, C.byref(d)), (2, C.byref(d), None), (3, C.byref(d), None), (3, None, C.byref(d)), (0, C.byref(d), C.byref(d)),
                         (4, C.byref(d), C.byref(d))):
        assert f(mask, lv, cv) == -1, mask
    assert b"tracks is 4" in L.bsc_last_error()
    assert f(3, C.byref(d), C.byref(d), 0) == -1 and b"1-based" in L.bsc_last_error()
    odd = _lib.BwTrackOut(room.out.data_ptr() + 4, 8, room.sec.data_ptr(), 0, room.zoom.data_ptr(), 0)
    assert f(2, None, C.byref(odd)) == -1 and b"8-byte" in L.bsc_last_error()
    torch.cuda.synchronize()
    assert (room.out.cpu().numpy() == GUARD).all() and (tot.cpu().numpy() == GUARD).all()
    assert device_tracks(caller, recs, x0, 5, None, bwp, 3) == m3


# ---- 7. each of the six rooms one short -------------------------------------------------------------------------------------------------------
def test_each_of_the_six_rooms_one_short(caller):
    rng = np.random.default_rng(9900)
    n, x0 = 700, 50
    recs = random_records(rng, n, x0, wide=True)
    bwp = {"items_per_section": 16, "reduction": 32}
    want = host_tracks(recs, 3, None, bwp, 3)
    exact = (want[2][0], want[2][2], want[2][3])
    assert min(exact) > 10
    assert device_tracks(caller, recs, x0, 3, None, bwp, 3, exact, exact) == want  # exactly enough
    for k in range(6):
        short = tuple(v - (1 if j == k % 3 else 0) for j, v in enumerate(exact))
        got = device_tracks(caller, recs, x0, 3, None, bwp, 3, short if k < 3 else exact, exact if k < 3 else short)  # (the guard bytes are checked inside)
        assert got[2] == want[2]  # the needs, and the sums, are reported all the same
        hit, other = (got[0], got[1]) if k < 3 else (got[1], got[0])
        assert other == (want[1] if k < 3 else want[0])  # the other track is complete
        assert hit[k % 3] is None and [g for j, g in enumerate(hit) if j != k % 3] == [w for j, w in enumerate(want[k // 3]) if j != k % 3]
    assert device_tracks(caller, recs, x0, 3, None, bwp, 3, (0, 0, 0), exact) == ((None, None, None), want[1], want[2])
    assert device_tracks(caller, recs, x0, 3, None, bwp, COV, None, (0, 0, 0)) == (None, (None, None, None), want[2][:4] + [0, 0])


# ---- 8. a one-CU grid -------------------------------------------------------------------------------------------------------------------------
def test_one_cu_grid(caller, one_cu):
    rng = np.random.default_rng(10000)
    # 6 300 positions: three rounds of the 2 048-position grid and a ragged fourth; sections + windows far beyond the 32 waves of the reduction
    for n, bwp in ((6_300, {"items_per_section": 7, "reduction": 5}), (200, {"items_per_section": 1, "reduction": 1}),
                   (6_300, {"items_per_section": 1024, "reduction": 1024})):
        recs = random_records(rng, n, 123, wide=True)
        want = host_tracks(recs, 1, None, bwp, 3)
        if n == 200:
            assert want[2][2] + want[2][3] > 32
        for mask in (LEVEL, COV, 3):
            small = device_tracks(one_cu, recs, 123, 1, None, bwp, mask)
            assert small == device_tracks(caller, recs, 123, 1, None, bwp, mask)
            if mask == 3:
                assert small == want
    exact = (want[2][0], want[2][2], want[2][3])
    short = (exact[0] - 1, exact[1], exact[2])
    got = device_tracks(one_cu, recs, 123, 1, None, bwp, 3, exact, short)
    assert got == (want[0], (None,) + want[1][1:], want[2])


# ---- 9. the block entry -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """A BAM of three contigs: 6 000 positions at ~40x, one of 60 positions (a block shorter than a tile), 30 000 positions covered thinly."""
    d = tmp_path_factory.mktemp("bigwig_cov_files")
    rng = np.random.default_rng(4712)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (BW.W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + BW.W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50)
            + BW.W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = BW._fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def inflate_sections(zdata, sizes):
    out, at = [], 0
    for s in sizes:
        d = zlib.decompressobj()
        out.append(d.decompress(zdata[at : at + int(s)]))  # (zlib verifies the Adler-32 at the stream's end)
        assert d.eof and not d.unused_data
        at += int(s)
    assert at == len(zdata)
    return b"".join(out)


@pytest.mark.parametrize("par", [{}, {"min_cov": 12, "min_phred": 30, "pass_only": 1}])
def test_block_entry_behind_both_keep_calls(caller, small, par):
    _, bam, _, refs, reference = small
    S, red = 50, 128
    bwp = {"items_per_section": S, "reduction": red}
    n_blocks, seen, cur = 0, 0, None
    flat = lambda g: None if g is None else (g[0], R.sum_rows(g[1]), R.sum_rows(g[2]))
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            ref = block_reference(codes, int(blk.x), int(blk.y))
            if name != cur:
                cur = name
                caller.meth_regions_attach(sorted([(0, len(codes))] + [(s, min(s + 100, len(codes))) for s in range(0, len(codes), 100)]))
            # without the call: the block, its table and its tabix scan, its index entries, the regions' sums, the bigBed items, the level entry's outputs
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
            table0 = caller.block_meth_kept(name, par)
            tbx0 = caller.block_meth_index_kept(14)
            tbx0 = (tbx0[0].tobytes(), tbx0[1])  # the tabix scan of that table
            ent0 = caller.block_csi_kept(14)[0].tobytes()
            caller.block_meth_regions_kept(par)
            acc0 = caller.meth_regions_read().copy()
            caller.meth_regions_reset()
            bb0 = caller.block_bigbed_kept(tid, par)
            bb0 = (bb0[0], bb0[1], bb0[2].tobytes(), bb0[3].tobytes())
            old = caller.block_bigwig_kept(tid, par, bwp)
            old_z = caller.block_bigwig_deflate()
            old = (old[0], R.sum_rows(old[2]), R.sum_rows(old[3]))
            decoded = [s for s in (MR.sites_of_bcf_record(d, par) for d in MC.bcf_records(bcf0)) if s is not None]
            cov_sites = [(p - 1, min(a + b, TOP)) for p, a, b in decoded]
            lv_sites = [(p - 1, BW.m_of(a, b)) for p, a, b in decoded]
            want_c = RC.block_entries(tid, cov_sites, S, red)  # what the file itself says
            py = bigwig.sections_of_sites(lv_sites, tid, S, red)
            want_l = (py[0], R.sum_rows(py[1]), R.sum_rows(py[2]))
            assert old == want_l
            for mask in (LEVEL, COV, 3):
                caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
                ns, lv, cv = caller.block_bigwig_tracks_kept(tid, mask, par, bwp)
                assert ns == len(decoded) and flat(lv) == (want_l if mask & LEVEL else None) and flat(cv) == (want_c if mask & COV else None)
                if mask & LEVEL:  # the level buffers are those of bsc_block_bigwig_kept: the reads and the deflate behind it give what they gave
                    assert caller.bigwig_stream_read(0, len(want_l[0])) == want_l[0]
                    z = caller.block_bigwig_deflate()
                    assert z[0] == old_z[0] and (z[1] == old_z[1]).all()
                else:
                    with pytest.raises(B.BscError):
                        caller.block_bigwig_deflate()
                if mask & COV:
                    zdata, zs = caller.block_bigwig_cov_deflate()
                    assert len(zs) == len(want_c[1]) and inflate_sections(zdata, zs) == want_c[0]
                    if want_c[0]:
                        assert caller.bigwig_cov_stream_read(8, 16) == want_c[0][8:24]
                else:
                    with pytest.raises(B.BscError):
                        caller.block_bigwig_cov_deflate()
                # everything else the block left is as it was
                assert caller.block_csi_kept(14)[0].tobytes() == ent0 and caller.block_meth_kept(name, par) == table0 and BW.kept_stream(caller, len(bcf0)) == bcf0
                tbx = caller.block_meth_index_kept(14)
                assert (tbx[0].tobytes(), tbx[1]) == tbx0
                caller.block_meth_regions_kept(par)
                assert (caller.meth_regions_read() == acc0).all()
                caller.meth_regions_reset()
                bb = caller.block_bigbed_kept(tid, par)
                assert (bb[0], bb[1], bb[2].tobytes(), bb[3].tobytes()) == bb0
            # behind the text encoder's keep call, and twice
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, reg_stop=len(codes))
            first = caller.block_bigwig_tracks_kept(tid, 3, par, bwp)
            assert (first[0], flat(first[1]), flat(first[2])) == (len(decoded), want_l, want_c)
            again = caller.block_bigwig_tracks_kept(tid, 3, par, bwp)
            assert (again[0], flat(again[1]), flat(again[2])) == (len(decoded), want_l, want_c)
            assert BW.kept_stream(caller, len(text)) == text and n_txt == n_rec
            # the level entry behind it leaves no coverage stream to read or deflate
            caller.block_bigwig_kept(tid, par, bwp)
            with pytest.raises(B.BscError):
                caller.block_bigwig_cov_deflate()
            seen += len(decoded)
            n_blocks += 1
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes))
            with pytest.raises(B.BscError, match="no single block"):
                caller.block_bigwig_tracks_kept(tid, 3, par, bwp)
    caller.meth_regions_attach([])
    assert n_blocks > 3 and seen > (100 if par else 1000)


# ---- 10. file to file -------------------------------------------------------------------------------------------------------------------------
def cov_blocks_of_table(rows, refs, cuts):
    """The (tid, [(start, c)]) blocks of a per-cytosine table's rows, cut where the reader cut its blocks: cuts = [(tid, x, y)]."""
    out = []
    for tid, x, y in cuts:
        mine = rows[(rows["chrom"] == refs[tid][0]) & (rows["start"] + 1 >= x) & (rows["start"] + 1 <= y)]
        out.append((tid, [(int(r["start"]), min(int(r["a"]) + int(r["b"]), TOP)) for r in mine]))
    return out


def test_bam2bcf_cov_bigwig_and_pipeline(caller, small):
    assert os.path.exists(BW.EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("c" + s))
    rd_ = lambda s: open(p(s), "rb").read()
    with DeviceBamReader(caller, bam, threads=2) as rd:
        cuts = [(int(b.tid), int(b.x), int(b.y)) for b in rd.device_blocks()]
    assert len(cuts) > 3
    geo = ["--meth-bigwig-section", "50", "--meth-bigwig-zoom", "8"]
    # the run without the switch, and with it: every other output byte-identical
    base = BW.run_exe("--meth", p(".0.meth"), "--meth-bigwig", p(".0.bw"), *geo, bam, fa, p(".0.bcf"), p(".0.json"), "S9").stdout
    r = BW.run_exe("--meth", p(".1.meth"), "--meth-bigwig", p(".1.bw"), "--cov-bigwig", p(".1.cov"), *geo, bam, fa, p(".1.bcf"), p(".1.json"), "S9")
    for ext in (".meth", ".bw", ".bcf", ".json"):
        assert rd_(".1" + ext) == rd_(".0" + ext), ext
    rows = methbed.read_bed(p(".1.meth"))
    blocks = cov_blocks_of_table(rows, refs, cuts)
    got = rd_(".1.cov")
    assert got == RC.build(refs, blocks, 50, 8)
    assert r.stdout == base + "%d coverage bigWig sites written\n" % len(rows)
    f = bigwig.BigWig(got)
    assert f.header["zoomLevels"] >= 2 and f.summary["basesCovered"] == len(rows) > 300
    col10 = [line.split(b"\t")[9] for line in rd_(".1.meth").splitlines() if line and not line.startswith((b"#", b"track"))]  # bedMethyl's coverage column
    every = [v for name, _ in refs for _, _, v in f.intervals(name)]
    assert [s for name, _ in refs for s, _, _ in f.intervals(name)] == [int(v) for v in rows["start"]]
    assert [np.float32(v).tobytes() for v in every] == [RC.f32(min(int(c), TOP)) for c in col10]
    # the switch alone: the same coverage file, the other outputs those of the plain run
    BW.run_exe(bam, fa, p(".2.bcf"), p(".2.json"), "S9")
    r = BW.run_exe("--cov-bigwig", p(".3.cov"), *geo, bam, fa, p(".3.bcf"), p(".3.json"), "S9")
    assert rd_(".3.cov") == got and rd_(".3.bcf") == rd_(".2.bcf") and rd_(".3.json") == rd_(".2.json")
    assert r.stdout.endswith("%d coverage bigWig sites written\n" % len(rows)) and "methylation bigWig" not in r.stdout
    # compressed: both files, the level file that of the run without --cov-bigwig
    BW.run_exe("--meth-bigwig", p(".4.bw"), "--meth-bigwig-compress", *geo, bam, fa, p(".4.bcf"), p(".4.json"), "S9")
    BW.run_exe("--meth-bigwig", p(".5.bw"), "--cov-bigwig", p(".5.cov"), "--meth-bigwig-compress", *geo, bam, fa, p(".5.bcf"), p(".5.json"), "S9")
    assert rd_(".5.bw") == rd_(".4.bw") and rd_(".5.bcf") == rd_(".2.bcf")
    RC.check_z(rd_(".5.cov"), refs, blocks, 50, 8)
    fz = bigwig.BigWig(rd_(".5.cov"))
    assert fz.summary == f.summary and [fz.intervals(n) for n, _ in refs] == [f.intervals(n) for n, _ in refs] and len(rd_(".5.cov")) < len(got)
    BW.run_exe("--cov-bigwig", p(".6.cov"), "--meth-bigwig-compress", *geo, bam, fa, p(".6.bcf"), p(".6.json"), "S9")
    assert rd_(".6.cov") == rd_(".5.cov")
    # pipeline.run writes the same files
    s = pipeline.run(bam, reference, p(".p1.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, bigwig_path=p(".p1.bw"),
                     cov_bigwig_path=p(".p1.cov"), bigwig_section=50, bigwig_zoom=8, meth_path=p(".p1.meth"))
    assert rd_(".p1.cov") == got and rd_(".p1.bw") == rd_(".0.bw") and s["cov_bigwig_sites"] == len(rows) == s["bigwig_sites"]
    assert rd_(".p1.bcf") == rd_(".0.bcf") and rd_(".p1.meth") == rd_(".0.meth")
    s = pipeline.run(bam, reference, p(".p2.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, cov_bigwig_path=p(".p2.cov"),
                     bigwig_section=50, bigwig_zoom=8, bigwig_compress=True)
    assert rd_(".p2.cov") == rd_(".5.cov") and "bigwig_sites" not in s
    pipeline.run(bam, reference, p(".p3.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, bigwig_path=p(".p3.bw"),
                 cov_bigwig_path=p(".p3.cov"), bigwig_section=50, bigwig_zoom=8, bigwig_compress=True)
    assert rd_(".p3.cov") == rd_(".5.cov") and rd_(".p3.bw") == rd_(".4.bw")
    # the thresholds apply: the coverage of the table the same thresholds give
    th = ["--meth-min-cov", "12", "--meth-min-gq", "30", "--meth-pass", "--meth-all"]
    BW.run_exe(*th, "--meth", p(".t.meth"), "--cov-bigwig", p(".t.cov"), bam, fa, p(".t.bcf"), p(".t.json"), "S9")
    rows_t = methbed.read_bed(p(".t.meth"))
    assert rd_(".t.cov") == RC.build(refs, cov_blocks_of_table(rows_t, refs, cuts), 1024, 1024) != RC.build(refs, blocks, 1024, 1024)
    # the refusals
    for extra in (["--rank", "0", "--world", "2"], ["--merge", "2"]):
        r = BW.run_exe("--cov-bigwig", p(".no.cov"), *extra, bam, fa, p(".no.bcf"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--cov-bigwig writes a single run's track" in r.stderr
    r = BW.run_exe("--cov-bigwig", p(".no.cov"), "--meth-bigwig-compress", "--meth-bigwig-section", "8158", bam, fa, p(".no.bcf"), p(".no.json"), ok=False)
    assert r.returncode == 2 and "8157" in r.stderr
    for var in ("BAM2BCF_HOST_READER", "BAM2BCF_HOST_BCF", "BAM2BCF_HOST_PREP"):
        r = subprocess.run([BW.EXE, "--cov-bigwig", p(".no.cov"), bam, fa, p(".no.bcf"), p(".no.json")], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, **{var: "1"}))
        assert r.returncode == 2 and "--cov-bigwig" in r.stderr
    for kw in (dict(device_reader=False), dict(shard_rank=0, shard_world=2), dict(bigwig_section=0), dict(bigwig_section=65536), dict(bigwig_zoom=0),
               dict(bigwig_compress=True, bigwig_section=8158)):
        with pytest.raises(ValueError):
            pipeline.run(bam, reference, p(".no"), **dict(dict(device_reader=True, cov_bigwig_path=p(".no.cov")), **kw))
    assert not os.path.exists(p(".no")) and not os.path.exists(p(".no.cov")) and not os.path.exists(p(".no.bcf"))
