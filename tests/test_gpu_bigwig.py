"""The methylation bigWig track on the device (csrc/bigwigdev.hip: the bsc_bigwig_*_kernel family): the block's data stream, the sections'
and the level-0 windows' summaries and the six totals against the host form (bsc_bigwig_sections_recs, which tests/test_bigwig_host.py
holds to the Python rule) on dense arrays of random record contents — every array length around a tile, every section size around its
border, window borders on and inside tiles, positions up to 2^32 - 1, with and without the chain's emit byte, under the thresholds, with
each room one short —, against bsc_meth_sites_device's line count, the block entry behind both _keep calls against the Python rule over the
DECODED BCF of the same block, and file to file (bam2bcf --meth-bigwig, pipeline.run(bigwig_path=...)) against tests/bigwig_ref.py.  Every
comparison is of exact integers or bytes."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bigwig_ref as R
import bs_call_amd as B
import methcpg_ref as RC
import methregions_ref as MR
from bs_call_amd import _lib, bigwig, methbed, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from methregions_ref import random_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
GUARD = 0xA5


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def guarded(n_bytes):
    """Room of n_bytes on the device with 64 guard bytes behind it (and at least 16 bytes in all), filled with the guard value."""
    return torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device="cuda")


def all_sites(recs, a=None, b=None):
    """Every record a site under the default parameters."""
    c = recs["core"]
    c["emit"], c["gt"], c["cg"] = 1, np.where(np.arange(len(recs)) % 3 == 0, 7, 4), b"C"
    recs["core"] = c
    recs["counts"] = np.maximum(recs["counts"], 1)
    if a is not None:
        recs["counts"][:, 5], recs["counts"][:, 6], recs["counts"][:, 7], recs["counts"][:, 4] = a, a, b, b
    return recs


def no_sites(recs):
    c = recs["core"]
    c["gt"] = 5
    recs["core"] = c
    return recs


def host_block(recs, chrom_id, par, bwp):
    raw, sec, zoom = bigwig.sections_recs_host(recs, chrom_id, par, bwp)
    tot = [len(raw), int(sec["count"].sum()) if len(sec) else 0, len(sec), len(zoom), int(sec["sum_m"].sum()) if len(sec) else 0,
           int(sec["sum_m2"].sum()) if len(sec) else 0]
    return raw, R.sum_rows(sec), R.sum_rows(zoom), tot


def unpack(out, sec, zoom, tot, rooms):
    """The device buffers as (bytes, sections, zoom0, totals); the guard bytes behind every room are checked here."""
    torch.cuda.synchronize()
    totals = [int(v) for v in tot.cpu().numpy().view(np.uint64)[:6]]
    assert (tot.cpu().numpy()[48:] == GUARD).all()
    res = []
    for buf, room, need, item in ((out, rooms[0], totals[0], 1), (sec, 40 * rooms[1], 40 * totals[2], 40), (zoom, 40 * rooms[2], 40 * totals[3], 40)):
        h = buf.cpu().numpy()
        assert (h[room:] == GUARD).all(), "written behind the room given"
        if need > room:
            assert (h == GUARD).all(), "a room too small is not written at all"
            res.append(None)
        else:
            res.append(h[:need].tobytes() if item == 1 else R.sum_rows(np.frombuffer(h[:need].tobytes(), dtype=bigwig.BW_SUM)))
    return res[0], res[1], res[2], totals


def device_block(caller, recs, x0, chrom_id=0, par=None, bwp=None, rooms=None):
    """bsc_bigwig_sites_device over the records' two halves.  rooms: (bytes, sections, windows); default: what every position a site needs."""
    n = len(recs)
    bp = dict({"items_per_section": 1024, "reduction": 1024}, **(bwp or {}))
    if rooms is None:
        n_sec = -(-n // bp["items_per_section"])
        rooms = (24 * n_sec + 8 * n, n_sec, n)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    out, sec, zoom, tot = guarded(rooms[0]), guarded(40 * rooms[1]), guarded(40 * rooms[2]), guarded(48)
    caller.bigwig_sites_device(d_core.data_ptr() if n else None, d_aux.data_ptr() if n else None, n, x0, chrom_id, out.data_ptr(), rooms[0], sec.data_ptr(),
                               rooms[1], zoom.data_ptr(), rooms[2], tot.data_ptr(), par, bp)
    return unpack(out, sec, zoom, tot, rooms)


def launch_with_emit(caller, recs, emit, x0, chrom_id=0, par=None, bwp=None):
    """The launcher behind the two entries (bsc_dev_launch_bigwig) with the chain's emit byte per position, as bsc_block_bigwig_kept hands it
    over — the public per-position entry has no such array."""
    L = caller._L
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.bsc_dev_launch_bigwig.restype = C.c_int
    L.bsc_dev_launch_bigwig.argtypes = [vp, vp, vp, u64, u32, u32, C.POINTER(_lib.MethParams), C.POINTER(_lib.BwParams), vp, vp, vp, vp, vp, vp, C.c_size_t,
                                        vp, vp, vp, u64, vp, u64, vp, u64, vp, C.c_int, vp]
    L.bsc_dev_scan_tmp_bytes_u64.restype = C.c_int
    L.bsc_dev_scan_tmp_bytes_u64.argtypes = [C.c_uint32, C.POINTER(C.c_size_t)]
    n = len(recs)
    n_tiles = (n + 63) // 64
    scan = C.c_size_t(0)
    assert L.bsc_dev_scan_tmp_bytes_u64(n_tiles + 1, C.byref(scan)) == 0
    bp = _lib.BwParams(**dict({"items_per_section": 1024, "reduction": 1024}, **(bwp or {})))
    n_sec = -(-n // bp.items_per_section)
    rooms = (24 * n_sec + 8 * n, n_sec, n)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux, d_emit = dev(raw[:, :64]), dev(raw[:, 64:]), dev(emit)
    d_val = dev((np.arange(1001, dtype=np.float64) / 10.0).astype(np.float32))
    ws = [guarded(8 * (n_tiles + 1)) for _ in range(4)] + [guarded(scan.value), guarded(8 * n), guarded(4 * (n + 1))]
    out, sec, zoom, tot = guarded(rooms[0]), guarded(40 * rooms[1]), guarded(40 * rooms[2]), guarded(48)
    torch.cuda.synchronize()
    mp = _lib.MethParams(**(par or {}))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc = L.bsc_dev_launch_bigwig(d_core.data_ptr(), d_aux.data_ptr(), d_emit.data_ptr(), n, x0, chrom_id, C.byref(mp), C.byref(bp), d_val.data_ptr(),
                                 ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr(), ws[3].data_ptr(), ws[4].data_ptr(), scan.value, ws[5].data_ptr(),
                                 ws[6].data_ptr(), out.data_ptr(), rooms[0], sec.data_ptr(), rooms[1], zoom.data_ptr(), rooms[2], tot.data_ptr(), cus, None)
    assert rc == 0
    got = unpack(out, sec, zoom, tot, rooms)
    for w, used in zip(ws, (8 * (n_tiles + 1),) * 4 + (scan.value, 8 * n, 4 * (n + 1))):  # nothing behind the workspaces either
        assert (w.cpu().numpy()[used:] == GUARD).all()
    return got


# ---- 1. array lengths, with and without the emit bytes ----------------------------------------------------------------------------------------
LENGTHS = [1, 63, 64, 65, 129, 64 * 37 + 5]


@pytest.mark.parametrize("n", LENGTHS)
def test_array_lengths_with_and_without_the_emit_bytes(caller, n):
    rng = np.random.default_rng(7000 + n)
    x0, bwp = 1000, {"items_per_section": 5, "reduction": 16}
    recs = random_records(rng, n, x0, wide=True)
    want = host_block(recs, 4, None, bwp)
    assert device_block(caller, recs, x0, 4, None, bwp) == want
    if n > 64:
        assert want[3][2] > 1 and want[3][3] > 1
    emit = rng.choice([0, 1, 1, 1, 255], n).astype(np.uint8)  # the chain's byte per position: 0 takes a record away, whatever its own bytes say
    gated = recs.copy()
    c = gated["core"]
    c["emit"][emit == 0] = 0
    gated["core"] = c
    want_e = host_block(gated, 4, None, bwp)
    assert launch_with_emit(caller, recs, emit, x0, 4, None, bwp) == want_e
    sites = [(p - 1, (2000 * a + a + b) // (2 * (a + b))) for p, a, b in MR.sites_of_rec_bytes(recs.tobytes(), None, emit)]
    py = bigwig.sections_of_sites(sites, 4, 5, 16)
    assert want_e[:3] == (py[0], R.sum_rows(py[1]), R.sum_rows(py[2]))
    if n >= 64:
        assert want_e != want


# ---- 2. section sizes around their borders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 64, 65, 1024])
def test_section_sizes_and_site_counts(caller, S):
    rng = np.random.default_rng(7100 + S)
    for count in (S - 1, S, S + 1, 2 * S + 1):
        bwp = {"items_per_section": S, "reduction": 64}
        # exactly `count` sites: dense, and thinned (a site every third position, so ranks and positions part ways)
        dense = all_sites(random_records(rng, max(count, 1), 77))
        if count == 0:
            dense = no_sites(dense)
        want = host_block(dense, 1, None, bwp)
        assert want[3][1] == count and want[3][2] == -(-count // S)
        assert device_block(caller, dense, 77, 1, None, bwp) == want
        thin = all_sites(random_records(rng, 3 * count + 1, 500))
        c = thin["core"]
        c["gt"][np.arange(len(thin)) % 3 != 1] = 0
        thin["core"] = c
        want = host_block(thin, 1, None, bwp)
        assert want[3][1] == count
        assert device_block(caller, thin, 500, 1, None, bwp) == want
        if count:
            last = want[1][-1]
            assert last[2] == (count - 1) % S + 1 and len(want[0]) == 24 * len(want[1]) + 8 * count


# ---- 3. windows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("red", [1, 7, 64, 100, 1024])
def test_reductions_with_borders_on_and_inside_tiles(caller, red):
    rng = np.random.default_rng(7200 + red)
    n = 64 * 37 + 5
    for x0 in (1, 30, 1000):  # x0 = 1: start = index, so a window of 64 or 1024 begins on a tile's border; the others begin inside a tile
        recs = random_records(rng, n, x0, wide=True)
        want = host_block(recs, 2, None, {"reduction": red})
        assert device_block(caller, recs, x0, 2, None, {"reduction": red}) == want
        starts = [z[0] // red for z in want[2]]
        assert starts == sorted(set(starts)) and sum(z[2] for z in want[2]) == want[3][1] > 1000
        if red == 1:
            assert want[3][3] == want[3][1]
        if red == 64 and x0 == 1:
            assert any(z[0] % 64 == 0 for z in want[2])


def test_a_window_whose_sites_span_three_tiles_and_wide_counts(caller):
    n, x0 = 200, 1025  # starts 1024 .. 1223: one window of 1024, in four tiles
    recs = all_sites(random_records(np.random.default_rng(7300), n, x0), a=3, b=1)
    recs["counts"][64:70] = 2**32 - 1  # a = b = 2^32 - 1: m = 500
    want = host_block(recs, 0, None, {"reduction": 1024})
    assert want[2] == [(1024, 1224, 200, 500, 750, 0, 194 * 750 + 6 * 500, 194 * 750 * 750 + 6 * 500 * 500)]
    assert device_block(caller, recs, x0, 0, None, {"reduction": 1024}) == want
    # two windows, the border inside the second tile
    want = host_block(recs, 0, None, {"reduction": 1100})
    assert [z[:3] for z in want[2]] == [(1024, 1100, 76), (1100, 1224, 124)]
    assert device_block(caller, recs, x0, 0, None, {"reduction": 1100}) == want


def test_positions_up_to_the_top_of_the_range(caller):
    n = 197
    x0 = 2**32 - n  # the last position is 2^32 - 1, the last start 2^32 - 2
    rng = np.random.default_rng(7400)
    for recs in (all_sites(random_records(rng, n, x0)), random_records(rng, n, x0, wide=True)):
        for bwp in ({"items_per_section": 10, "reduction": 64}, {"items_per_section": 65535, "reduction": 2**32 - 1}, {"items_per_section": 1, "reduction": 3}):
            want = host_block(recs, 7, None, bwp)
            assert device_block(caller, recs, x0, 7, None, bwp) == want
    assert want[1][-1][1] == 2**32 - 1 or want[3][1] < n


# ---- 4. the thresholds, no site at all, the line count of the table ---------------------------------------------------------------------------
def test_thresholds_and_all_contexts(caller):
    rng = np.random.default_rng(7500)
    n, x0 = 1500, 4000
    recs = random_records(rng, n, x0)
    bwp = {"items_per_section": 100, "reduction": 50}
    plain = device_block(caller, recs, x0, 0, None, bwp)
    assert plain == host_block(recs, 0, None, bwp)
    for par in ({"min_cov": 5}, {"min_phred": 100}, {"pass_only": 1}, {"contexts": 1}, {"contexts": 1, "min_cov": 3, "min_phred": 20, "pass_only": 1}):
        got = device_block(caller, recs, x0, 0, par, bwp)
        assert got == host_block(recs, 0, par, bwp) and got != plain, par
        if par == {"contexts": 1}:
            assert got[3][1] > plain[3][1]
        elif "contexts" not in par:
            assert 0 < got[3][1] < plain[3][1]


def test_no_site_at_all(caller):
    recs = no_sites(random_records(np.random.default_rng(7600), 300, 10))
    assert device_block(caller, recs, 10) == (b"", [], [], [0] * 6) == host_block(recs, 0, None, None)
    assert device_block(caller, recs[:0], 10) == (b"", [], [], [0] * 6)  # no position either


def test_site_count_equals_the_table_s_line_count(caller):
    rng = np.random.default_rng(7700)
    n, x0 = 64 * 37 + 5, 1000
    recs = random_records(rng, n, x0, wide=True)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    d_out = torch.zeros(400 * n, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    for par in ({}, {"contexts": 1, "min_cov": 2}):
        caller.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chrW", d_out.data_ptr(), d_out.numel(), d_tot.data_ptr(), params=par)
        torch.cuda.synchronize()
        lines = int(d_tot.cpu().numpy().view(np.uint64)[1])
        got = device_block(caller, recs, x0, 0, par)
        assert got[3][1] == lines > 500 and sum(s[2] for s in got[1]) == lines == sum(z[2] for z in got[2])


# ---- 5. each room one short -------------------------------------------------------------------------------------------------------------------
def test_each_room_one_short(caller):
    rng = np.random.default_rng(7800)
    n, x0 = 700, 50
    recs = random_records(rng, n, x0, wide=True)
    bwp = {"items_per_section": 16, "reduction": 32}
    want = host_block(recs, 3, None, bwp)
    exact = (want[3][0], want[3][2], want[3][3])
    assert min(exact) > 10
    assert device_block(caller, recs, x0, 3, None, bwp, rooms=exact) == want  # exactly enough
    for k in range(3):
        rooms = tuple(v - (1 if j == k else 0) for j, v in enumerate(exact))
        got = device_block(caller, recs, x0, 3, None, bwp, rooms=rooms)  # (the guard bytes, and that the short array holds nothing, are checked inside)
        assert got[3] == want[3]  # the needs, and the sums, are reported all the same
        assert got[k] is None and [g for j, g in enumerate(got[:3]) if j != k] == [w for j, w in enumerate(want[:3]) if j != k]
    got = device_block(caller, recs, x0, 3, None, bwp, rooms=(0, 0, 0))
    assert got == (None, None, None, want[3])
    # the host form refuses the same rooms
    for k in range(3):
        with pytest.raises(B.BscError):
            bigwig.sections_recs_host(recs, 3, None, bwp, room=tuple(v - (1 if j == k else 0) for j, v in enumerate(exact)))


def test_errors_leave_the_context_usable(caller):
    L, h = caller._L, caller._h
    recs = random_records(np.random.default_rng(7900), 300, 100, wide=True)
    want = host_block(recs, 0, None, None)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    out, tot = guarded(4096), guarded(48)
    ok, bp = _lib.MethParams(), _lib.BwParams()
    A = (d_core.data_ptr(), d_aux.data_ptr(), 300)
    Z = (out.data_ptr(), 0, out.data_ptr(), 0, out.data_ptr(), 0, tot.data_ptr(), None)
    f = L.bsc_bigwig_sites_device
    assert f(h, *A, 0, 0, C.byref(ok), C.byref(bp), *Z) == -1 and b"1-based" in L.bsc_last_error()
    assert f(h, *A, 2**32 - 299, 0, C.byref(ok), C.byref(bp), *Z) == -1 and b"beyond" in L.bsc_last_error()
    assert f(h, *A, 100, 0, None, C.byref(bp), *Z) == -1 and f(h, *A, 100, 0, C.byref(ok), None, *Z) == -1
    assert f(h, *A, 100, 0, C.byref(_lib.MethParams(contexts=2)), C.byref(bp), *Z) == -1
    for bad in (_lib.BwParams(0, 1), _lib.BwParams(65536, 1), _lib.BwParams(1, 0)):
        assert f(h, *A, 100, 0, C.byref(ok), C.byref(bad), *Z) == -1 and b"items_per_section" in L.bsc_last_error()
    assert f(h, d_core.data_ptr() + 8, d_aux.data_ptr(), 299, 100, 0, C.byref(ok), C.byref(bp), *Z) == -1 and b"16-byte" in L.bsc_last_error()
    assert f(h, *A, 100, 0, C.byref(ok), C.byref(bp), out.data_ptr() + 4, 8, *Z[2:]) == -1 and b"8-byte" in L.bsc_last_error()
    assert f(h, None, d_aux.data_ptr(), 300, 100, 0, C.byref(ok), C.byref(bp), *Z) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all() and (tot.cpu().numpy() == GUARD).all()
    # a kept call with nothing kept, and with a block pending
    nb, ns, nsec, nz, ps, pz = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), C.c_void_p(1), C.c_void_p(1)
    K = (C.byref(ok), C.byref(bp), C.byref(nb), C.byref(ns), C.byref(ps), C.byref(nsec), C.byref(pz), C.byref(nz))
    assert L.bsc_block_bigwig_kept(h, 0, *K) == -1 and b"no single block" in L.bsc_last_error()
    assert (nb.value, ns.value, nsec.value, nz.value, ps.value, pz.value) == (0, 0, 0, 0, None, None)
    tpl, seq = B.synth_reads_host(88172645463325252, 9_000, 3_000, 10)
    x, y = 8_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    pinned = B.PinnedBuffer(y - x + 1, B.VCF_REC)
    caller.block_records_submit(tpl, seq, x, y, B.synth_ref_host(88172645463325252, x, y - x + 3), pinned.array)
    assert L.bsc_block_bigwig_kept(h, 0, *K) == -1 and b"no single block" in L.bsc_last_error()
    caller.block_records_fetch()
    with pytest.raises(B.BscError):
        caller.bigwig_stream_read(0, 8)  # no block's stream is there
    assert device_block(caller, recs, 100) == want


# ---- 6. the block entry -----------------------------------------------------------------------------------------------------------------------
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
    """The BAM of three contigs the methylation-table tests use: 6 000 positions at ~40x, one of 60 positions (a block shorter than a tile),
    and 30 000 positions covered thinly in several blocks."""
    d = tmp_path_factory.mktemp("bigwig_files")
    rng = np.random.default_rng(4711)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50)
            + W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


def m_of(a, b):
    return (2000 * a + (a + b)) // (2 * (a + b))


@pytest.mark.parametrize("par", [{}, {"min_cov": 12, "min_phred": 30, "pass_only": 1}])
def test_block_entry_behind_both_keep_calls(caller, small, par):
    _, bam, _, refs, reference = small
    bwp = {"items_per_section": 50, "reduction": 128}
    n_blocks, seen, cur = 0, 0, None
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            ref = block_reference(codes, int(blk.x), int(blk.y))
            if name != cur:
                cur = name
                regs = sorted([(0, len(codes))] + [(s, min(s + 100, len(codes))) for s in range(0, len(codes), 100)])
                caller.meth_regions_attach(regs)
            # without the call: the block, its table, its index entries, the regions' sums
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
            table0 = caller.block_meth_kept(name, par)
            ent0 = caller.block_csi_kept(14)[0].tobytes()
            caller.block_meth_regions_kept(par)
            acc0 = caller.meth_regions_read().copy()
            caller.meth_regions_reset()
            sites = [(p - 1, m_of(a, b)) for p, a, b in (s for s in (MR.sites_of_bcf_record(d, par) for d in RC.bcf_records(bcf0)) if s is not None)]
            py = bigwig.sections_of_sites(sites, tid, 50, 128)  # what the file itself says
            want = (py[0], len(sites), R.sum_rows(py[1]), R.sum_rows(py[2]))
            flat = lambda g: (g[0], g[1], R.sum_rows(g[2]), R.sum_rows(g[3]))
            # before anything else is read
            caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
            assert flat(caller.block_bigwig_kept(tid, par, bwp)) == want
            assert caller.block_csi_kept(14)[0].tobytes() == ent0 and caller.block_meth_kept(name, par) == table0 and kept_stream(caller, len(bcf0)) == bcf0
            caller.block_meth_regions_kept(par)
            assert (caller.meth_regions_read() == acc0).all()
            caller.meth_regions_reset()
            # after them, and twice
            bcf2, n_rec2, _ = caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
            assert caller.block_meth_kept(name, par) == table0 and caller.block_csi_kept(14)[0].tobytes() == ent0
            caller.block_meth_regions_kept(par)
            assert flat(caller.block_bigwig_kept(tid, par, bwp)) == want == flat(caller.block_bigwig_kept(tid, par, bwp))
            assert (caller.meth_regions_read() == acc0).all()
            caller.meth_regions_reset()
            assert bcf2 == bcf0 and n_rec2 == n_rec and kept_stream(caller, len(bcf0)) == bcf0 and caller.block_meth_kept(name, par) == table0
            if want[0]:
                assert caller.bigwig_stream_read(8, 16) == want[0][8:24]
            # behind the text encoder's keep call
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, reg_stop=len(codes))
            assert flat(caller.block_bigwig_kept(tid, par, bwp)) == want
            assert kept_stream(caller, len(text)) == text and n_txt == n_rec and caller.block_meth_kept(name, par) == table0
            seen += len(sites)
            n_blocks += 1
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes))
            with pytest.raises(B.BscError):
                caller.block_bigwig_kept(tid, par, bwp)
    caller.meth_regions_attach([])
    assert n_blocks > 3 and seen > (100 if par else 1000)


# ---- 7. file to file --------------------------------------------------------------------------------------------------------------------------
def run_exe(*args, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr + r.stdout
    return r


def blocks_of_table(rows, refs, cuts):
    """The (tid, [(start, m)]) blocks of a per-cytosine table's rows, cut where the reader cut its blocks: cuts = [(tid, x, y)]."""
    out = []
    for tid, x, y in cuts:
        mine = rows[(rows["chrom"] == refs[tid][0]) & (rows["start"] + 1 >= x) & (rows["start"] + 1 <= y)]
        out.append((tid, [(int(r["start"]), m_of(int(r["a"]), int(r["b"]))) for r in mine]))
    return out


def test_bam2bcf_meth_bigwig_and_pipeline(caller, small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("w" + s))
    with DeviceBamReader(caller, bam, threads=2) as rd:
        cuts = [(int(b.tid), int(b.x), int(b.y)) for b in rd.device_blocks()]
    assert len(cuts) > 3
    # the run without the switch, and with it: everything else byte-identical
    base = run_exe("--meth", p(".0.meth"), bam, fa, p(".0.bcf"), p(".0.json"), "S9").stdout
    r = run_exe("--meth", p(".1.meth"), "--meth-bigwig", p(".1.bw"), "--meth-bigwig-section", "50", "--meth-bigwig-zoom", "8", bam, fa, p(".1.bcf"),
                p(".1.json"), "S9")
    table = open(p(".1.meth"), "rb").read()
    assert table == open(p(".0.meth"), "rb").read() and open(p(".1.bcf"), "rb").read() == open(p(".0.bcf"), "rb").read()
    assert open(p(".1.json")).read() == open(p(".0.json")).read()
    rows = methbed.read_bed(p(".1.meth"))
    got = open(p(".1.bw"), "rb").read()
    assert got == R.build(refs, blocks_of_table(rows, refs, cuts), 50, 8)
    assert r.stdout == base + "%d methylation bigWig sites written\n" % len(rows)
    f = bigwig.BigWig(got)
    assert f.header["zoomLevels"] >= 2 and f.summary["basesCovered"] == len(rows) > 300
    a_rows = rows[rows["chrom"] == "chrA"]
    assert [s for s, _, _ in f.intervals("chrA")] == [int(v) for v in a_rows["start"]]
    # pipeline.run writes the same file
    s = pipeline.run(bam, reference, p(".p1.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, bigwig_path=p(".p1.bw"),
                     bigwig_section=50, bigwig_zoom=8, meth_path=p(".p1.meth"))
    assert open(p(".p1.bw"), "rb").read() == got and s["bigwig_sites"] == len(rows)
    assert open(p(".p1.bcf"), "rb").read() == open(p(".0.bcf"), "rb").read() and open(p(".p1.meth"), "rb").read() == table
    # the defaults; without --meth, compressed, indexed, as text, with --meth-merge beside it: the track is per cytosine, the rest that of the plain run
    opts = ["--format", "vcf", "-O", "b", "--index"]
    run_exe(*opts, bam, fa, p(".v0.gz"), p(".v0.json"), "S9")
    run_exe(*opts, "--meth-bigwig", p(".v1.bw"), bam, fa, p(".v1.gz"), p(".v1.json"), "S9")
    want_default = R.build(refs, blocks_of_table(rows, refs, cuts), 1024, 1024)
    assert open(p(".v1.bw"), "rb").read() == want_default
    assert open(p(".v1.gz"), "rb").read() == open(p(".v0.gz"), "rb").read() and open(p(".v1.gz.csi"), "rb").read() == open(p(".v0.gz.csi"), "rb").read()
    assert open(p(".v1.json")).read() == open(p(".v0.json")).read()
    run_exe("--meth", p(".m.meth"), "--meth-merge", "--meth-bigwig", p(".m.bw"), bam, fa, p(".m.bcf"), p(".m.json"), "S9")
    assert open(p(".m.bw"), "rb").read() == want_default
    pipeline.run(bam, reference, p(".p2.gz"), sample="S9", benchmark_mode=True, device_reader=True, text=True, bigwig_path=p(".p2.bw"))
    assert open(p(".p2.bw"), "rb").read() == want_default
    # the thresholds apply: the track of the table the same thresholds give
    th = ["--meth-min-cov", "12", "--meth-min-gq", "30", "--meth-pass", "--meth-all"]
    run_exe(*th, "--meth", p(".t.meth"), "--meth-bigwig", p(".t.bw"), bam, fa, p(".t.bcf"), p(".t.json"), "S9")
    rows_t = methbed.read_bed(p(".t.meth"))
    assert open(p(".t.bw"), "rb").read() == R.build(refs, blocks_of_table(rows_t, refs, cuts), 1024, 1024) != want_default
    # the refusals
    for extra in (["--rank", "0", "--world", "2"], ["--merge", "2"]):
        r = run_exe("--meth-bigwig", p(".no.bw"), *extra, bam, fa, p(".no.bcf"), p(".no.json"), ok=False)
        assert r.returncode == 2 and "--meth-bigwig writes a single run's track" in r.stderr
    for kw in (dict(device_reader=False), dict(shard_rank=0, shard_world=2), dict(bigwig_section=0), dict(bigwig_section=65536), dict(bigwig_zoom=0)):
        with pytest.raises(ValueError):
            pipeline.run(bam, reference, p(".no"), **dict(dict(device_reader=True, bigwig_path=p(".no.bw")), **kw))
    assert not os.path.exists(p(".no")) and not os.path.exists(p(".no.bw")) and not os.path.exists(p(".no.bcf"))
