"""The per-region methylation summary on the device (csrc/methregionsdev.hip: bsc_meth_regions_tile_kernel / _region_kernel): the
accumulators against the host form (bsc_meth_regions_sum_recs, which tests/test_methregions_host.py holds to the Python rule) on dense
arrays of random record contents — every array length around a tile, every region edge in index space, every relation between regions,
with and without the chain's emit byte —, against bsc_meth_sites_device's totals, across calls, under the thresholds, the refusals, the
block entry behind both _keep calls against the Python rule over the DECODED BCF of the same block, and file to file (bam2bcf
--meth-regions / --meth-window, pipeline.run(meth_regions=...)).  Every comparison is of exact integers or bytes."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import methcpg_ref as RC
import methregions_ref as R
from bs_call_amd import _lib, methbed, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from methregions_ref import random_records, region_sets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def all_sites(recs, a=None, b=None):
    """Every record a site under the default parameters."""
    c = recs["core"]
    c["emit"], c["gt"], c["cg"] = 1, np.where(np.arange(len(recs)) % 3 == 0, 7, 4), b"C"
    recs["core"] = c
    recs["counts"] = np.maximum(recs["counts"], 1)
    if a is not None:
        recs["counts"][:, 5], recs["counts"][:, 6], recs["counts"][:, 7], recs["counts"][:, 4] = a, a, b, b
    return recs


def add(caller, recs, x0, par=None):
    """The public per-position entry over the records' two halves."""
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    caller.meth_regions_sites_device(d_core.data_ptr(), d_aux.data_ptr(), len(recs), x0, par)
    torch.cuda.synchronize()


def device_sums(caller, recs, x0, regs, par=None):
    caller.meth_regions_attach(regs)
    add(caller, recs, x0, par)
    return caller.meth_regions_read().tolist()


def host_sums(recs, regs, par=None):
    return methbed.region_summary(recs, regs, methbed.params(**(par or {}))).tolist()


def launch_with_emit(caller, recs, emit, x0, regs, par=None):
    """The launcher behind the two entries (bsc_dev_launch_meth_regions) with the chain's emit byte per position, as
    bsc_block_meth_regions_kept hands it over — the public per-position entry has no such array.  Every region is a candidate."""
    L = caller._L
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.bsc_dev_launch_meth_regions.restype = C.c_int
    L.bsc_dev_launch_meth_regions.argtypes = [vp, vp, vp, u64, u32, C.POINTER(_lib.MethParams), vp, vp, vp, C.c_size_t, vp, u32, u32, vp, C.c_int, vp]
    L.bsc_dev_scan_tmp_bytes_u64.restype = C.c_int
    L.bsc_dev_scan_tmp_bytes_u64.argtypes = [C.c_uint32, C.POINTER(C.c_size_t)]
    n = len(recs)
    n_tiles = (n + 63) // 64
    scan = C.c_size_t(0)
    assert L.bsc_dev_scan_tmp_bytes_u64(n_tiles + 1, C.byref(scan)) == 0
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux, d_emit = dev(raw[:, :64]), dev(raw[:, 64:]), dev(emit)
    d_reg = dev(np.array(regs, dtype=np.uint32))
    d_acc = torch.zeros(4 * len(regs) + 4, dtype=torch.int64, device="cuda")
    d_acc[-4:] = 77
    z = lambda k: torch.full((max(k, 16),), 0xEE, dtype=torch.uint8, device="cuda")
    d_pl, d_sc, d_tmp = z(32 * (n_tiles + 1)), z(32 * (n_tiles + 1)), z(scan.value)
    torch.cuda.synchronize()
    mp = _lib.MethParams(**(par or {}))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc = L.bsc_dev_launch_meth_regions(d_core.data_ptr(), d_aux.data_ptr(), d_emit.data_ptr(), n, x0, C.byref(mp), d_pl.data_ptr(), d_sc.data_ptr(),
                                       d_tmp.data_ptr(), scan.value, d_reg.data_ptr(), 0, len(regs), d_acc.data_ptr(), cus, None)
    assert rc == 0
    torch.cuda.synchronize()
    acc = d_acc.cpu().numpy().view(np.uint64)
    assert (acc[-4:] == 77).all()  # nothing behind the last region's accumulators
    totals = d_sc.cpu().numpy().view(np.uint64).reshape(4, n_tiles + 1)[:, -1]
    return acc[:-4].reshape(-1, 4).tolist(), [int(v) for v in totals]


# ---- 1. array lengths -------------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 63, 64, 65, 129, 64 * 37 + 5]


@pytest.mark.parametrize("n", LENGTHS)
def test_array_lengths_with_and_without_the_emit_bytes(caller, n):
    rng = np.random.default_rng(9000 + n)
    x0 = 1000
    recs = random_records(rng, n, x0, wide=True)
    regs = region_sets(x0, n)
    want = host_sums(recs, regs)
    assert device_sums(caller, recs, x0, regs) == want
    if n > 1:
        assert max(w[0] for w in want) > 0
    # the chain's byte per position: 0 takes a record away, whatever its own bytes say
    emit = rng.choice([0, 1, 1, 1, 255], n).astype(np.uint8)
    gated = recs.copy()
    c = gated["core"]
    c["emit"][emit == 0] = 0
    gated["core"] = c
    want_e = host_sums(gated, regs)
    got_e, totals = launch_with_emit(caller, recs, emit, x0, regs)
    assert got_e == want_e == R.summary(R.sites_of_rec_bytes(recs.tobytes(), None, emit), regs)
    whole = want_e[regs.index((x0 - 51, x0 - 1 + n + 50))]
    assert totals == whole  # the scans' last entries: the whole array's sums
    if n >= 64:
        assert want_e != want


# ---- 2. region edges --------------------------------------------------------------------------------------------------------------------------
def edge_regions(x0, n):
    """Regions whose index interval [i_lo, i_hi) has its edges at every place that matters: 0, 1, 63, 64, 65, the tile borders, n - 1, n;
    both in one tile, both on borders, empty, beside the array on either side, clipped at either end."""
    edges = sorted({e for e in (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, n - 1, n) if 0 <= e <= n})
    top = 2**32 - 1
    regs = [(x0 + lo - 1, x0 + hi - 1) for lo in edges for hi in edges if lo <= hi]  # start < pos <= end  <=>  i_lo <= i < i_hi
    if x0 > 30:
        regs += [(x0 - 30, x0 - 1), (x0 - 30, x0 - 2), (x0 - 30, x0), (x0 - 20, x0 + 10), (0, x0 - 1), (0, x0 + 70)]  # ending at / before it; clipped in front
    regs += [(s, min(e, top)) for s, e in ((x0 + n - 1, x0 + n + 5), (x0 + n - 2, x0 + n + 5), (x0 + n - 10, x0 + n + 20)) if s <= top]  # at / behind; clipped
    regs += [(min(x0 + n, top), min(x0 + n + 9, top)), (0, top)]
    return sorted((s, e) for s, e in regs if 0 <= s <= e <= top)


@pytest.mark.parametrize("x0", [500, 1, 2**32 - 197])
def test_region_edges_in_index_space(caller, x0):
    n = 197  # three tiles and five positions; with x0 = 2^32 - 197 the last position is 2^32 - 1
    rng = np.random.default_rng(9100 + x0 % 1000)
    regs = edge_regions(x0, n)
    assert (x0 - 1, x0 - 1) in regs and (x0 - 1, x0 + 63) in regs and (x0 + 63, x0 + 127) in regs and (x0 - 1, x0) in regs
    if x0 == 1:
        assert regs[0][0] == 0  # start = 0 with x0 = 1: the first position lies inside
    for recs in (all_sites(random_records(rng, n, x0), a=3, b=1), random_records(rng, n, x0, wide=True)):
        want = host_sums(recs, regs)
        got = device_sums(caller, recs, x0, regs)
        assert got == want
    # on all-site records a region's sites are its clipped length
    recs = all_sites(random_records(rng, n, x0), a=3, b=1)
    got = device_sums(caller, recs, x0, regs)
    for (s, e), acc in zip(regs, got):
        length = max(0, min(e, x0 + n - 1) - max(s, x0 - 1))
        assert acc == [length, 3 * length, length, 75 * length], (s, e)


# ---- 3. region relations ----------------------------------------------------------------------------------------------------------------------
def test_duplicates_nesting_overlaps_and_the_superset(caller):
    rng = np.random.default_rng(9200)
    n, x0 = 64 * 9 + 17, 10_000
    recs = random_records(rng, n, x0, wide=True)
    # one region over the whole array — and far beyond — listed first, then 300 short ones: lo = 0 for every array, wherever it lies
    short = sorted((int(s), int(s + w)) for s, w in zip(rng.integers(x0 - 40, x0 + n + 40, 300), rng.integers(0, 90, 300)))
    regs = [(0, 2_000_000)] + short + [(x0 + 5, x0 + 300)] * 3
    regs = [regs[0]] + sorted(regs[1:])
    want = host_sums(recs, regs)
    assert device_sums(caller, recs, x0, regs) == want and want[0][0] > 100
    # a second array far behind all the short ones: they are candidates of no wave's work, the whole one still adds
    recs2 = random_records(rng, 130, 1_000_000, wide=True)
    add(caller, recs2, 1_000_000)
    want2 = methbed.region_summary(recs2, regs).tolist()
    assert want2[0][0] > 20 and all(w == [0, 0, 0, 0] for w in want2[1:])
    assert caller.meth_regions_read().tolist() == [[a + b for a, b in zip(u, v)] for u, v in zip(want, want2)]
    # an array in front of every region but the first
    caller.meth_regions_reset()
    recs3 = random_records(rng, 100, 50, wide=True)
    add(caller, recs3, 50)
    assert caller.meth_regions_read().tolist() == methbed.region_summary(recs3, regs).tolist()


# ---- 4. against the per-cytosine encoder's totals ---------------------------------------------------------------------------------------------
def test_whole_array_region_and_windows_equal_the_table_s_totals(caller):
    rng = np.random.default_rng(9300)
    n, x0 = 64 * 37 + 5, 1000
    recs = random_records(rng, n, x0, wide=True)
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    d_out = torch.zeros(400 * n, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    for par in ({}, {"contexts": 1, "min_cov": 2}):
        caller.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chrW", d_out.data_ptr(), d_out.numel(), d_tot.data_ptr(), params=par)
        torch.cuda.synchronize()
        lines, sum_a, sum_b = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)[1:]]
        assert lines > 500 and sum_a > 2**32
        assert [v[:3] for v in device_sums(caller, recs, x0, [(0, x0 + n)], par)] == [[lines, sum_a, sum_b]]
        for w in (1, 7, 64, 100):
            acc = np.array(device_sums(caller, recs, x0, methbed.window_regions(x0 + n - 1, w), par), dtype=object)
            assert len(acc) == -(-(x0 + n - 1) // w) and [int(v) for v in acc.sum(axis=0)[:3]] == [lines, sum_a, sum_b], w


def test_wide_counts_do_not_wrap(caller):
    n, x0, m = 200, 77, 2**32 - 1
    recs = all_sites(random_records(np.random.default_rng(9400), n, x0), a=1, b=1)
    recs["counts"][64:70] = m  # six sites of tile 1 with every count 2^32 - 1
    regs = [(x0 + 60, x0 + 130), (x0 + 63, x0 + 69)]
    got = device_sums(caller, recs, x0, regs)
    assert got == host_sums(recs, regs)
    assert got[1] == [6, 6 * m, 6 * m, 6 * 50] and got[1][1] > 2**32 and got[0][1] == 6 * m + 64


# ---- 5. across calls --------------------------------------------------------------------------------------------------------------------------
def test_accumulation_across_calls_reset_and_a_second_attach(caller):
    rng = np.random.default_rng(9500)
    a, b = random_records(rng, 150, 300, wide=True), random_records(rng, 90, 700, wide=True)  # 300 .. 449, a gap, 700 .. 789
    regs = sorted([(250, 800), (400, 720), (449, 699), (440, 460), (690, 710), (0, 299), (789, 900)])
    caller.meth_regions_attach(regs)
    add(caller, a, 300)
    first = caller.meth_regions_read().tolist()
    assert first == host_sums(a, regs)
    add(caller, b, 700)
    both = np.concatenate([a, b])
    want = host_sums(both, regs)
    assert caller.meth_regions_read().tolist() == want and want[regs.index((449, 699))] == [0, 0, 0, 0] and want[regs.index((250, 800))][0] > first[regs.index((250, 800))][0]
    caller.meth_regions_reset()
    assert caller.meth_regions_read().tolist() == [[0, 0, 0, 0]] * len(regs)
    add(caller, b, 700)
    assert caller.meth_regions_read().tolist() == host_sums(b, regs)
    other = [(300, 350), (300, 450)]
    assert caller.meth_regions_attach(other) == 2  # replaces: other regions, their sums zero
    assert caller.meth_regions_read().tolist() == [[0, 0, 0, 0]] * 2
    add(caller, a, 300)
    assert caller.meth_regions_read().tolist() == host_sums(a, other)


# ---- 6. the thresholds ------------------------------------------------------------------------------------------------------------------------
def test_thresholds_change_the_result_as_the_rule_says(caller):
    rng = np.random.default_rng(9600)
    n, x0 = 1500, 4000
    recs = random_records(rng, n, x0)
    regs = region_sets(x0, n)
    sites = lambda par: R.summary(R.sites_of_rec_bytes(recs.tobytes(), par), regs)
    plain = device_sums(caller, recs, x0, regs)
    assert plain == sites({})
    whole = regs.index((x0 - 51, x0 - 1 + n + 50))
    for par in ({"min_cov": 5}, {"min_phred": 100}, {"pass_only": 1}, {"contexts": 1}, {"contexts": 1, "min_cov": 3, "min_phred": 20, "pass_only": 1}):
        got = device_sums(caller, recs, x0, regs, par)
        assert got == sites(par) and got != plain, par
        if par == {"contexts": 1}:
            assert got[whole][0] > plain[whole][0]
        elif "contexts" not in par:
            assert 0 < got[whole][0] < plain[whole][0]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(caller):
    L, h = caller._L, caller._h
    rng = np.random.default_rng(9700)
    recs = random_records(rng, 300, 100, wide=True)
    regs = [(90, 200), (150, 420)]
    want = host_sums(recs, regs)
    assert device_sums(caller, recs, 100, regs) == want

    def still_right():
        caller.meth_regions_reset()
        add(caller, recs, 100)
        assert caller.meth_regions_read().tolist() == want

    for bad, word in (([(150, 420), (90, 200)], b"sort"), ([(90, 200), (90, 100)], b"sort"), ([(90, 200), (300, 250)], b"start 300 > end 250")):
        r = np.array(bad, dtype=np.uint32)
        assert L.bsc_meth_regions_attach(h, r.ctypes.data, len(r)) == -1 and word in L.bsc_last_error()
        still_right()  # the previous attachment stays
    assert L.bsc_meth_regions_attach(h, np.zeros(2, np.uint32).ctypes.data, (1 << 27) + 1) == -1 and b"2^27" in L.bsc_last_error()
    still_right()
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    ok = _lib.MethParams()
    A = (d_core.data_ptr(), d_aux.data_ptr(), 300)
    assert L.bsc_meth_regions_sites_device(h, *A, 0, C.byref(ok), None) == -1 and b"1-based" in L.bsc_last_error()
    assert L.bsc_meth_regions_sites_device(h, *A, 2**32 - 299, C.byref(ok), None) == -1 and b"beyond" in L.bsc_last_error()
    assert L.bsc_meth_regions_sites_device(h, *A, 100, None, None) == -1
    assert L.bsc_meth_regions_sites_device(h, *A, 100, C.byref(_lib.MethParams(contexts=2)), None) == -1
    assert L.bsc_meth_regions_sites_device(h, d_core.data_ptr() + 8, d_aux.data_ptr(), 299, 100, C.byref(ok), None) == -1 and b"aligned" in L.bsc_last_error()
    assert L.bsc_meth_regions_sites_device(h, None, d_aux.data_ptr(), 300, 100, C.byref(ok), None) == -1
    acc = np.zeros((3, 4), np.uint64)
    assert L.bsc_meth_regions_read(h, acc.ctypes.data, 3) == -1 and b"2 regions are attached" in L.bsc_last_error()
    still_right()
    # a kept call with nothing kept, and with a block pending
    ns, sums = C.c_uint64(7), (C.c_uint64 * 3)(7, 7, 7)
    assert L.bsc_block_meth_regions_kept(h, C.byref(ok), C.byref(ns), sums) == -1 and b"no single block" in L.bsc_last_error()
    assert ns.value == 0 and list(sums) == [0, 0, 0]
    tpl, seq = B.synth_reads_host(88172645463325252, 9_000, 3_000, 10)
    x, y = 8_998, int((tpl["pos"] + tpl["len"]).max()) - 1
    out = B.PinnedBuffer(y - x + 1, B.VCF_REC)
    caller.block_records_submit(tpl, seq, x, y, B.synth_ref_host(88172645463325252, x, y - x + 3), out.array)
    assert L.bsc_block_meth_regions_kept(h, C.byref(ok), None, None) == -1 and b"no single block" in L.bsc_last_error()
    caller.block_records_fetch()
    still_right()
    # nothing attached: the device call and the kept call are refused, reading gives nothing
    assert caller.meth_regions_attach([]) == 0
    assert L.bsc_meth_regions_sites_device(h, *A, 100, C.byref(ok), None) == -1 and b"no regions are attached" in L.bsc_last_error()
    assert caller.meth_regions_read().shape == (0, 4)
    caller.meth_regions_reset()
    assert device_sums(caller, recs, 100, regs) == want


# ---- 8. the block entry -----------------------------------------------------------------------------------------------------------------------
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
    d = tmp_path_factory.mktemp("methregions_files")
    rng = np.random.default_rng(4711)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50)
            + W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = _fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def contig_regions(length, rng):
    """Windows of 100, three nested regions, a whole-contig one listed first, staggered overlaps, an empty one: sorted."""
    regs = [(0, length)] + [(s, min(s + 100, length)) for s in range(0, length, 100)]
    regs += [(length // 4, 3 * length // 4), (length // 3, length // 2), (length // 3, length // 2), (length // 2, length // 2)]
    regs += [(int(s), min(int(s) + 250, length)) for s in rng.integers(0, length, 20)]
    return sorted(regs)


def kept_stream(caller, n):
    out = np.zeros(max(n, 1), np.uint8)
    assert caller._L.bsc_bcf_stream_read(caller._h, 0, n, out.ctypes.data) == 0
    caller.synchronize()
    return out[:n].tobytes()


@pytest.mark.parametrize("par", [{}, {"min_cov": 12, "min_phred": 30, "pass_only": 1}])
def test_block_entry_behind_both_keep_calls(caller, small, par):
    _, bam, _, refs, reference = small
    rng = np.random.default_rng(9800)
    n_blocks, cur, regs, want, seen = 0, None, None, None, 0
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
            ref = block_reference(codes, int(blk.x), int(blk.y))
            if name != cur:  # the contig change: its regions attached, their sums zero
                cur, regs = name, contig_regions(len(codes), rng)
                caller.meth_regions_attach(regs)
                want = [[0, 0, 0, 0] for _ in regs]
            # not at all: the block, its table and its index entries without a regions call
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
            table0 = caller.block_meth_kept(name, par)
            ent0 = caller.block_csi_kept(14)[0].tobytes()
            sites = [s for s in (R.sites_of_bcf_record(d, par) for d in RC.bcf_records(bcf0)) if s is not None]  # what the file itself says
            block_sums = (len(sites), sum(s[1] for s in sites), sum(s[2] for s in sites))
            # before the table and the stream are read
            caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
            assert caller.block_meth_regions_kept(par) == block_sums
            assert caller.block_meth_kept(name, par) == table0 and kept_stream(caller, len(bcf0)) == bcf0
            want = R.summary(sites, regs, want)
            assert caller.meth_regions_read().tolist() == want, (name, int(blk.x))
            # after them
            bcf2, n_rec2, _ = caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
            assert caller.block_meth_kept(name, par) == table0 and caller.block_csi_kept(14)[0].tobytes() == ent0
            assert caller.block_meth_regions_kept(par) == block_sums
            assert bcf2 == bcf0 and n_rec2 == n_rec and kept_stream(caller, len(bcf0)) == bcf0 and caller.block_meth_kept(name, par) == table0
            want = R.summary(sites, regs, want)
            # behind the text encoder's keep call
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, reg_stop=len(codes))
            assert caller.block_meth_regions_kept(par) == block_sums
            assert kept_stream(caller, len(text)) == text and n_txt == n_rec and caller.block_meth_kept(name, par) == table0
            want = R.summary(sites, regs, want)
            assert caller.meth_regions_read().tolist() == want, (name, int(blk.x))
            seen += len(sites)
            n_blocks += 1
            # refused behind a call that kept nothing; the sums stay
            caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes))
            with pytest.raises(B.BscError):
                caller.block_meth_regions_kept(par)
            assert caller.meth_regions_read().tolist() == want
    caller.meth_regions_attach([])
    assert n_blocks > 3 and seen > (100 if par else 1000)


# ---- 9. file to file --------------------------------------------------------------------------------------------------------------------------
def run_exe(*args, ok=True):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr + r.stdout
    return r


def expected_summary(bed_rows, refs, region_sets_by_contig):
    out = []
    for name, _ in refs:  # the BAM header's order
        if name not in region_sets_by_contig:
            continue
        regs, names = region_sets_by_contig[name]
        rows = bed_rows[bed_rows["chrom"] == name]
        out.append(methbed.format_regions(name, regs, names, methbed.region_summary(rows, regs)))
    return b"".join(out)


def test_bam2bcf_meth_regions_and_pipeline(small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("r" + s))
    rng = np.random.default_rng(9900)
    lines = ["# regions of the small fixture", "track name=regions"]
    for name, length in (("chrG", 30_000), ("chrZ", 500), ("chrA", 6_000), ("chrT", 60)):  # not in the header's order; chrZ is not in the header
        for k, (s, e) in enumerate(contig_regions(length, rng)[::-1]):  # unsorted
            lines.append("%s\t%d\t%d" % (name, s, e) + ("\t%s_%d\t0\t+" % (name, k) if k % 3 else ""))
    bed_text = ("\n".join(lines) + "\n").encode()
    open(p(".bed"), "wb").write(bed_text)
    sets = methbed.parse_regions(bed_text)
    n_z = len(sets.pop("chrZ")[0])
    # the run without the switch, and with it: everything else byte-identical
    base = run_exe("--meth", p(".0.meth"), bam, fa, p(".0.bcf"), p(".0.json"), "S9").stdout
    r = run_exe("--meth", p(".1.meth"), "--meth-regions", p(".bed"), "--meth-regions-out", p(".1.tsv"), bam, fa, p(".1.bcf"), p(".1.json"), "S9")
    table = open(p(".1.meth"), "rb").read()
    assert table == open(p(".0.meth"), "rb").read() and open(p(".1.bcf"), "rb").read() == open(p(".0.bcf"), "rb").read()
    assert open(p(".1.json")).read() == open(p(".0.json")).read()
    rows = methbed.read_bed(p(".1.meth"))
    want = expected_summary(rows, refs, sets)
    got = open(p(".1.tsv"), "rb").read()
    assert got == want and got.count(b"\n") == sum(len(v[0]) for v in sets.values())
    assert r.stdout == base + "%d methylation region lines written\n" % got.count(b"\n")
    assert ("%d regions on 1 contigs the BAM header does not name were skipped" % n_z) in r.stderr
    whole = [ln.split(b"\t") for ln in got.split(b"\n") if ln.startswith(b"chrA\t0\t6000\t")]
    a_rows = rows[rows["chrom"] == "chrA"]
    assert len(whole) == 1 and [int(v) for v in whole[0][4:8]] == [len(a_rows), int((a_rows["a"] + a_rows["b"]).sum()), int(a_rows["a"].sum()), int(a_rows["b"].sum())]
    assert len(a_rows) > 300
    # without --meth, compressed, indexed, as text: the summary is the same, the main file and its index are those of the plain run
    opts = ["--format", "vcf", "-O", "b", "--index"]
    run_exe(*opts, bam, fa, p(".v0.gz"), p(".v0.json"), "S9")
    run_exe(*opts, "--meth-regions-out", p(".v1.tsv"), "--meth-regions", p(".bed"), bam, fa, p(".v1.gz"), p(".v1.json"), "S9")
    assert open(p(".v1.tsv"), "rb").read() == want
    assert open(p(".v1.gz"), "rb").read() == open(p(".v0.gz"), "rb").read() and open(p(".v1.gz.csi"), "rb").read() == open(p(".v0.gz.csi"), "rb").read()
    assert open(p(".v1.json")).read() == open(p(".v0.json")).read()
    # the thresholds apply: the summary of the table the same thresholds give
    th = ["--meth-min-cov", "12", "--meth-min-gq", "30", "--meth-pass"]
    run_exe(*th, "--meth", p(".t.meth"), "--meth-regions", p(".bed"), "--meth-regions-out", p(".t.tsv"), bam, fa, p(".t.bcf"), p(".t.json"), "S9")
    got_t = open(p(".t.tsv"), "rb").read()
    assert got_t == expected_summary(methbed.read_bed(p(".t.meth")), refs, sets) and got_t != want
    # --meth-window: the lines partition each contig, their sums are the table's
    run_exe("--meth-window", "1000", "--meth-regions-out", p(".w.tsv"), bam, fa, p(".w.bcf"), p(".w.json"), "S9")
    win = [ln.split(b"\t") for ln in open(p(".w.tsv"), "rb").read().split(b"\n") if ln]
    assert open(p(".w.bcf"), "rb").read() == open(p(".0.bcf"), "rb").read()
    for name, length in refs:
        mine = [f for f in win if f[0] == name.encode()]
        assert [(int(f[1]), int(f[2])) for f in mine] == [(s, min(s + 1000, length)) for s in range(0, length, 1000)] and all(f[3] == b"." for f in mine)
        c_rows = rows[rows["chrom"] == name]
        assert [sum(int(f[k]) for f in mine) for k in (4, 6, 7)] == [len(c_rows), int(c_rows["a"].sum()), int(c_rows["b"].sum())]
    assert b"".join(b"\t".join(f) + b"\n" for f in win) == expected_summary(rows, refs, {n: (methbed.window_regions(l, 1000), None) for n, l in refs})
    # a malformed BED file: the line's number, and no run
    open(p(".bad.bed"), "wb").write(b"chrA\t1\t2\nchrA\t5\t4\n")
    r = run_exe("--meth-regions", p(".bad.bed"), "--meth-regions-out", p(".bad.tsv"), bam, fa, p(".bad.bcf"), p(".bad.json"), ok=False)
    assert "line 2" in r.stderr and not os.path.exists(p(".bad.bcf"))
    r = run_exe("--meth-regions", p(".bed"), bam, fa, p(".bad.bcf"), p(".bad.json"), ok=False)
    assert r.returncode == 2 and "--meth-regions-out" in r.stderr
    # pipeline.run: a path, a list, windows
    s = pipeline.run(bam, reference, p(".p1.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, meth_regions=p(".bed"),
                     meth_regions_path=p(".p1.tsv"), meth_path=p(".p1.meth"))
    assert open(p(".p1.tsv"), "rb").read() == want and s["meth_region_lines"] == want.count(b"\n")
    assert open(p(".p1.bcf"), "rb").read() == open(p(".0.bcf"), "rb").read() and open(p(".p1.meth"), "rb").read() == table
    as_list = [(n, int(r_["start"]), int(r_["end"]), nm) for n, (regs, names) in sets.items() for r_, nm in zip(regs, names)][::-1]
    s = pipeline.run(bam, reference, p(".p2.gz"), sample="S9", benchmark_mode=True, device_reader=True, text=True, meth_regions=as_list, meth_regions_path=p(".p2.tsv"))
    assert open(p(".p2.tsv"), "rb").read().count(b"\n") == want.count(b"\n") == s["meth_region_lines"]
    assert sorted(open(p(".p2.tsv"), "rb").read().split(b"\n")) == sorted(want.split(b"\n"))  # (equal regions in the list's order, not the file's)
    pipeline.run(bam, reference, p(".p3.bcf"), sample="S9", benchmark_mode=True, device_reader=True, compressed=False, meth_window=1000, meth_regions_path=p(".p3.tsv"))
    assert open(p(".p3.tsv"), "rb").read() == open(p(".w.tsv"), "rb").read()
    for kw in (dict(meth_regions=p(".bed")), dict(meth_regions_path=p(".no.tsv")), dict(meth_regions=p(".bed"), meth_window=10, meth_regions_path=p(".no.tsv")),
               dict(meth_window=0, meth_regions_path=p(".no.tsv")), dict(meth_window=10, meth_regions_path=p(".no.tsv"), device_reader=False)):
        with pytest.raises(ValueError):
            pipeline.run(bam, reference, p(".no"), **dict(dict(device_reader=True), **kw))
    assert not os.path.exists(p(".no")) and not os.path.exists(p(".no.tsv"))
