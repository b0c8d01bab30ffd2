"""The grid-stride rounds of every kernel, at a grid of one CU (and once of three).

Every launcher in csrc/*.hip caps its grid at a multiple of the context's CU count and lets a wave (or a workgroup) stride over the rest.
On a whole device the second round of that loop starts far above the shapes a CPU reference can follow, so what runs only from round two on
— the reset of the per-wave lists, the barrier before a list is rewritten, the reuse of a workgroup's DEFLATE scratch, accumulators carried
across tiles, the `last tile` special cases — is held to a reference here: BSC_NUM_CUS (read once, by bsc_create) lowers the CU count the
grids and their workspaces follow, and every stage runs through its public entry against the reference its own test module uses, at the
smallest shape that gives three full rounds and a ragged fourth.  Each case also compares the one-CU bytes with those of a context on the
whole device: the output must not depend on the grid.  Where only the order of float additions depends on it (the two methylation
profiles of the statistics: atomic adds of doubles) the comparison is the 1e-12 of tests/test_site_stats.py, and the case says so.

Not every launcher that takes the CU count strides by it: bsc_meth_eval_kernel (a grid of one workgroup per CU over a table of fixed size) runs
in every statistics case here whenever the statistics are read, but has no rounds to count.  The device BAM reader's grids do not follow the
CU count.  The record bytes of the oracle's print thread go through the host's exp / log: on a host whose libm is not the replica's the cases
that compare them skip, with the reason the modules they borrow from give."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import bs_call_amd as B
from bs_call_amd.abi import SITE_STATS, VCF_REC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 88172645463325252
DEV = "cuda:0"

# COUPLING: what ONE round of each launcher's grid covers at ONE CU, copied by hand from the launchers (file: function — grid cap x waves
# or threads x what a wave / thread takes).  A launcher whose cap changes must be changed here too: a case would otherwise go on passing
# while no longer reaching round two (the first test pins the chain's entry of the table through the public window quantum, nothing pins
# the others).
ROUND = {
    "call": 4 * 4 * 64,          # kernels.hip bsc_dev_launch_call: num_cus * (4 waves/SIMD * 4) / (TILE / 64) = 4 workgroups of 4 wave-tiles
    "fisher": 2 * 4096 * 64,     # kernels.hip bsc_dev_launch_call: 2 workgroups per CU, a chunk of at most 4096 wave-tiles each
    "accumulate": 48 * 4 * 64,   # accumulate.hip launch_accumulate: 6 * 8 workgroups per CU x ACC_WAVES wave-tiles
    "records": 24 * 4 * 64,      # vcfcore.hip bsc_dev_launch_vcf: 3 * 8 workgroups per CU x VW wave-tiles
    "stats": 16 * 64,            # sitestats.hip bsc_dev_launch_site_stats: 1 workgroup per CU of SS_THREADS / 64 wave-tiles
    "gc": 1024,                  # sitestats.hip bsc_dev_launch_gc_cov_gtm: 1 workgroup per CU of 1024 threads, a position each
    "chain": 16 * 60,            # fused.hip bsc_dev_chain_quantum: 1 workgroup per CU x FW waves x FT records
    "packing": 32 * 4 * 64,      # compact.hip bsc_dev_launch_compact: 32 workgroups per CU x 4 wave-tiles
    "encoders": 12 * 4 * 64,     # bcfdev.hip bsc_dev_launch_bcf, vcftextdev.hip: 12 workgroups per CU x 4 wave-tiles (records or positions)
    "bcf_len_size": 2 * 256 * 64,  # bcfdev.hip bsc_dev_launch_bcf, sized from the chain's length bytes (per position, no names, short ids):
                                   # bsc_bcf_size_bytes_kernel, 2 workgroups per CU x 256 threads, a tile each
    "bcf_len_write": 16 * 4 * 64,  # ... and its write kernel: 4 * BCF_WPE_SITES = 16 workgroups per CU x 4 wave-tiles
    "fmt_g": 16 * 256,           # vcftextdev.hip bsc_dev_launch_fmt_g: 16 workgroups per CU x 256 threads, a value each
    "tables": 8 * 4 * 64,        # methdev / methregionsdev / bigwigdev / bigbeddev: 8 workgroups per CU x 4 wave-tiles
    "tables2": 8 * 4,            # ... their second stages: a wave per region / section / window
    "bgzf": 1,                   # bscall_api.c bsc_bgzf_compress: grid = CUs, a member per workgroup
    "zlib_small": 4,             # zlibdev.hip bsc_dev_zlib_grid: 4 workgroups per CU for pieces <= ZL_SMALL_PIECE, a piece each
    "zlib_large": 1,             # ... 1 for longer pieces
    "zlib_gather": 8 * 4,        # zlibdev.hip zlib_launch: 8 workgroups per CU x 4 pieces
    "csi": 8 * 256,              # csidev.hip bsc_dev_launch_csi_scan: 8 workgroups per CU x 256 threads, an interval each
    "dbsnp": 8 * 256,            # dbsnpdev.hip bsc_dbf_grid: 8 workgroups per CU x 256 threads; an item = 16 positions, or a name
    "prep": 4 * 32,              # prepdev.hip bsc_dev_launch_prep: (occupancy per CU, queried) x PREP_WAVES x 32 templates — times _prep_per_cu()
}


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


TC = _load("sg_chain", "tests/test_gpu_chain.py")
RC = _load("sg_reads_chain", "tests/test_gpu_reads_chain.py")
TR = _load("sg_records", "tests/test_gpu_records.py")
TP = _load("sg_parity", "tests/test_gpu_parity.py")
TS = _load("sg_site_stats", "tests/test_site_stats.py")
BC = _load("sg_bcf", "tests/test_gpu_bcf.py")
VT = _load("sg_vcf_text", "tests/test_gpu_vcf_text.py")
MB = _load("sg_methbed", "tests/test_gpu_methbed.py")
MC = _load("sg_methcpg", "tests/test_gpu_methcpg.py")
MR = _load("sg_methregions", "tests/test_gpu_methregions.py")
BW = _load("sg_bigwig", "tests/test_gpu_bigwig.py")
BB = _load("sg_bigbed", "tests/test_gpu_bigbed.py")
ZW = _load("sg_bigwig_z", "tests/test_gpu_bigwig_z.py")
TG = _load("sg_bgzf", "tests/test_gpu_bgzf.py")
CS = _load("sg_csi", "tests/test_gpu_csi.py")
DB = _load("sg_dbsnp", "tests/test_gpu_dbsnp_dev.py")
PR = _load("sg_prep", "tests/test_gpu_prep.py")


def _caller_under(env):
    """A context created while `env` is in the environment (bsc_create reads its switches once); the environment is put back."""
    old = {}
    for k, v in env.items():
        old[k] = os.environ.get(k)
        os.environ[k] = v
    try:
        return B.SiteCaller()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def full():
    c = B.SiteCaller()
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    c = _caller_under({"BSC_NUM_CUS": "1"})
    yield c
    c.close()


@pytest.fixture(scope="module")
def small3():
    c = _caller_under({"BSC_NUM_CUS": "3"})
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_lane():
    """one CU, and the lane-per-record packing of the chain's aux array (bsc_compact_aux_kernel)"""
    c = _caller_under({"BSC_NUM_CUS": "1", "BSC_NO_EMIT_BYTES": "1"})
    yield c
    c.close()


def _rounds(group, n, cus=1, unit=64, scale=1):
    """Asserts that n units give at least three full rounds of the group's grid and a ragged last one; returns the number of rounds.
    unit = 64: n counts positions or records walked in tiles of 64 — ragged then also means a last tile that is not full and a tile count
    that is no multiple of the round's."""
    r = ROUND[group] * cus * scale
    print("%s: %d units, a round of %d at %d CU(s): %.2f rounds" % (group, n, r, cus, n / r))
    assert n > 3 * r and (r == 1 or n % r != 0), (group, n, r)  # (a grid of one unit: the caller makes its last unit a partial one)
    if unit == 64 and r % 64 == 0:
        assert n % 64 != 0 and ((n + 63) // 64) % (r // 64) != 0, (group, n, r)
    return n / r


_MEMO = {}


def _memo(key, make):
    """A reference (or an input) is computed once and shared by the cases that need it; nobody writes to what this returns."""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _need_exact(libm_exact):
    """one policy for every case that compares record bytes with the oracle's print thread: that of the modules the references come from"""
    if not libm_exact:
        pytest.skip("host libm differs from the replica: the record bytes go through exp/log")


def _flav(oracle, libm_exact):
    return oracle.LIBM if libm_exact else oracle.BSM


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


# ---- 0. the knob took effect --------------------------------------------------------------------------------------------------------------------
def test_the_knob_took_effect(full, small, small3):
    """Without this a variable that is silently ignored would make the whole module pass while testing nothing."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ROUND["chain"] == 960
    assert small.window_quantum() == 960 and small3.window_quantum() == 3 * 960 and full.window_quantum() == 960 * cus
    for bad in ("", "0", "-1", "x", "1x", " ", str(cus + 1), "99999999999999999999"):  # anything else leaves the device's count
        c = _caller_under({"BSC_NUM_CUS": bad})
        try:
            assert c.window_quantum() == 960 * cus, bad
        finally:
            c.close()
    c = _caller_under({"BSC_NUM_CUS": str(cus)})  # the device's own count is in range
    try:
        assert c.window_quantum() == 960 * cus
    finally:
        c.close()
    assert "BSC_NUM_CUS" not in os.environ and "BSC_NO_EMIT_BYTES" not in os.environ


# ---- 1. calling kernel + Fisher pass ---------------------------------------------------------------------------------------------------------------
def _census(c, got, skip, n):
    s = c.stats()
    cov = skip == 0
    assert s["sites"] == n and s["covered"] == int(cov.sum())
    assert s["gt_hist"] == np.bincount(got["max_gt"][cov], minlength=10).tolist()
    assert s["het_calls"] == int(B.GT_HET[got["max_gt"]][cov].sum())


def test_calling_kernel(full, small, oracle, tables, libm_exact):
    n = 26_005
    _rounds("call", n)
    pile, ref = B.synth_pileup_host(SEED + 1, 4242, n, 30, 1)
    small.reset_stats()
    got, skip = small.call_sites(pile, ref)
    TP._check(oracle, tables, libm_exact, pile, ref, got, skip)
    _census(small, got, skip, n)
    fgot, fskip = full.call_sites(pile, ref)
    assert got.tobytes() == fgot.tobytes() and skip.tobytes() == fskip.tobytes()


def test_fisher_pass_with_listed_calls_in_every_chunk(full, small, oracle, tables, libm_exact):
    """A workgroup of the Fisher pass takes a second chunk only when the block has more than 2 x 4096 wave-tiles: 1.57 M positions are the
    smallest block with three rounds (the previous chunk's list and scan are then reused three times) — of the dense heterozygous pile-ups of
    tests/test_gpu_parity.py, so that every chunk lists more calls than its LDS list takes at once.  Drawing that block and calling it on the
    CPU is what this case's few seconds go to; no smaller block reaches a workgroup's second chunk."""
    n = 3 * ROUND["fisher"] + 5 * 64 + 15
    _rounds("fisher", n)
    pile, ref2, _ = TC._adversarial(np.random.default_rng(99), n)
    ref = ref2[:n].copy()
    d_cts, d_ref = _dev(pile), _dev(ref)
    outs = []
    for c in (small, full):
        d_out = torch.full((n * 200,), 0xEE, dtype=torch.uint8, device=DEV)
        d_skip = torch.empty(n, dtype=torch.uint8, device=DEV)
        c.reset_stats()
        c.call_sites_device(d_cts.data_ptr(), d_ref.data_ptr(), n, d_out.data_ptr(), d_skip.data_ptr(), 200, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((d_out.cpu().numpy().view(B.GT_METH), d_skip.cpu().numpy()))
        del d_out, d_skip
    got, skip = outs[0]
    exp, eskip = oracle.call_sites(pile, ref, tables, _flav(oracle, libm_exact), -8)
    TP._assert_exact(got, skip, exp, eskip)
    _census(small, got, skip, n)
    het = B.GT_HET[exp["max_gt"]] & (skip == 0)
    per_chunk = np.add.reduceat(het.astype(np.int64), np.arange(0, n, 4096 * 64))
    assert len(per_chunk) == 7 and per_chunk[:6].min() > 2048 and per_chunk[6] > 0  # FI_LIST = 2048: several fills of the list in every full chunk
    assert got.tobytes() == outs[1][0].tobytes() and skip.tobytes() == outs[1][1].tobytes()


# ---- 2. accumulate -----------------------------------------------------------------------------------------------------------------------------------
def test_accumulate(full, small, oracle):
    """The deep block (200x over 3 000 positions: the issue's shape) is there for the depth, not for the rounds: it is a quarter of one."""
    for cov, n_sites, x0, rounds in ((30, 37_500, 9_000, True), (200, 3_000, 777, False)):
        tpl, seq, x, y = TR._block(SEED + 200 + cov, x0, n_sites, cov)
        if rounds:
            _rounds("accumulate", y - x + 1)
        rc, exp = oracle.accumulate(tpl, seq, x, y, 20)
        got = small.accumulate(tpl, seq, x, y)
        assert rc == 0 and got.tobytes() == exp.tobytes(), cov
        assert full.accumulate(tpl, seq, x, y).tobytes() == got.tobytes(), cov


# ---- 3. unfused records and statistics -------------------------------------------------------------------------------------------------------------
def _called(oracle, tables, libm_exact):
    def make():
        n, x = 26_005, 4_000
        pile, ref = B.synth_pileup_host(SEED + 300, x, n + 2, 30, 1)
        out, skip = oracle.call_sites(pile[:n], ref[:n], tables, _flav(oracle, libm_exact), -8)
        return n, x, out, skip, ref

    return _memo("called", make)


def test_unfused_records_and_statistics(full, small, oracle, tables, libm_exact):
    """The statistics kernel is given the ORACLE's records, so that it alone is under test; integers exact.  The two methylation profiles
    are sums of doubles added atomically: their order depends on the grid, so they are held to the 1e-12 of tests/test_site_stats.py against
    the oracle and against the whole device, not to bytes."""
    _need_exact(libm_exact)
    n, x, out, skip, ref = _called(oracle, tables, libm_exact)
    _rounds("records", n)
    _rounds("stats", n)
    rng = np.random.default_rng(11)
    ref = ref.copy()
    ref[rng.integers(0, n + 2, size=n // 60)] = 0
    skip = skip.copy()
    skip[rng.integers(0, n, size=n // 25)] = 1
    db = rng.choice([0, 1, 3], size=n, p=[0.9, 0.05, 0.05]).astype(np.uint8)
    for kw in (dict(), dict(all_positions=True), dict(reg_start=x + 100, reg_stop=x + n // 2), dict(dbsnp=db)):
        st = np.zeros(1, dtype=SITE_STATS)
        exp_rec = oracle.vcf_block_stats(out, skip, ref, x, st, np.zeros(2, dtype=np.uint32), tables.lfact_store, **kw)
        got_rec = small.vcf_records(out, skip, ref, x, **kw)
        assert got_rec.tobytes() == exp_rec.tobytes(), list(kw)
        assert full.vcf_records(out, skip, ref, x, **kw).tobytes() == got_rec.tobytes(), list(kw)
        both = []
        for c in (small, full):
            c.reset_site_stats()
            c.vcf_stats(exp_rec, out, dbsnp=kw.get("dbsnp"))
            both.append(c.site_stats().copy())
        TS._compare(both[0], st[0])
        TS._compare(both[0], both[1])


def test_statistics_carry_across_a_call_that_ends_in_a_late_round(small, oracle, tables, libm_exact):
    """One block as two consecutive calls cut inside a CpG: the pending cytosine is left by the workgroup that runs the first call's last tile,
    here in its thirteenth round or later (on a whole device every tile of such a block is in the first)."""
    n, x, out, skip, ref = _called(oracle, tables, libm_exact)
    rec = oracle.vcf_block(out, skip, ref, x, all_positions=True)
    plus = (rec["emit"] == 1) & (rec["cg"] == b"C") & np.isin(rec["gt"], [1, 4, 6])
    minus = (rec["emit"] == 1) & (rec["cg"] == b"C") & np.isin(rec["gt"], [2, 7, 8])
    pairs = np.flatnonzero(plus[:-1] & minus[1:])
    cut = [int(p) + 1 for p in pairs if p > 0.7 * n and (int(p) + 1) % 64 != 0][0]
    assert cut > 12 * ROUND["stats"] and n - cut > 3 * ROUND["stats"] and cut % 64 != 0
    blocks = [(out[:cut], skip[:cut], ref[: cut + 2], x), (out[cut:], skip[cut:], ref[cut:], x + cut)]
    exp, recs = TS._oracle_stats(oracle, tables, blocks, all_positions=True)
    small.reset_site_stats()
    for (g, s, r, bx), rc in zip(blocks, recs):
        small.vcf_stats(rc, g)
    TS._compare(small.site_stats(), exp)
    small.reset_site_stats()
    small.vcf_stats(recs[0], blocks[0][0])
    small.reset_site_stats()
    small.vcf_stats(recs[1], blocks[1][0])
    second, _ = TS._oracle_stats(oracle, tables, blocks[1:], all_positions=True)
    TS._compare(small.site_stats(), second)  # a context that has not seen the first call does not know the pending cytosine


def _gc_setup(n, x0, ref2):
    """tests/test_gpu_chain.py's test_gc_by_coverage: a contig that starts 7 positions into the block and ends 150 before its end, an N in a bin"""
    from bs_call_amd.caller import gc_bins

    ref2 = ref2.copy()
    ref2[12_345] = 0
    codes = np.zeros(x0 - 1 + n - 150, dtype=np.uint8)
    codes[x0 - 1 :] = ref2[: n - 150]
    codes[x0 - 1 : x0 + 6] = 0
    start, bins = gc_bins(codes)
    assert start == x0 + 7 and 255 in bins.tolist()
    return ref2, start, bins


def _gc_census(core, depth, x0, start, bins):
    """... and its reference: every position that reached the printer counts under [total depth][G+C of its 100-base bin]"""
    exp = np.zeros((4096, 101), dtype=np.uint64)
    for i in np.nonzero(core["pos"] != 0)[0]:
        pos = x0 + int(i)
        if pos < start:
            continue
        bn = (pos - start) // 100
        if bn < len(bins) and bins[bn] <= 100:
            exp[min(int(depth[i]), 4095), bins[bn]] += 1
    return exp


def test_gc_by_coverage_unfused(full, small, oracle, tables, libm_exact):
    n, x, out, skip, ref = _called(oracle, tables, libm_exact)
    _rounds("gc", n)
    ref2, start, bins = _gc_setup(n, x, ref)
    core = oracle.vcf_block(out, skip, ref2, x)
    exp = _gc_census(core, out["counts"].sum(axis=1), x, start, bins)
    assert int(exp.sum()) > 20_000
    for c in (small, full):
        c.reset_site_stats()
        c.set_gc_bins_host(bins, start)
        try:
            c.vcf_stats(core, out)
            tab = c.gc_stats()
        finally:
            c.set_gc_bins_host(None, 0)
        assert (tab == exp).all()


# ---- 4. the fused chain and the reads chain --------------------------------------------------------------------------------------------------------
def _windows(c, n, limit):
    """the block cut into windows of c.window_size(limit): every resident wave runs the same number of tiles in each but the last"""
    w = c.window_size(limit)
    assert 3 * c.window_quantum() < w <= limit
    return [(a, min(w, n - a)) for a in range(0, n, w)]


def _chain_kws(n, x, db):
    return (dict(dbsnp=db), dict(all_positions=True), dict(reg=(x + n // 4, x + n // 2), dbsnp=db))


def _pileup_chain_case(c, full, cus, oracle, tables, libm_exact, pile, ref2, x, db, what, windowed=True):
    n = len(pile)
    for kw in _chain_kws(n, x, db):
        ecore, est, ecnt = _memo((what, n, tuple(kw)), lambda: TC._oracle_chain(oracle, tables, libm_exact, pile, ref2, x, **kw))
        cuts = [[(0, n)]] + ([_windows(c, n, 7_000 * cus)] if windowed else [])
        for wins in cuts:
            got, gst, gcnt = TC._fused(c, pile, ref2, x, wins, **kw)
            TC._same_core(got, ecore, "%s %s, %d windows at %d CUs" % (what, list(kw), len(wins), cus))
            TC._same_stats(gst, est)
            assert gcnt == ecnt
            fgot, fst, fcnt = TC._fused(full, pile, ref2, x, wins, **kw)
            assert fgot.tobytes() == got.tobytes() and fcnt == gcnt
            TC._same_stats(gst, fst)  # (the profiles: float sums in the grid's order)


def _chain_pileups(cus):
    def make():
        n = 26_005 * cus + (0 if cus == 1 else 11)
        pile, ref2 = TC._block(SEED + 400 + cus, n, 30, flags=1)
        rng = np.random.default_rng(400 + cus)
        db = np.zeros(n, dtype=np.uint8)
        idx = rng.choice(n, n // 300, replace=False)
        db[idx] = np.where(rng.random(len(idx)) < 0.1, 3, 1)
        apile, aref2, aflags = TC._adversarial(np.random.default_rng(20261004 + cus), n)
        return n, pile, ref2, db, apile, aref2, aflags

    return _memo(("chain pileups", cus), make)


@pytest.mark.parametrize("cus", [1, 3])
def test_fused_chain(full, small, small3, oracle, tables, libm_exact, cus):
    """Records, statistics and counters of the pile-up-in chain against the oracle's calc + print threads, with dbSNP flags, -A and a region,
    the block in one piece (27 rounds: every wave gets a run of 62-record tiles behind its first) and in windows of window_size()."""
    _need_exact(libm_exact)
    c = {1: small, 3: small3}[cus]
    n, pile, ref2, db, apile, aref2, aflags = _chain_pileups(cus)
    _rounds("chain", n, cus, unit=60)
    assert n % 64 != 0 and n % 60 != 0
    _pileup_chain_case(c, full, cus, oracle, tables, libm_exact, pile, ref2, 1000, db, "synthetic")
    _pileup_chain_case(c, full, cus, oracle, tables, libm_exact, apile, aref2, 777, aflags, "adversarial")


def test_fused_chain_deep_block_drains_its_lists_more_than_once(full, small, oracle, tables, libm_exact):
    """300x over 3 007 positions: CpG cytosines beyond the LDS pair table go to the pair table in HBM or to the overflow list, and the exp /
    lgamma fall-backs run — at one CU a wave meets such positions in each of its three or four tiles, not in its only one."""
    _need_exact(libm_exact)
    n = 3_007
    _rounds("chain", n, unit=60)
    pile, ref2 = TC._block(SEED + 11, n, 300)
    assert pile["counts"].sum(axis=1)[:, 4:].max() >= 64
    _pileup_chain_case(small, full, 1, oracle, tables, libm_exact, pile, ref2, 50, None, "300x", windowed=False)


def test_gc_by_coverage_fused(full, small, oracle, tables, libm_exact):
    """the chain's own form of the table (bsc_gc_cov_kernel: the window's depths, left by the chain kernel), in two windows; the census is
    of the ORACLE chain's records"""
    _need_exact(libm_exact)
    n, x0 = 26_005, 4000
    _rounds("gc", n)
    pile, ref2 = TC._block(SEED + 77, n, 30, flags=1)
    ref2, start, bins = _gc_setup(n, x0, ref2)
    d_bins = _dev(bins)
    ecore = TC._oracle_chain(oracle, tables, libm_exact, pile, ref2, x0)[0]
    exp = _gc_census(ecore, pile["counts"].reshape(n, 16).sum(axis=1), x0, start, bins)
    tabs = []
    for c in (small, full):
        c.reset_site_stats()
        c.set_gc_bins(d_bins.data_ptr(), len(bins), start)
        try:
            got, gst, _ = TC._fused_keep(c, pile, ref2, x0, [(0, 11_111), (11_111, n - 11_111)])
            tabs.append(c.gc_stats())
        finally:
            c.set_gc_bins(None, 0, 0)
        TC._same_core(got, ecore, "records behind the GC table")
        assert (tabs[-1] == exp).all() and int(exp.sum()) > 20_000


def _reads_block(cus):
    def make():
        n_sites = {1: 26_005, 3: 78_050}[cus]
        tpl, seq, x, y = RC._block(SEED + 700 + cus, 9_000, n_sites, 30)
        sz = y - x + 1
        ref2 = B.synth_ref_host(SEED + 700 + cus, x, sz + 2)
        db = np.random.default_rng(700 + cus).choice([0, 1, 3], size=sz, p=[0.9, 0.05, 0.05]).astype(np.uint8)
        return tpl, seq, x, y, sz, ref2, db

    return _memo(("reads block", cus), make)


def _reads_chain_case(c, full, oracle, tables, libm_exact, blk, kws, what):
    tpl, seq, x, y, sz, ref2, db = blk
    for kw in kws:
        ecore, eaux, est, gtm, skip = _memo((what, sz, tuple(kw)), lambda: RC._oracle_chain(oracle, tables, libm_exact, tpl, seq, x, y, ref2, **kw))
        for fused in (False, True):  # the pile-up through HBM (accumulate kernel, then the chain), and the reads-in chain kernel
            outs = []
            for cc in (c, full):
                cc.set_reads_fused(fused)
                try:
                    outs.append(RC._reads_chain(cc, tpl, seq, x, y, ref2, **kw))
                finally:
                    cc.set_reads_fused(False)
            core, aux, gst, cnt = outs[0]
            TC._same_core(core, ecore, "%s %s one_kernel=%s" % (what, list(kw), fused))
            assert aux.tobytes() == eaux.tobytes(), [f for f in RC.AUX.names if aux[f].tobytes() != eaux[f].tobytes()]
            TC._same_stats(gst, est)
            assert cnt["sites"] == sz and cnt["covered"] == int((skip == 0).sum())
            assert cnt["gt_hist"] == np.bincount(gtm["max_gt"][skip == 0], minlength=10).tolist()
            assert outs[1][0].tobytes() == core.tobytes() and outs[1][1].tobytes() == aux.tobytes() and outs[1][3] == cnt
            TC._same_stats(gst, outs[1][2])  # (the profiles: float sums in the grid's order)


@pytest.mark.parametrize("cus", [1, 3])
def test_reads_chain(full, small, small3, oracle, tables, libm_exact, cus):
    _need_exact(libm_exact)
    c = {1: small, 3: small3}[cus]
    blk = _reads_block(cus)
    tpl, seq, x, y, sz, ref2, db = blk
    _rounds("chain", sz, cus, unit=60)
    kws = (dict(), dict(all_positions=True), dict(reg=(x + sz // 4, x + sz // 2)), dict(dbsnp=db))
    _reads_chain_case(c, full, oracle, tables, libm_exact, blk, kws if cus == 1 else kws[2:], "reads")


def test_reads_chain_deep_block(full, small, oracle, tables, libm_exact):
    _need_exact(libm_exact)
    tpl, seq, x, y = RC._block(SEED + 700 + 300, 40, 3_000, 300)
    sz = y - x + 1
    _rounds("chain", sz, unit=60)
    ref2 = B.synth_ref_host(SEED + 700 + 300, x, sz + 2)
    _reads_chain_case(small, full, oracle, tables, libm_exact, (tpl, seq, x, y, sz, ref2, None), (dict(), dict(all_positions=True)), "reads 300x")


# ---- 5. packing, all four forms -----------------------------------------------------------------------------------------------------------------------
def _expected_records(oracle, tables, libm_exact, cus, **kw):
    tpl, seq, x, y, sz, ref2, db = _reads_block(cus)
    return _memo(("expected records", cus, tuple(sorted(kw))), lambda: TR._expected(oracle, tables, libm_exact, tpl, seq, x, y, ref2, **kw))


def _third_round_cap(sel, cus=1):
    """an out_cap that falls inside a tile of the packing's third round: some, not all, of that tile's records lie below it"""
    tile = (2 * ROUND["packing"] * cus) // 64 + 45  # (45: a tile of 64 records in _emit_pattern)
    below, inside = int(sel[: tile * 64].sum()), int(sel[tile * 64 : tile * 64 + 64].sum())
    assert inside >= 2
    return below + inside // 2


def _compact(c, core, second, stride, n, cap, d_dbsnp=None):
    """bsc_vcf_compact_device into a room of `cap` records with 64 guard bytes behind it -> (count, the room's bytes)"""
    d_core, d_second = _dev(core), _dev(second)
    d_db = None if d_dbsnp is None else _dev(d_dbsnp)
    d_out = torch.full((cap * 128 + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    d_cnt = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    c.vcf_compact_device(d_core.data_ptr(), d_second.data_ptr(), stride, n, d_out.data_ptr(), cap, d_cnt.data_ptr(), None if d_db is None else d_db.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[cap * 128 :] == 0xEE).all(), "the guard bytes behind the capacity were written"
    return int(d_cnt.item()), out[: cap * 128]


def _check_compact(c, full, core, second, stride, want, what, cus=1, dbsnp=None):
    n, sel = len(core), core["emit"] != 0
    exp = want.tobytes()
    cnt, out = _compact(c, core, second, stride, n, n, dbsnp)
    assert cnt == len(want) and out[: cnt * 128].tobytes() == exp, what
    assert (out[cnt * 128 :] == 0xEE).all(), what  # nothing behind the last record
    cap = _third_round_cap(sel, cus)
    cnt2, out2 = _compact(c, core, second, stride, n, cap, dbsnp)
    assert cnt2 == len(want) > cap and out2.tobytes() == exp[: cap * 128], what  # the count is the full one, the records below the cap unchanged
    fcnt, fout = _compact(full, core, second, stride, n, n, dbsnp)
    assert fcnt == cnt and fout.tobytes() == out.tobytes(), what


def _emit_pattern(n, cus=1):
    """what the generator's blocks do not give: whole tiles with no record, whole tiles with 64, and the last tile of each round with a single
    record, in lane 63"""
    emit = (np.random.default_rng(5).random(n) < 0.5).astype(np.uint8)
    tiles = (n + 63) // 64
    per_round = ROUND["packing"] * cus // 64
    for t in range(tiles):
        if t % 4 == 0:
            emit[t * 64 : t * 64 + 64] = 0
        elif t % 4 == 1:
            emit[t * 64 : t * 64 + 64] = 1
        if t % per_round == per_round - 1 and t * 64 + 63 < n:
            emit[t * 64 : t * 64 + 64] = 0
            emit[t * 64 + 63] = 1
    assert tiles > 3 * per_round
    return emit


def _aux_inputs(oracle, tables, libm_exact, cus, pattern):
    """(core, aux, the packed records) of the chain's per-position arrays, as the oracle chain forms them; pattern: the emit flags rewritten"""
    tpl, seq, x, y, sz, ref2, db = _reads_block(cus)
    ecore, eaux, _, _, _ = _memo(("reads", sz, ("all_positions",)), lambda: RC._oracle_chain(oracle, tables, libm_exact, tpl, seq, x, y, ref2, all_positions=True))
    core = ecore.copy()
    if pattern:
        core["emit"] = _emit_pattern(sz, cus)
    sel = core["emit"] != 0
    want = np.zeros(int(sel.sum()), dtype=VCF_REC)
    raw = want.view(np.uint8).reshape(-1, 128)
    raw[:, :64] = core[sel].view(np.uint8).reshape(-1, 64)
    raw[:, 64:] = eaux[sel].view(np.uint8).reshape(-1, 64)
    return core, eaux, want


@pytest.mark.parametrize("cus", [1, 3])
def test_packing_behind_the_chain(full, small, small3, oracle, tables, libm_exact, cus):
    """bsc_block_records: the chain leaves its emit bytes, bsc_tile_emit_bytes_kernel counts them and bsc_compact_aux_emit_kernel packs.  The
    host entry refuses a room that is too small (and names the count); its device half is held to the capacity rule in the cases below."""
    _need_exact(libm_exact)
    c = {1: small, 3: small3}[cus]
    tpl, seq, x, y, sz, ref2, db = _reads_block(cus)
    _rounds("packing", sz, cus)
    for kw in (dict(), dict(all_positions=True), dict(dbsnp=db)) if cus == 1 else (dict(dbsnp=db),):
        exp, gtm, skip, core = _expected_records(oracle, tables, libm_exact, cus, **kw)
        got = c.block_records(tpl, seq, x, y, ref2, **kw)
        assert len(got) == len(exp) and got.tobytes() == exp.tobytes(), list(kw)
        assert full.block_records(tpl, seq, x, y, ref2, **kw).tobytes() == got.tobytes()
        cap = _third_round_cap(core["emit"] == 1, cus)
        room = np.full(cap * 128 + 64, 0xEE, dtype=np.uint8)
        with pytest.raises(B.BscError) as e:
            c.block_records(tpl, seq, x, y, ref2, out=room[: cap * 128].view(VCF_REC), **kw)
        assert str(len(exp)) in str(e.value) and (room[cap * 128 :] == 0xEE).all()


@pytest.mark.parametrize("pattern", [False, True])
def test_packing_gt_meth_form(full, small, oracle, tables, libm_exact, pattern):
    """bsc_vcf_compact_device with stride 200 and dbSNP flags: bsc_tile_emit_kernel + bsc_compact_kernel"""
    _need_exact(libm_exact)
    tpl, seq, x, y, sz, ref2, db = _reads_block(1)
    _rounds("packing", sz)
    exp, gtm, skip, core = _expected_records(oracle, tables, libm_exact, 1, dbsnp=db)
    core = core.copy()
    if pattern:
        core["emit"] = _emit_pattern(sz) & (core["pos"] != 0)  # (a record the printer did not form cannot be written)
    sel = core["emit"] == 1
    want = np.zeros(int(sel.sum()), dtype=VCF_REC)
    want["core"], want["counts"], want["qual"] = core[sel], gtm["counts"][sel], gtm["qual"][sel]
    want["mq"], want["aq"], want["max_gt"], want["rs_found"] = gtm["mq"][sel], gtm["aq"][sel], gtm["max_gt"][sel], db[sel]
    if not pattern:
        assert want.tobytes() == exp.tobytes()
    _check_compact(small, full, core, gtm, 200, want, "gt_meth form, pattern=%s" % pattern, dbsnp=db)


@pytest.mark.parametrize("pattern", [False, True])
@pytest.mark.parametrize("form", ["emit_bytes", "lane_per_record"])
def test_packing_aux_forms(full, small, small_lane, oracle, tables, libm_exact, form, pattern):
    """bsc_vcf_compact_device with stride 0 over the chain's aux array: the counting pass leaves the emit bytes and
    bsc_compact_aux_emit_kernel packs (its list in LDS is rewritten for every tile of a wave); under BSC_NO_EMIT_BYTES the lane-per-record
    bsc_compact_aux_kernel, which no other test reaches."""
    _need_exact(libm_exact)
    c = small if form == "emit_bytes" else small_lane
    core, aux, want = _aux_inputs(oracle, tables, libm_exact, 1, pattern)
    _rounds("packing", len(core))
    _check_compact(c, full, core, aux, 0, want, "%s, pattern=%s" % (form, pattern))


def test_packing_aux_form_at_three_cus(full, small3, oracle, tables, libm_exact):
    _need_exact(libm_exact)
    core, aux, want = _aux_inputs(oracle, tables, libm_exact, 3, True)
    _rounds("packing", len(core), 3)
    _check_compact(small3, full, core, aux, 0, want, "emit bytes at 3 CUs", cus=3)


# ---- 6. BCF and VCF text ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [1, 3])
def test_bcf_over_packed_records(full, small, small3, cus):
    c = {1: small, 3: small3}[cus]
    recs, names = _memo("bcf block", lambda: BC._random_block(np.random.default_rng(20261004), 9_999, named=0.3, long_names=True))
    if cus == 3:  # the same block three times, each copy behind the one before (drawing 30 000 records one by one takes seconds)
        span = int(recs["core"]["pos"].max()) + 200
        parts = []
        for k in range(3):
            r = recs.copy()
            core = r["core"]
            core["pos"] = core["pos"] + k * span
            r["core"] = core
            parts.append(r)
        recs = np.concatenate(parts)
        nb = int(names[1][-1])
        names = (np.concatenate([names[0] + np.uint32(k * span) for k in range(3)]),
                 np.concatenate([names[1][:-1] + np.uint32(k * nb) for k in range(3)] + [np.array([3 * nb], dtype=np.uint32)]), names[2] * 3)
    n = len(recs)
    _rounds("encoders", n, cus)
    want = b"".join(BC._host_stream(recs, 5, names))
    got, total, bad = BC._device_stream(c, recs, 5, names)
    assert total == len(want) and bad == 0 and got[:total].tobytes() == want
    fgot, ftotal, fbad = BC._device_stream(full, recs, 5, names)
    assert (ftotal, fbad) == (total, bad) and fgot[:total].tobytes() == want
    if cus == 1:  # wide dictionary indices: the general emitter; and no table: no record is named
        ids = BC._lib.BcfIds(*[int(v) for v in np.random.default_rng(7).choice([5, 127, 128, 300, 32767, 32768, 1_000_000], 17)])
        want = b"".join(BC._host_stream(recs, 24, names, ids))
        got, total, bad = BC._device_stream(c, recs, 24, names, ids)
        assert total == len(want) and bad == 0 and got[:total].tobytes() == want
        want = b"".join(BC._host_stream(recs, 3, None))
        got, total, bad = BC._device_stream(c, recs, 3, None)
        assert total == len(want) and got[:total].tobytes() == want


@pytest.mark.parametrize("cus", [1, 3])
def test_vcf_text_over_packed_records(full, small, small3, cus):
    c = {1: small, 3: small3}[cus]
    n = {1: 9_999, 3: 28_001}[cus]
    _rounds("encoders", n, cus)
    rng = np.random.default_rng(9000 + n)
    recs = VT.random_records(rng, n)
    names, ids = VT.names_table(rng, recs)
    for nm, idmap in ((names, ids), (None, None)) if cus == 1 else ((names, ids),):
        want = VT.host_lines(recs, b"chr12", idmap)
        stream = b"".join(want)
        out, tot = VT.encode_packed(c, recs, b"chr12", names=nm)
        assert tot[0] == len(stream) and tot[2] == sum(1 for w in want if w) and out[: tot[0]].tobytes() == stream
        fout, ftot = VT.encode_packed(full, recs, b"chr12", names=nm)
        assert ftot == tot and fout[: tot[0]].tobytes() == stream


def _bcf_block(cus):
    """a block long enough for three rounds of the per-position BCF form's size kernel (a thread per tile)"""
    def make():
        n_sites = {1: 100_000, 3: 300_000}[cus]
        tpl, seq, x, y = RC._block(SEED + 900 + cus, 9_000, n_sites, 30)
        sz = y - x + 1
        return tpl, seq, x, y, sz, B.synth_ref_host(SEED + 900 + cus, x, sz + 2)

    return _memo(("bcf block", cus), make)


@pytest.mark.parametrize("cus", [1, 3])
def test_block_bcf_sized_from_the_chain_s_length_bytes(full, small, small3, oracle, tables, libm_exact, cus):
    """bsc_block_bcf without names and with one-byte dictionary indices: the sizes come from the chain's length bytes — bsc_bcf_size_bytes_kernel,
    a thread per tile, which carries its count of written records across its tiles — and the write kernel has a grid of its own.  Against
    the host encoder over the ORACLE chain's records (tests/test_bcf.py pins it to the Python encoder record by record), and the first 10 000
    records against the Python encoder itself (50 000 and more records in Python take seconds)."""
    import oracle_chain as OC

    _need_exact(libm_exact)
    c = {1: small, 3: small3}[cus]
    tpl, seq, x, y, sz, ref2 = _bcf_block(cus)
    _rounds("bcf_len_size", sz, cus)
    _rounds("bcf_len_write", sz, cus)
    exp, gtm, skip, core = _memo(("bcf block expected", cus), lambda: TR._expected(oracle, tables, libm_exact, tpl, seq, x, y, ref2))
    want = BC.vcf.bcf_block(exp, 3)
    sel = np.flatnonzero(core["emit"] == 1)[:10_000]
    head = OC.bcf_stream(core[sel], gtm[sel], 3)
    assert want[: len(head)] == head
    blob, n_bcf = c.block_bcf(tpl, seq, x, y, ref2, 3)
    assert n_bcf == len(exp) and blob == want
    fblob, fn = full.block_bcf(tpl, seq, x, y, ref2, 3)
    assert fn == n_bcf and fblob == blob


@pytest.mark.parametrize("cus", [1, 3])
def test_per_position_encoders_behind_the_chain(full, small, small3, oracle, tables, libm_exact, cus):
    """With dbSNP flags and names (the sizes then come from the records: bsc_bcf_size_kernel at the packed form's grid, the write kernel at the
    per-position form's): bsc_block_bcf against the host encoder over the ORACLE chain's records, and bsc_vcf_text_sites_device over the reads
    chain's arrays against the host lines of the oracle's records."""
    _need_exact(libm_exact)
    c = {1: small, 3: small3}[cus]
    tpl, seq, x, y, sz, ref2, db = _reads_block(cus)
    _rounds("encoders", sz, cus)
    _rounds("bcf_len_write", sz, cus)
    expd = _expected_records(oracle, tables, libm_exact, cus, dbsnp=db)[0]
    names, ids = VT.names_table(np.random.default_rng(6), expd, lens=(4, 9, 63, 70))
    assert ids
    want = b"".join(BC._host_stream(expd, 3, names))
    blob, n_bcf = c.block_bcf(tpl, seq, x, y, ref2, 3, names=names, dbsnp=db)
    assert n_bcf == len(expd) and blob == want
    fblob, fn = full.block_bcf(tpl, seq, x, y, ref2, 3, names=names, dbsnp=db)
    assert fn == n_bcf and fblob == blob
    wtext = b"".join(VT.host_lines(expd, b"chrS", ids))
    d_tpl, d_seq, d_ref, d_db = _dev(tpl), _dev(seq), _dev(ref2), _dev(db)
    for cc in (c, full):
        d_core = torch.zeros(sz * 64, dtype=torch.uint8, device=DEV)
        d_aux = torch.zeros(sz * 64, dtype=torch.uint8, device=DEV)
        cc.reads_chain_device(d_tpl.data_ptr(), len(tpl), d_seq.data_ptr(), seq.size, x, y, d_ref.data_ptr(), d_core.data_ptr(), d_aux.data_ptr(),
                              d_dbsnp=d_db.data_ptr())
        cap = len(wtext) + 4096
        d_out = torch.zeros(cap, dtype=torch.uint8, device=DEV)
        d_tot = torch.zeros(3, dtype=torch.int64, device=DEV)
        cc.vcf_text_sites_device(d_core.data_ptr(), d_aux.data_ptr(), sz, b"chrS", d_out.data_ptr(), cap, d_tot.data_ptr(), names=names)
        torch.cuda.synchronize()
        assert [int(v) for v in d_tot.cpu()] == [len(wtext), 0, len(expd)]
        assert d_out.cpu().numpy()[: len(wtext)].tobytes() == wtext


def test_fmt_g(full, small):
    """bsc_fmt_g_device: a thread per value; every value against the host form, a part against Python's %g"""
    rng = np.random.default_rng(7002)
    n = 3 * ROUND["fmt_g"] + 1_111
    _rounds("fmt_g", n, unit=1)
    bits = np.concatenate([(-rng.random(n // 2) * 10.0 ** rng.integers(-4, 5, n // 2)).astype(np.float32).view(np.uint32),
                           rng.integers(0, 1 << 32, n - n // 2, dtype=np.uint64).astype(np.uint32)])
    bits = bits[rng.permutation(n)]
    want = VT.host_slots(bits)
    got = VT.device_slots(small, bits)
    assert got.tobytes() == want.tobytes() and VT.device_slots(full, bits).tobytes() == want.tobytes()
    for i in range(0, n, 7):
        assert bytes(got[i][: got[i][15]]) == VT.py_g(int(bits[i])), i  # (a slot's last byte is its length)


def test_several_blocks_in_one_launch_sequence(full, small, oracle, tables, libm_exact):
    """bsc_blocks_records: the chain kernel's multi-block form (a segment table, every block its share of the waves) and the reference padding
    behind it, three blocks of 27, 5 and 3 rounds of the chain handed over together, in both forms of the reads -> records path."""
    _need_exact(libm_exact)
    tpl, seq, x, y, sz, ref2, db = _reads_block(1)
    blocks, refs, dbs, exps = [(tpl, seq, x, y)], [ref2], [db], [_expected_records(oracle, tables, libm_exact, 1, dbsnp=db)[0]]
    for k, n_sites in enumerate((5_000, 3_000)):
        t, s, bx, by = RC._block(SEED + 950 + k, blocks[-1][3] + 150, n_sites, 30)
        _rounds("chain", by - bx + 1, unit=60)
        r = B.synth_ref_host(SEED + 950 + k, bx, by - bx + 3)
        d = np.random.default_rng(950 + k).choice([0, 1, 3], size=by - bx + 1, p=[0.9, 0.05, 0.05]).astype(np.uint8)
        blocks.append((t, s, bx, by))
        refs.append(r)
        dbs.append(d)
        exps.append(TR._expected(oracle, tables, libm_exact, t, s, bx, by, r, dbsnp=d)[0])
    want = np.concatenate(exps).tobytes()
    for fused in (False, True):
        for c in (small, full):
            c.set_reads_fused(fused)
            try:
                got, per = c.blocks_records(blocks, refs, dbsnp=dbs)
            finally:
                c.set_reads_fused(False)
            assert [int(v) for v in per] == [len(e) for e in exps] and got.tobytes() == want, fused


# ---- 7. the tables over records ------------------------------------------------------------------------------------------------------------------------
N_TAB, X0_TAB = 6_300, 1000
THRESHOLDS = {"min_cov": 5, "min_phred": 20, "pass_only": 1}


def _table_records():
    return _memo("table records", lambda: MR.random_records(np.random.default_rng(7300), N_TAB, X0_TAB, wide=True))


@pytest.mark.parametrize("par", [{}, {"contexts": 1}, THRESHOLDS], ids=["CpG", "all contexts", "thresholds"])
def test_bedmethyl_and_cpg_table(full, small, par):
    _rounds("tables", N_TAB)
    recs = _table_records()
    want = MB.host_lines(recs, b"chr1", par)
    stream = b"".join(want)
    out, tot = MB.encode_packed(small, recs, b"chr1", par)
    assert tot == [len(stream)] + MB.host_sums(recs, want) and out[: tot[0]].tobytes() == stream and tot[1] > 100
    fout, ftot = MB.encode_packed(full, recs, b"chr1", par)
    assert ftot == tot and fout[: tot[0]].tobytes() == stream
    if "contexts" in par:  # (the combined-strand table is of CpGs alone)
        return
    cwant, ctot = MC.check_packed(small, recs, b"chr1", par, what="CpG table")
    assert ctot[1] > 100
    fout, ftot = MC.encode_packed(full, recs, b"chr1", par)
    assert ftot == ctot and fout[: ctot[0]].tobytes() == cwant


@pytest.mark.parametrize("par", [None, THRESHOLDS], ids=["plain", "thresholds"])
def test_regions(full, small, par):
    _rounds("tables", N_TAB)
    recs = _table_records()
    regs = sorted(MR.edge_regions(X0_TAB, N_TAB) + MR.region_sets(X0_TAB, N_TAB))
    _rounds("tables2", len(regs), unit=1)
    want = MR.host_sums(recs, regs, par)
    assert MR.device_sums(small, recs, X0_TAB, regs, par) == want and max(w[0] for w in want) > 100
    assert MR.device_sums(full, recs, X0_TAB, regs, par) == want
    small.meth_regions_reset()
    full.meth_regions_reset()


@pytest.mark.parametrize("par", [None, THRESHOLDS], ids=["plain", "thresholds"])
def test_bigwig_and_bigbed(full, small, par):
    """sections / blocks of 8 sites (3 under the thresholds) and windows of 16 bases: more than a hundred of each"""
    _rounds("tables", N_TAB)
    recs = _table_records()
    items = 3 if par else 8
    bwp = {"items_per_section": items, "reduction": 16}
    want = BW.host_block(recs, 4, par, bwp)
    _rounds("tables2", want[3][2], unit=1)
    _rounds("tables2", want[3][3], unit=1)
    assert BW.device_block(small, recs, X0_TAB, 4, par, bwp) == want
    assert BW.device_block(full, recs, X0_TAB, 4, par, bwp) == want
    bbp = {"items_per_block": items, "reduction": 16}
    bpar = dict(par or {}, contexts=1)
    want = BB.host_block(recs, 4, bpar, bbp)
    _rounds("tables2", want[3][2], unit=1)
    _rounds("tables2", want[3][3], unit=1)
    assert BB.device_block(small, recs, X0_TAB, 4, bpar, bbp) == want
    assert BB.device_block(full, recs, X0_TAB, 4, bpar, bbp) == want


# ---- 8. DEFLATE ----------------------------------------------------------------------------------------------------------------------------------------
KINDS = ["text", "zeros", "random", "abc", "skewed", "period8", "ff"]


@pytest.mark.parametrize("piece,n_pieces", [(8216, 101), (ZW.M, 4)])
def test_zlib_pieces_of_mixed_kinds(full, small, piece, n_pieces):
    """Neighbouring pieces of different kinds: a workgroup's scratch and tables go dynamic -> stored -> dynamic from one piece to its next.
    101 pieces of a section's size: 25 rounds of the small-piece grid, three of the gather's; 4 pieces and 77 bytes of the longest: five rounds
    of the large-piece grid."""
    small_kernel = piece <= 8224
    _rounds("zlib_small" if small_kernel else "zlib_large", n_pieces + (0 if small_kernel else 1), unit=1)  # (the last piece: 77 bytes)
    if small_kernel:
        _rounds("zlib_gather", n_pieces, unit=1)
    data = b"".join(ZW.source(KINDS[k % len(KINDS)], piece) for k in range(n_pieces - (1 if small_kernel else 0))) + ZW.source("text", 77)
    streams, zs, tot = ZW.zpieces(small, data, piece, 1)
    kinds = ZW.check_streams(streams, data, piece)
    assert tot == [sum(len(s) for s in streams), len(streams)] and 0 in kinds and 2 in kinds
    assert kinds[KINDS.index("random")] == 0 and kinds[KINDS.index("zeros")] == 2 and kinds[KINDS.index("random") + 1] == 2
    fstreams, _, ftot = ZW.zpieces(full, data, piece, 1)
    assert fstreams == streams and ftot == tot


@pytest.mark.parametrize("longest,n_ranges", [(8216, 101), (ZW.M, 5)])
def test_zlib_ranges_of_mixed_lengths_and_kinds(full, small, longest, n_ranges):
    """bsc_zlib_ranges_device: the same two grids over ranges of varying length (the bigBed blocks' form)"""
    small_kernel = longest <= 8224
    _rounds("zlib_small" if small_kernel else "zlib_large", n_ranges, unit=1)
    lens = [[longest, 1, 255, 4097, longest - 1, 46, 2049][k % 7] for k in range(n_ranges)]
    data = b"".join(ZW.source(KINDS[k % len(KINDS)], ln) for k, ln in enumerate(lens))
    streams, zs, tot, pieces = BB.zranges(small, data, lens, longest, 1)
    kinds = BB.check_streams(streams, pieces)
    assert tot == [sum(len(s) for s in streams), n_ranges, 0] and 0 in kinds and 2 in kinds
    fstreams, _, ftot, _ = BB.zranges(full, data, lens, longest, 1)
    assert fstreams == streams and ftot == tot


def test_bgzf_members_of_different_kinds_through_one_workgroup(full, small):
    """5 members and 123 bytes: the single workgroup compresses six members one after the other on the same scratch — dynamic, dynamic,
    stored, dynamic, dynamic, and a short last one."""
    M = TG.M
    data = ZW.source("text", M) + bytes(M) + ZW.source("random", M) + (b"abc" * M)[:M] + ZW.source("skewed", M) + ZW.source("text", 123)
    _rounds("bgzf", -(-len(data) // M), unit=1)
    assert len(data) % M == 123
    blob = TG.dev_compress(small, data)
    ms = TG.check_bgzf(blob, data)
    assert [p[0] & 7 for _, p, _, _ in ms][:4] == [5, 5, 1, 5]  # final + dynamic / stored
    assert TG.dev_compress(full, data) == blob
    assert TG.dev_compress(small, data, pieces=[1, M - 1, 2 * M + 17, 5]) == blob  # however the writes are split


# ---- 9. CSI scan and dbSNP flags / names -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bcf", "vcf"])
def test_csi_scan(full, small, fmt):
    def make():
        rng = np.random.default_rng(20261020)
        top = 3 * ROUND["csi"] * 64 + 30_000
        pos = {1, top} | set(int(v) for v in rng.integers(1, 3000, 1500)) | set(int(v) for v in rng.integers(3000, top, 1500))
        recs = CS._recs(rng, sorted(pos))
        return {"n": len(recs), "bcf": CS.vcf.bcf_block(recs, 3), "vcf": ("\n".join(CS.vcf.format_records_c(recs, "chrS")) + "\n").encode()}

    streams = _memo("csi streams", make)
    s, N = streams[fmt], streams["n"]
    sync = CS._tile_sync(s, fmt)
    _rounds("csi", len(sync) - 1, unit=1)
    for min_shift in (6, 14):
        want = CS.csi_ref.entries_of(s, fmt, min_shift, sync=sync)
        assert CS._scan(small, fmt, s, sync, min_shift) == (want, len(want), N, 0)
        assert CS._scan(full, fmt, s, sync, min_shift) == (want, len(want), N, 0)


def test_dbsnp_flags_and_names(full, small, tmp_path):
    length = 3 * ROUND["dbsnp"] * 16 + 12_000
    sites = DB.K.random_sites(length, 3, 21)
    path = DB.K.write(tmp_path / "random.idx", {"r3": sites})
    db = DB.DbSnpIndex(path)
    try:
        assert db.load_contig("r3") == len(sites)
        whole = max(s[0] for s in sites) + 200
        _rounds("dbsnp", whole // 16, unit=1)
        _rounds("dbsnp", len(sites) + 1, unit=1)
        want = db.flags(1, whole)
        assert (want == DB._oracle_flags(path, "r3", whole)).all() and int((want != 0).sum()) == len(sites)
        pos, off, by = db.names(1, whole)
        for c in (small, full):
            c.dbsnp_attach(db)
            try:
                assert c.dbsnp_count(1, whole) == (len(pos), len(by))
                for x0, n in ((1, whole), (5, whole - 9)):
                    assert DB.D.flags_device(c, x0, n).cpu().numpy().tobytes() == want[x0 - 1 : x0 - 1 + n].tobytes()
                d_pos, d_off, d_by = DB.D.names_device(c, 1, whole)
                torch.cuda.synchronize()
                assert (d_pos.cpu().numpy().view(np.uint32) == pos).all() and (d_off.cpu().numpy().view(np.uint32) == off).all()
                assert d_by.cpu().numpy().tobytes() == by
            finally:
                c.dbsnp_detach()
    finally:
        db.close()


# ---- 10. read pre-processing ----------------------------------------------------------------------------------------------------------------------------
def _prep_per_cu(c):
    """The occupancy bsc_dev_launch_prep asks the runtime for (workgroups of its copy and its profile kernel per CU; its grids are that many
    times the CU count), asked the same way.  COUPLING: the two names are the kernels' mangled symbols in libbscall_amd.so; a change of
    either kernel's parameter list changes its name, and this fails until the name is changed here (nothing stands in for the query: the
    case is to be sized from what the launcher uses)."""
    fn = c._L.hipOccupancyMaxActiveBlocksPerMultiprocessor
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_size_t]
    got = []
    for sym in ("_Z20bsc_prep_copy_kernelPK13bsc_prep_planPK13bsc_prep_descjPKhPK9bsc_mismsPKyiP12bsc_templatePhmPy",
                "_Z23bsc_prep_profile_kernelPK13bsc_prep_planPK13bsc_prep_descjPK9bsc_mismsPKyPK12bsc_templatePKhmPySE_13bsc_prep_prof"):
        try:
            handle = C.c_void_p.in_dll(c._L, sym)
        except ValueError:
            raise AssertionError("the library has no symbol %s: the kernel's parameters changed, restate its name here" % sym)
        nb = C.c_int(0)
        rc = fn(C.byref(nb), C.addressof(handle), 256, 0)
        c._L.hipGetLastError()  # (a refused query must not stay behind as the runtime's last error: the library reads that after its launches)
        assert rc == 0 and 1 <= nb.value <= 8, (sym, rc, nb.value)  # (a CU holds 2048 threads: at most 8 workgroups of 256)
        got.append(nb.value)
    print("prep: %d and %d workgroups per CU" % tuple(got))
    return max(got)


def test_read_preprocessing(full, small):
    from bs_call_amd.caller import ReadProfile, prepare_templates
    from oracle import py_prep

    T = PR.T
    per_cu = _prep_per_cu(small)
    rng = np.random.default_rng(4711)
    ok, p0 = [], 2000
    for i in range(3 * per_cu * ROUND["prep"] + 700):
        r0, m0, s0 = T._random_read(rng, 20)
        r1, m1, s1 = T._random_read(rng, 20)
        p0 += int(rng.integers(0, 6))
        kind = rng.random()
        if kind < 0.1:
            t = T.tpl((p0, 0), (s0, 0), (r0, None), (m0, ()))
        elif kind < 0.15:
            t = T.tpl((0, p0), (0, s1), (None, r1), ((), m1))
        else:
            t = T.tpl((p0, p0 + int(rng.integers(0, s0 + 40))), (s0, s1), (r0, r1), (m0, m1))
        t["orientation"] = int(rng.integers(0, 2))
        t["bs_strand"] = int(rng.integers(0, 3))
        try:  # keep the templates the reference would not abort on
            py_prep.prepare([t])
            ok.append(t)
        except py_prep.PrepError:
            pass
    _rounds("prep", len(ok), unit=1, scale=per_cu)
    kw = dict(left_trim=(2, 0), right_trim=(0, 3), min_qual=20)
    for c in (small, full):
        assert PR._both(c, ok, **kw) is not None
    raw, seq, ms = T.to_arrays(ok)
    h_tpl, h_seq, _ = prepare_templates(raw, seq, ms, **kw)
    x = max(1, int(min(p for p in h_tpl["pos"].ravel() if p)) - 2)
    y = int((h_tpl["pos"].astype(np.int64) + h_tpl["len"]).max()) + 3
    ref = rng.integers(0, 5, size=y - x + 3).astype(np.uint8)
    pf_h = ReadProfile(cap=4096)
    prepare_templates(raw, seq, ms, profile=pf_h, x=x, ref=ref, **kw)
    for c in (small, full):
        pf_d = ReadProfile(cap=4096)
        c.prepare_templates_device(raw, seq, ms, profile=pf_d, x=x, ref=ref, **kw)
        assert pf_d.used == pf_h.used and pf_d.counts[: pf_d.used].tobytes() == pf_h.counts[: pf_h.used].tobytes()
        assert not pf_d.counts[pf_d.used :].any()
    assert pf_h.used > 60 and int(pf_h.counts[1 : pf_h.used].sum()) > 1000
