"""The index of the compressed methylation tables on the device (csrc/beddev.hip over csrc/bedidx_core.h): bsc_bed_scan_device against its
host form (bsc_bed_entries_host) entry for entry and total for total, over tables the device's own encoders made (per cytosine and combined
strand: there every line covers two bases and lines straddle window borders), under every kind of interval offsets, a capacity one short,
streams damaged by hand, and a one-CU grid; the block entry bsc_block_meth_index_kept behind both _keep calls and both table calls against
the Python run rule (tests/tabix_ref.py), with everything else the block left unchanged; and file to file — bam2bcf --meth-bgzf / --meth-index
and pipeline.run(meth_index=...) against tests/tabix_ref.py's index of the same file, methbed.fetch against a linear scan."""
import ctypes as C
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import tabix_ref as R
from bs_call_amd import _lib, methbed, pipeline
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader
from bs_call_amd.caller import BED_ENTRY, bed_entries_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
GUARD = 0x7E


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


MC = _load("tbx_methcpg", "tests/test_gpu_methcpg.py")  # its record generator and its small BAM


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


@pytest.fixture(scope="module")
def one_cu():
    """A context whose launchers see one CU (BSC_NUM_CUS, read once by bsc_create): the grids are capped at 8 workgroups."""
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


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The small BAM the methylation tests generate (tests/test_gpu_methcpg.py: three contigs — 6 000 positions at ~40x, 60 positions, 30 000
    positions covered thinly in several blocks)."""
    d = tmp_path_factory.mktemp("tabix_files")
    rng = np.random.default_rng(4711)
    reference = {"chrA": rng.integers(1, 5, 6_000).astype(np.uint8), "chrT": np.array(([2, 3, 1, 4, 2, 3] * 10), dtype=np.uint8),
                 "chrG": rng.integers(1, 5, 30_000).astype(np.uint8)}
    recs = (MC.W.wgbs_records(rng, reference["chrA"], 0, 1_200, het_every=300) + MC.W.wgbs_records(rng, reference["chrT"], 1, 40, read_len=30, insert=50)
            + MC.W.wgbs_records(rng, reference["chrG"], 2, 60))
    bam, fa, refs = MC._fixture_files(d, reference, recs, "small")
    return d, bam, fa, refs, reference


def scan(c, d_table, n_bytes, sync, min_shift, cap=None):
    """bsc_bed_scan_device with guard bytes behind the entries' room: (entries as bytes-comparable array, entries there are, lines, bits)."""
    n_sync = 0 if sync is None else len(sync) - 1
    if cap is None:
        cap = (n_sync if sync is not None else 1) + n_bytes // 6 + 2
    ent = torch.full((cap * 24 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    tot = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    d_sync = None if sync is None else torch.from_numpy(np.ascontiguousarray(sync, dtype=np.uint64).view(np.int64).copy()).to("cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = c._L.bsc_bed_scan_device(c._h, C.c_void_p(d_table.data_ptr()) if n_bytes else None, n_bytes, None if d_sync is None else C.c_void_p(d_sync.data_ptr()),
                                  n_sync, min_shift, C.c_void_p(ent.data_ptr()), cap, C.c_void_p(tot.data_ptr()), st)
    assert rc == 0, c._L.bsc_last_error()
    torch.cuda.synchronize()
    t = [int(v) for v in tot.cpu().numpy().view(np.uint64)]
    assert t[3] == 77  # three totals, not four
    e = ent.cpu().numpy()
    assert (e[cap * 24 :] == GUARD).all()  # nothing behind the room given
    n = min(t[0], cap)
    assert (e[n * 24 : cap * 24] == GUARD).all()  # nothing behind the entries there are
    return e[: n * 24].view(BED_ENTRY).copy(), t[0], t[1], t[2]


def same_as_host(c, d_table, table, sync, min_shift, cap=None):
    got = scan(c, d_table, len(table), sync, min_shift, cap)
    want = bed_entries_host(table, sync, min_shift, cap_entries=cap if cap is not None else len(table) // 6 + (0 if sync is None else len(sync)) + 2)
    assert got[1:] == want[1:], (min_shift, got[1:], want[1:])
    assert got[0].tobytes() == want[0].tobytes(), min_shift
    return got


def device_table(c, rng, n, cpg, par=None, present="some", around=None):
    """A table the device's encoder makes of n dense random records (the sites form: one array position a record): (device tensor, bytes)."""
    recs = MC.random_records(rng, n, present)
    if around is not None and n:  # the positions placed around a window border: start = pos - 1
        core = recs["core"]
        core["pos"] = core["pos"].astype(np.int64) - int(core["pos"][min(n // 2, 1500)]) + around
        recs["core"] = core
    raw = recs.view(np.uint8).reshape(-1, 128)
    d_core, d_aux = MC.dev(raw[:, :64]), MC.dev(raw[:, 64:])
    cap = 400 * n + 64
    d_out = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(5, dtype=torch.int64, device="cuda")
    enc = c.meth_cpg_sites_device if cpg else c.meth_sites_device
    enc(d_core.data_ptr(), d_aux.data_ptr(), n, b"chrS", d_out.data_ptr(), cap, d_tot.data_ptr(), params=par or {})
    torch.cuda.synchronize()
    nb = int(d_tot.cpu()[0])
    assert nb <= cap
    table = d_out.cpu().numpy()[:nb].tobytes()
    return d_out, table, recs


def tile_sync(table, recs):
    """Interval offsets as the encoders leave them — a tile is 64 array positions, its interval the lines whose start lies in them —,
    computed in Python from the records' positions: empty intervals where a tile has no line."""
    pos = recs["core"]["pos"].astype(np.int64)
    lines = R.lines_of(table)
    starts = np.array([l[1] + 1 for l in lines], dtype=np.int64)  # the line's 1-based position
    offs = np.array([l[3] for l in lines] + [len(table)], dtype=np.uint64)
    edges = pos[::64]
    return [0] + [int(offs[np.searchsorted(starts, e, "left")]) for e in edges[1:]] + [len(table)]


SIZES = [63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("cpg", [False, True])
@pytest.mark.parametrize("n", SIZES + [20_003])
def test_scan_equals_the_host_form(caller, n, cpg):
    rng = np.random.default_rng(900 + n + cpg)
    big = n > 1000
    straddlers = 0
    for around in (None, 16_384 + 1):  # 1-based positions around 16 384: starts around 16 383 / 16 384
        d_t, table, recs = device_table(caller, rng, n, cpg, present="some" if big else "all", around=around)
        assert table.count(b"\n") > (n // 8)
        every = [l[3] for l in R.lines_of(table)] + [len(table)]
        tiles = tile_sync(table, recs)
        assert len(tiles) == (n + 63) // 64 + 1 and sorted(tiles) == tiles
        for ms in (4, 6, 14, 0, 31):
            a = same_as_host(caller, d_t, table, None, ms)
            b = same_as_host(caller, d_t, table, tiles, ms)
            e = same_as_host(caller, d_t, table, every, ms)
            assert a[2] == b[2] == e[2] == len(every) - 1 and a[3] == 0 and e[1] == len(every) - 1
            want = R.runs_of(table, ms)  # and the host form is the Python rule
            assert [tuple(int(v) for v in x) for x in a[0]] == want
            assert [tuple(int(v) for v in x) for x in b[0]] == R.runs_of(table, ms, sync=tiles)
            if ms in (4, 6, 14):
                straddlers += sum(1 for w in want if w[1] > w[0])
            if ms == 6 and not big:  # a capacity one short: the count still comes back, the guard stays
                got = same_as_host(caller, d_t, table, tiles, ms, cap=b[1] - 1)
                assert got[1] == b[1] and len(got[0]) == b[1] - 1 and got[0].tobytes() == b[0][:-1].tobytes()
    if cpg:
        assert straddlers >= 24 or not big  # pairs that lie in two windows: entries of their own
    else:
        assert straddlers == 0  # a cytosine's line covers one base


def test_thresholds_that_leave_whole_tiles_without_a_line(caller):
    rng = np.random.default_rng(77)
    for cpg in (False, True):
        d_t, table, recs = device_table(caller, rng, 6_000, cpg, par={"min_cov": 1 << 31, "min_phred": 20})
        tiles = tile_sync(table, recs)
        assert sum(a == b for a, b in zip(tiles, tiles[1:])) > 5 and table.count(b"\n") > 20
        for ms in (4, 14):
            got = same_as_host(caller, d_t, table, tiles, ms)
            assert got[3] == 0 and [tuple(int(v) for v in x) for x in got[0]] == R.runs_of(table, ms, sync=tiles)
    # no table at all
    empty = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert scan(caller, empty, 0, None, 14)[1:] == (0, 0, 0) and scan(caller, empty, 0, [0, 0, 0], 14)[1:] == (0, 0, 0)


def test_streams_built_by_hand_for_each_error_bit(caller):
    good = b"".join(b"c\t%d\t%d\tCG\t9\n" % (p, p + 2) for p in (10, 20, 16_383, 16_390))
    second = good.index(b"\n") + 1
    cases = [(good[:-1], None, 1), (good + b"c\t30", None, 1),  # a line that leaves its interval
             (good + b"c\t5\t7\n", None, 2),  # a start below the one before it
             (good + b"c 16400 16402\n", None, 4), (good + b"c\t16400\t16400\n", None, 4), (good + b"c\t16400\t4294967297\n", None, 4),
             (good + b"c\t00000016400\t16402\n", None, 4), (good + b"c\t16400\n", None, 4),
             (good, [0, len(good), second, len(good)], 8), (good, [0, len(good) + 1], 8),  # offsets that descend, that lie beyond the stream
             (good + b"c\t5\t7\n" + good, [0, len(good) + 6, 2 * len(good) + 6], 2)]  # the walk of THAT interval stops, the next is walked
    for data, sync, bit in cases:
        d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda")
        got = same_as_host(caller, d, data, sync, 14)
        assert got[3] & bit and (got[3] == bit or bit == 8), (data[-20:], got[3])
    assert caller._L.bsc_bed_scan_device(caller._h, None, 0, None, 0, 32, None, 0, C.c_void_p(8), None) == -1
    assert caller._L.bsc_bed_scan_device(caller._h, None, 0, None, 0, 14, None, 0, None, None) == -1


def test_grid_stride_rounds_at_one_cu(one_cu):
    """8 workgroups of 256 lanes: more than 2 048 intervals go round the grid-stride loops, here about ten times with a ragged last round."""
    rng = np.random.default_rng(31)
    for cpg in (False, True):
        d_t, table, recs = device_table(one_cu, rng, 20_003, cpg, present="all")
        every = [l[3] for l in R.lines_of(table)] + [len(table)]
        assert len(every) - 1 > 3 * 2048 and (len(every) - 1) % 2048
        for ms in (4, 14):
            got = same_as_host(one_cu, d_t, table, every, ms)
            assert got[1] == len(every) - 1 and got[3] == 0
            tiles = tile_sync(table, recs)
            same_as_host(one_cu, d_t, table, tiles, ms)
            same_as_host(one_cu, d_t, table, None, ms)


# ---- the block entry -------------------------------------------------------------------------------------------------------------------------
def merged(entries):
    """Adjacent entries with equal windows become one: what is left does not depend on where the intervals were cut."""
    out = []
    for wb, wl, n, z, u in entries:
        if out and out[-1][:2] == [wb, wl]:
            out[-1][2] += n
        else:
            out.append([wb, wl, n, z, u])
    return [tuple(e) for e in out]


def test_block_entry_behind_both_keep_calls_and_both_tables(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    p, n, r = C.c_void_p(), C.c_uint64(), C.c_uint64()
    with B.SiteCaller() as fresh:  # no table on the context
        assert L.bsc_block_meth_index_kept(fresh._h, 14, C.byref(p), C.byref(n), C.byref(r)) == -1 and b"no table" in L.bsc_last_error()
    bwp, bbp = {"items_per_section": 50, "reduction": 128}, {"items_per_block": 50, "reduction": 128}
    flat = lambda g: (g[0], g[1], g[2].tobytes(), g[3].tobytes())
    n_blocks = n_lines = n_straddle = 0
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            tid = int(blk.tid)
            name, codes = refs[tid][0], reference[refs[tid][0]]
            ref = block_reference(codes, int(blk.x), int(blk.y))
            caller.meth_regions_attach([(0, len(codes))])
            for keep_text in (False, True):
                if keep_text:
                    stream0, n_rec, _ = caller.block_vcf_rawdev(blk, ref, name, reg_stop=len(codes))
                else:
                    stream0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, tid, reg_stop=len(codes), keep=True)
                ent0 = caller.block_csi_kept(14)[0].tobytes()
                caller.block_meth_regions_kept({})
                acc0 = caller.meth_regions_read().copy()
                caller.meth_regions_reset()
                bw0, bb0 = flat(caller.block_bigwig_kept(tid, {}, bwp)), flat(caller.block_bigbed_kept(tid, {}, bbp))
                for merge in (False, True):
                    table, lines, sums = caller.block_meth_kept(name, {}, merge=merge)
                    for ms in (14, 6, 4):
                        ent, nl = caller.block_meth_index_kept(ms)
                        assert nl == lines == table.count(b"\n")
                        got = [tuple(int(v) for v in e) for e in ent]
                        assert merged(got) == R.runs_of(table, ms), (name, int(blk.x), merge, ms)
                        starts = {l[3] for l in R.lines_of(table)}
                        assert all(e[4] in starts and e[3] == 0 for e in got) and sum(e[2] for e in got) == lines
                        n_straddle += sum(1 for e in got if e[1] > e[0])
                    n_lines += lines
                    # nothing else the block left has changed
                    out = np.zeros(max(len(table), 1), np.uint8)
                    if table:
                        assert L.bsc_meth_stream_read(h, 0, len(table), out.ctypes.data) == 0
                        caller.synchronize()
                        assert out.tobytes() == table
                    assert MC.kept_stream(caller, len(stream0)) == stream0 and caller.block_csi_kept(14)[0].tobytes() == ent0
                    caller.block_meth_regions_kept({})
                    assert (caller.meth_regions_read() == acc0).all()
                    caller.meth_regions_reset()
                    assert flat(caller.block_bigwig_kept(tid, {}, bwp)) == bw0 and flat(caller.block_bigbed_kept(tid, {}, bbp)) == bb0
                    assert caller.block_meth_kept(name, {}, merge=merge) == (table, lines, sums)
                    assert L.bsc_block_meth_index_kept(h, 32, C.byref(p), C.byref(n), C.byref(r)) == -1
                    if table and merge and keep_text:  # after the table has changed hands: refused
                        d_m, n_m = C.c_void_p(), C.c_uint64()
                        assert L.bsc_meth_stream_detach(h, C.byref(d_m), C.byref(n_m)) == 0
                        assert L.bsc_block_meth_index_kept(h, 14, C.byref(p), C.byref(n), C.byref(r)) == -1 and b"detached" in L.bsc_last_error()
                        assert L.bsc_detached_free(h, d_m) == 0
            n_blocks += 1
    assert n_blocks > 3 and n_lines > 1000 and n_straddle >= 4


# ---- file to file ----------------------------------------------------------------------------------------------------------------------------
def run_exe(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


@pytest.fixture(scope="module")
def files(small):
    """The small BAM and a runner: run(stem, options, table path) -> {"main", "json", "table", and every other output there is: bytes}."""
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / s)

    def run(stem, opts, table):
        run_exe(*opts, "--meth", table, bam, fa, p(stem + ".out"), p(stem + ".json"), "S9")
        out = {"main": open(p(stem + ".out"), "rb").read(), "json": open(p(stem + ".json")).read(), "table": open(table, "rb").read()}
        for ext in (".out.csi", ".bw", ".bb", ".tsv"):
            if os.path.exists(p(stem + ext)):
                out[ext] = open(p(stem + ext), "rb").read()
        return out

    return d, bam, fa, refs, reference, run


OTHER = lambda p, s: ["--meth-bigwig", p(s + ".bw"), "--meth-bigbed", p(s + ".bb"), "--meth-window", "1000", "--meth-regions-out", p(s + ".tsv")]
CASES = {
    "bgzf-tbi": ([], ["--meth-bgzf", "--meth-index", "tbi"], "tbi"),
    "bgzf-csi": ([], ["--meth-bgzf", "--meth-index", "csi"], "csi"),
    "Ob-tbi-index": (["-O", "b", "--index"], ["--meth-index", "tbi"], "tbi"),
    "vcf-merge-csi": (["--format", "vcf", "-O", "b", "--meth-merge"], ["--meth-index", "csi"], "csi"),
    "all-others-tbi": (["--meth-all", "--meth-min-cov", "2"], ["--meth-bgzf", "--meth-index", "tbi"], "tbi"),
    "merge-Ob-bgzf-tbi": (["-O", "b", "--meth-merge"], ["--meth-bgzf", "--meth-index", "tbi"], "tbi"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bam2bcf_meth_index(files, case):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference, run = files
    p = lambda s: str(d / s)
    common, new, kind = CASES[case]
    with_others = case == "all-others-tbi"
    a, b = case + ".a", case + ".b"
    plain = run(a, common + (OTHER(p, a) if with_others else []), p(a + ".bed"))
    got = run(b, common + new + (OTHER(p, b) if with_others else []), p(b + ".bed.gz"))
    was_compressed = "-O" in common
    want_table = gzip.decompress(plain["table"]) if was_compressed else plain["table"]
    blob = got.pop("table")
    assert blob.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    table = gzip.decompress(blob)
    assert table == want_table and table.count(b"\n") > 300  # the table of the run without the switches
    if was_compressed:
        assert blob == plain["table"]  # and, where it was compressed already, the same file
    plain.pop("table")
    assert got == plain and ("main" in got and "json" in got)  # every other output byte for byte
    if with_others:
        assert {".bw", ".bb", ".tsv"} <= set(got)
    if "--index" in common:
        assert ".out.csi" in got
    # the index = the Python builder's, from the inflated table and the members
    ix_path = p(b + ".bed.gz." + kind)
    assert not os.path.exists(p(b + ".bed.gz." + ("csi" if kind == "tbi" else "tbi")))
    names, lens = [r[0] for r in refs], [r[1] for r in refs]
    raw = open(ix_path, "rb").read()
    assert gzip.decompress(raw) == R.build(kind, table, R.member_sizes(blob), names, lens, 14)
    # fetch = linear scan
    rng = np.random.default_rng(5)
    qs = [(n, 0, l) for n, l in refs] + [("chrG", 16_383, 16_384), ("chrG", 16_384, 16_385), ("chrG", 16_383, 16_385), ("chrA", 5, 5), ("nope", 0, 9)]
    for _ in range(60):
        n, l = refs[int(rng.integers(0, len(refs)))]
        s = int(rng.integers(0, l))
        qs.append((n, s, s + int(rng.choice([1, 2, 10, 300, 5000]))))
    hits = 0
    for n, s, e in qs:
        f = methbed.fetch(p(b + ".bed.gz"), n, s, e)
        assert f == R.linear(table, n, s, e), (n, s, e)
        hits += bool(f)
    assert hits > 20


@pytest.mark.parametrize("kind", ["tbi", "csi"])
def test_pipeline_meth_index(files, kind):
    d, bam, fa, refs, reference, _ = files
    out = str(d / ("pipe." + kind))
    merge = kind == "csi"
    s0 = pipeline.run(bam, reference, out + ".0", sample="S9", benchmark_mode=True, device_reader=True, meth_path=out + ".0.bed.gz", meth_merge=merge)
    s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, meth_path=out + ".bed.gz", meth_merge=merge, meth_index=kind)
    blob = open(out + ".bed.gz", "rb").read()
    assert blob == open(out + ".0.bed.gz", "rb").read() and open(out, "rb").read() == open(out + ".0", "rb").read() and s["meth_lines"] == s0["meth_lines"] > 300
    table = gzip.decompress(blob)
    got = gzip.decompress(open(out + ".bed.gz." + kind, "rb").read())
    assert got == R.build(kind, table, R.member_sizes(blob), [r[0] for r in refs], [r[1] for r in refs], 14)
    assert methbed.fetch(out + ".bed.gz", "chrG", 100, 20_000) == R.linear(table, "chrG", 100, 20_000) != []
    for bad in (dict(meth_index="tbi"), dict(meth_index="tbi", meth_path=out + ".x.bed", compressed=False), dict(meth_index="bai", meth_path=out + ".x.bed.gz")):
        with pytest.raises(ValueError):
            pipeline.run(bam, reference, out + ".x", device_reader=True, **bad)
    assert not os.path.exists(out + ".x")
