"""The combined-strand CpG table on the device (csrc/methdev.hip: bsc_meth_cpg_size_kernel / _write_kernel): the encoder against the host
form (bsc_meth_cpg_format_recs) byte for byte and total for total — both input forms, the neighbour across every tile border and at both
ends of the array, the count on the device, the emit-byte gate, every phase of a tile's span, the parts path, capacity —, the block entry
behind both _keep calls against the Python rule (tests/methcpg_ref.py) over the DECODED BCF of the same block and against the
per-cytosine table's sums, and file to file (bam2bcf --meth --meth-merge, pipeline.run(meth_merge=True))."""
import ctypes as C
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import methcpg_ref as R
from bs_call_amd import _lib, methbed, pipeline, vcf
from bs_call_amd.abi import VCF_REC
from bs_call_amd.bam import block_reference
from bs_call_amd.bamdev import DeviceBamReader

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
spec = importlib.util.spec_from_file_location("make_bam", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(spec)
spec.loader.exec_module(W)
PAD = 0xEE


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def host_table(recs, contig, par, n=None):
    recs = recs if n is None else recs[:n]
    return methbed.format_cpg_recs(recs, contig, _lib.MethParams(**par), totals=True)


def half(recs, i, strand, pos=None, a=None, b=None):
    """Record i becomes a half of that strand that no threshold of these tests gates."""
    c = recs["core"]
    c["emit"][i], c["gt"][i], c["cg"][i], c["flt"][i], c["phred"][i] = 1, 4 if strand == "+" else 7, b"C", 0, 200
    if pos is not None:
        c["pos"][i] = pos
    recs["core"] = c
    cnt = recs["counts"]
    cnt[i] = np.maximum(cnt[i], 1)
    if a is not None:
        cnt[i, 6 if strand == "-" else 5], cnt[i, 4 if strand == "-" else 7] = a, b
    recs["counts"] = cnt


def random_records(rng, n, present="some"):
    """Random bytes in every field, at positions that run consecutively and then jump; emit, gt, cg and the counts then drawn so that
    records are halves and neighbours pair.  present: "some" (most of them, with stretches of none longer than a tile), "none", "all"
    (every record a half: plus and minus in random order)."""
    raw = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    recs = raw.view(VCF_REC).reshape(-1)
    if not n:
        return recs
    core = recs["core"]
    core["pos"] = 1 + np.cumsum(np.where(rng.random(n) < 0.85, 1, rng.choice([2, 3, 70], n)))
    core["emit"] = rng.choice([0, 1, 1, 1, 1, 1, 255], n)
    core["gt"] = rng.choice([4, 7, 4, 7, 4, 7, 0, 5], n)
    core["flt"] = rng.choice([0, 0, 0, 1, 8, 128, 143], n)
    core["phred"] = rng.choice([0, 19, 20, 99, 100, 255], n)
    core["cg"] = rng.choice(list(b"CCCCCCHN"), n).astype(np.uint8).view("S1")
    scale = rng.choice([0, 1, 3, 30, 1000, 70000, 2**32 - 1], (n, 8))
    recs["counts"] = (rng.random((n, 8)) * (scale + 1)).astype(np.uint64).clip(0, 2**32 - 1).astype(np.uint32)
    if present == "none":
        core["emit"] = 0
    elif present == "all":
        core["emit"], core["gt"], core["cg"] = 1, rng.choice([4, 7], n), b"C"
        recs["counts"] = np.maximum(recs["counts"], 1)
    else:
        for s in range(100, n - 200, 1500):
            core["emit"][s : s + 150] = 0
    recs["core"] = core
    return recs


def encode_packed(caller, recs, contig, par, cap=None, n=None):
    d_recs = dev(recs) if len(recs) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_n = torch.tensor([len(recs) if n is None else n], dtype=torch.int64, device="cuda")
    cap = max(16, 400 * len(recs)) if cap is None else cap
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_tot = torch.full((6,), 77, dtype=torch.int64, device="cuda")
    caller.meth_cpg_block_device(d_recs.data_ptr(), d_n.data_ptr(), len(recs), contig, d_out.data_ptr(), cap, d_tot.data_ptr(), params=par)
    torch.cuda.synchronize()
    tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
    assert tot[5] == 77  # five totals, not six
    tot = tot[:5]
    out = d_out.cpu().numpy()
    assert (out[cap:] == PAD).all()  # nothing behind the room given
    if tot[0] <= cap:
        assert (out[tot[0] : tot[0] + 16] == PAD).all() and (out[tot[0] : cap] == PAD).all()  # nothing behind the stream's end
    return out[:cap], tot


def check_packed(caller, recs, contig, par, n=None, what=""):
    want, wtot = host_table(recs, contig, par, n)
    out, tot = encode_packed(caller, recs, contig, par, n=n)
    assert tot == wtot, (what, tot, wtot)
    assert out[: tot[0]].tobytes() == want, what
    return want, tot


# ---- 1. the packed form against the host form ------------------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, 128, 129, 4096 + 17]


@pytest.mark.parametrize("n", SIZES)
def test_packed_records_equal_the_host_table(caller, n):
    rng = np.random.default_rng(7000 + n)
    contig = [b"c", b"chr1", b"chrUn_KI270742v1"][n % 3]
    for present in ("some", "none", "all") if n else ("some",):
        recs = random_records(rng, n, present)
        want, tot = check_packed(caller, recs, contig, {}, what=present)
        if present == "none":
            assert tot == [0, 0, 0, 0, 0]
        if present == "all":
            assert tot[1] + tot[4] == n  # every record is a half, of a line of its own or of a pair's
    if n == 4096 + 17:  # the thresholds, on the device as on the host: min_cov on the sum
        recs = random_records(rng, n, "some")
        plain = host_table(recs, contig, {})[1]
        for par in ({"min_cov": 5}, {"min_phred": 100}, {"pass_only": 1}, {"min_cov": 5, "min_phred": 100, "pass_only": 1}):
            _, tot = check_packed(caller, recs, contig, par, what=par)
            assert 0 < tot[1] < plain[1] and 0 < tot[4], (par, tot)


@pytest.mark.parametrize("n", [2, 64, 65, 128, 129, 4096 + 17])
def test_the_neighbour_across_tile_borders_and_at_both_ends(caller, n):
    rng = np.random.default_rng(7100 + n)
    borders = [i for i in range(63, n - 1, 64)]
    # a pair across every tile border: plus at lane 63, minus at lane 0
    recs = random_records(rng, n, "some")
    for i in borders:
        half(recs, i, "+", a=3, b=1)
        half(recs, i + 1, "-", pos=int(recs["core"]["pos"][i]) + 1, a=2, b=4)
        if i + 2 < n and recs["core"]["pos"][i + 2] <= recs["core"]["pos"][i + 1]:
            recs["core"]["emit"][i + 2] = 0
    want, tot = check_packed(caller, recs, b"chrB", {}, what="border pairs")
    for i in borders:
        assert (b"chrB\t%d\t%d\tCG\t10\t.\t" % (recs["core"]["pos"][i] - 1, recs["core"]["pos"][i] + 1)) in want
    assert tot[4] >= len(borders)
    # ... and the same pairs alone, nothing else in their tiles: the minus half's tile has no bytes and no wave
    alone = recs.copy()
    keep = np.zeros(n, bool)
    keep[borders] = True
    keep[[i + 1 for i in borders]] = True
    alone["core"]["emit"][~keep] = 0
    _, tot = check_packed(caller, alone, b"chrB", {}, what="border pairs alone")
    assert tot[1] == tot[4] == len(borders)
    # a minus half at lane 0 whose predecessor is no half (even borders), or a plus half one position too far (odd borders)
    recs = random_records(rng, n, "some")
    for k, i in enumerate(borders):
        half(recs, i + 1, "-", a=2, b=4)
        if k % 2:
            half(recs, i, "+", pos=int(recs["core"]["pos"][i + 1]) - 2, a=3, b=1)
        else:
            recs["core"]["gt"][i] = 5
    want, _ = check_packed(caller, recs, b"chrB", {}, what="lane 0 singles")
    for i in borders:
        assert (b"chrB\t%d\t%d\tCG\t6\t-\t" % (recs["core"]["pos"][i + 1] - 2, recs["core"]["pos"][i + 1])) in want
    # a plus half as the very last record, a minus half as the very first
    recs = random_records(rng, n, "all")
    half(recs, n - 1, "+", a=3, b=1)
    half(recs, 0, "-", a=2, b=4)
    want, _ = check_packed(caller, recs, b"chrB", {}, what="ends")
    assert want.startswith(b"chrB\t%d\t%d\tCG\t6\t-\t" % (recs["core"]["pos"][0] - 2, recs["core"]["pos"][0]))
    assert want.split(b"\n")[-2].startswith(b"chrB\t%d\t%d\tCG\t4\t+\t" % (recs["core"]["pos"][n - 1] - 1, recs["core"]["pos"][n - 1] + 1))


@pytest.mark.parametrize("n, n_max", [(1, 2), (63, 64), (64, 65), (64, 128), (127, 128), (128, 129), (128, 4096), (4096, 4096 + 17)])
def test_records_beyond_the_count_do_not_exist(caller, n, n_max):
    """n_recs < max_recs, a plus half at n_recs - 1 and a valid minus half, one position on, stored at index n_recs: a single, not a pair —
    also where n_recs is a tile border, and where it is not."""
    rng = np.random.default_rng(7200 + n)
    recs = random_records(rng, n_max, "all")
    half(recs, n - 1, "+", a=3, b=1)
    half(recs, n, "-", pos=int(recs["core"]["pos"][n - 1]) + 1, a=2, b=4)
    want, tot = check_packed(caller, recs, b"chrN", {}, n=n, what="count")
    assert want.split(b"\n")[-2].startswith(b"chrN\t%d\t%d\tCG\t4\t+\t" % (recs["core"]["pos"][n - 1] - 1, recs["core"]["pos"][n - 1] + 1))
    full, ftot = check_packed(caller, recs, b"chrN", {}, what="all of them")  # with the count at the arrays' size the same two are a pair
    assert b"\t%d\tCG\t10\t.\t" % (recs["core"]["pos"][n - 1] + 1) in full and ftot[4] >= 1
    _, tot0 = check_packed(caller, recs, b"chrN", {}, n=0, what="no records")
    assert tot0 == [0, 0, 0, 0, 0]
    out, tot_over = encode_packed(caller, recs, b"chrN", {}, n=n_max + 1000)  # a count beyond the arrays: clamped
    assert tot_over == ftot and out[: ftot[0]].tobytes() == full


# ---- 2. the per-position form ----------------------------------------------------------------------------------------------------------------
def encode_sites(caller, raw, contig, par, cap):
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(5, dtype=torch.int64, device="cuda")
    caller.meth_cpg_sites_device(d_core.data_ptr(), d_aux.data_ptr(), len(raw), contig, d_out.data_ptr(), cap, d_tot.data_ptr(), params=par)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), [int(v) for v in d_tot.cpu()]


@pytest.mark.parametrize("par", [{}, {"min_cov": 5, "min_phred": 20}])
def test_sites_form_on_split_arrays(caller, par):
    rng = np.random.default_rng(7300)
    n = 4096 + 17
    recs = random_records(rng, n, "some")
    raw = recs.view(np.uint8).reshape(-1, 128).copy()
    off = raw[:, 4] == 0
    raw[off] = rng.integers(0, 256, (int(off.sum()), 128), dtype=np.uint8)  # a position without a record: garbage but for its flag
    raw[off, 4] = 0
    recs = raw.view(VCF_REC).reshape(-1)
    want, wtot = host_table(recs, b"chrS", par)
    out, tot = encode_sites(caller, raw, b"chrS", par, len(want) + 64)
    assert tot == wtot and tot[4] > 50 and out[: tot[0]].tobytes() == want and (out[tot[0] :] == PAD).all()
    packed, tot2 = encode_packed(caller, recs, b"chrS", par)
    assert tot2 == tot and packed[: tot2[0]].tobytes() == want


def launch_with_emit(caller, raw, emit, contig, par, cap):
    """The launcher behind the three entries (bsc_dev_launch_meth, cpg = 1) with the chain's emit byte per position, as bsc_block_meth_cpg_kept
    hands it over — the public per-position entry has no such array."""
    L = caller._L
    vp, u64 = C.c_void_p, C.c_uint64
    L.bsc_dev_launch_meth.restype = C.c_int
    L.bsc_dev_launch_meth.argtypes = [vp, vp, vp, vp, u64, vp, C.c_char_p, C.c_uint32, C.POINTER(_lib.MethParams), vp, vp, vp, vp, C.c_size_t, vp, u64, vp, C.c_int,
                                      C.c_int, vp]
    L.bsc_dev_scan_tmp_bytes_u64.restype = C.c_int
    L.bsc_dev_scan_tmp_bytes_u64.argtypes = [C.c_uint32, C.POINTER(C.c_size_t)]
    n = len(raw)
    n_tiles = (n + 63) // 64
    scan = C.c_size_t(0)
    assert L.bsc_dev_scan_tmp_bytes_u64(n_tiles + 1, C.byref(scan)) == 0
    d_core, d_aux, d_emit = dev(raw[:, :64]), dev(raw[:, 64:]), dev(emit)
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device="cuda")
    d_tb, d_to, d_ll, d_scan = z(8 * (n_tiles + 1)), z(8 * (n_tiles + 1)), z(128 * (n_tiles + 1)), z(scan.value)
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    mp = _lib.MethParams(**par)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rc = L.bsc_dev_launch_meth(None, d_core.data_ptr(), d_aux.data_ptr(), None, n, d_emit.data_ptr(), contig, len(contig), C.byref(mp), d_tb.data_ptr(), d_to.data_ptr(),
                               d_ll.data_ptr(), d_scan.data_ptr(), scan.value, d_out.data_ptr(), cap, d_tot.data_ptr(), 1, cus, None)
    assert rc == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), [int(v) for v in d_tot.cpu()]


@pytest.mark.parametrize("n", [2, 65, 128, 4096 + 17])
def test_sites_form_with_the_emit_byte_array(caller, n):
    """The chain's byte per position beside the records: a position whose byte is 0 has no record, whatever its bytes say — it gives no
    line and is nobody's partner.  Every tile border holds a pair by the records' bytes; the emit byte takes the minus half away at the
    even borders and the plus half at the odd ones."""
    rng = np.random.default_rng(7400 + n)
    recs = random_records(rng, n, "all")
    borders = [i for i in range(63, n - 1, 64)] or [0]
    emit = rng.choice([0, 1, 1, 1, 255], n).astype(np.uint8)
    for k, i in enumerate(borders):
        half(recs, i, "+", a=3, b=1)
        half(recs, i + 1, "-", pos=int(recs["core"]["pos"][i]) + 1, a=2, b=4)
        emit[i], emit[i + 1] = (1, 0) if k % 2 == 0 else (0, 1)
        if i:
            emit[i - 1] = 0  # (so that the plus half is nobody else's business)
        if i + 2 < n:
            emit[i + 2] = 0
    raw = recs.view(np.uint8).reshape(-1, 128)
    want, wtot = R.of_rec_bytes(raw.tobytes(), b"chrE", {}, emit=emit)
    gated = recs.copy()
    gated["core"]["emit"][emit == 0] = 0
    assert host_table(gated, b"chrE", {}) == (want, wtot)  # the host form over records whose own flag says the same
    out, tot = launch_with_emit(caller, raw, emit, b"chrE", {}, len(want) + 64)
    assert tot == wtot and out[: tot[0]].tobytes() == want and (out[tot[0] :] == PAD).all()
    for k, i in enumerate(borders):
        p = int(recs["core"]["pos"][i])
        assert (b"chrE\t%d\t%d\tCG\t%s\t" % (p - 1, p + 1, b"4\t+" if k % 2 == 0 else b"6\t-")) in want
    # without the array the same bytes pair
    out2, tot2 = encode_sites(caller, raw, b"chrE", {}, 400 * n)
    assert tot2 == host_table(recs, b"chrE", {})[1] and tot2[4] >= len(borders) and tot2 != tot


# ---- 3. placement and errors, as for the per-cytosine encoder ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "last"])
def test_a_tile_s_ragged_head_and_tail_at_every_phase(caller, which):
    """Two tiles with one line each, at the tile's first or its last record.  The contig's name grows by a byte 16 times: tile 1's span
    begins — and tile 0's ends — at every phase 0 .. 15 of a 16-byte piece; tile 1's end moves by two bytes a step, and by the odd ones
    with a GQ of one digit more in tile 0's line."""
    heads, tails = set(), set()
    base = random_records(np.random.default_rng(7500), 128, "all")
    base["core"]["emit"] = 0
    for k in range(16):
        for gq in (5, 50):
            recs = base.copy()
            for t in (0, 64):
                half(recs, t + (0 if which == "first" else 63), "+-"[t // 64], a=3, b=1)
            recs["core"]["phred"][0 if which == "first" else 63] = gq
            contig = b"q" * (1 + k)
            want, tot = check_packed(caller, recs, contig, {})
            first = want.split(b"\n")[0] + b"\n"
            assert tot[1] == 2 and tot[4] == 0
            heads.add(len(first) % 16)
            tails.add(tot[0] % 16)
    assert heads == set(range(16)) == tails


def line_sizes(recs, contig):
    sizes = np.zeros(len(recs), dtype=np.int64)
    sites = [R.site_of_rec_bytes(r.tobytes()) for r in recs]
    for i, ln, _, _, _ in R.lines(contig, sites):
        sizes[i] = len(ln)
    return sizes


def test_tiles_of_the_longest_lines_go_out_in_eight_parts(caller):
    """the wave's image is 4 KB: 16 lines of 365 bytes do not fit it, 8 do — a tile of 64 single plus halves with the longest single's line
    goes out in eight parts of 8 lanes.  Tile 1 mixes them with shorter lines; tile 2 is 32 pairs with the longest line there is (366
    bytes, at lanes 0, 2, ..: four parts); tile 3 has ten singles in every 32 lanes (two parts), tile 4 eleven in all (one part)."""
    n, contig, m = 64 * 5, b"k" * 255, 2**32 - 1
    recs = np.zeros(n, dtype=VCF_REC)
    core = recs["core"]
    core["pos"] = m - 2 * n + 2 * np.arange(n, dtype=np.uint32)
    core["emit"], core["gt"], core["flt"], core["phred"], core["cg"] = 1, 4, 128, 255, b"C"
    core["pos"][128:192] = m - 4 * n + np.arange(64)  # tile 2: consecutive positions, plus and minus in turn
    core["gt"][129:192:2] = 7
    recs["core"] = core
    recs["counts"] = m
    recs["counts"][:, 5] = m - 5
    recs["counts"][:, 6] = m - 5
    recs["counts"][64 + 20 : 64 + 50] = 3
    recs["core"]["pos"][64 + 20 : 64 + 50] = 7 + 2 * np.arange(30)
    lane = np.arange(n) % 64
    recs["core"]["emit"][(np.arange(n) // 64 == 3) & (lane % 32 >= 10)] = 0
    recs["core"]["emit"][(np.arange(n) // 64 == 4) & (lane >= 11)] = 0
    sizes = line_sizes(recs, contig)
    tile = sizes.reshape(5, 64)
    assert sizes.max() == 366 == sizes[128] and sizes[0] == 365 and sizes[:16].sum() > 4096 >= sizes[:8].sum() and 0 < sizes[64 + 20] < 320
    assert (tile[2][1::2] == 0).all() and tile[2].reshape(2, 32).sum(axis=1).min() > 4096 >= tile[2].reshape(4, 16).sum(axis=1).max()
    assert tile[3].sum() > 4096 >= tile[3].reshape(2, 32).sum(axis=1).max() and 4096 - 366 < tile[4].sum() <= 4096
    want, tot = check_packed(caller, recs, contig, {})
    assert tot[:2] == [int(sizes.sum()), int((sizes > 0).sum())] and tot[4] == 32


def test_a_stream_longer_than_the_room_is_cut_at_a_tile(caller):
    recs = random_records(np.random.default_rng(7600), 4000, "all")
    full, ftot = host_table(recs, b"chr3", {})
    sizes = line_sizes(recs, b"chr3")
    assert sizes.sum() == len(full)
    tiles = [int(sizes[t : t + 64].sum()) for t in range(0, len(sizes), 64)]
    for cap in (len(full) - 1, (len(full) // 2) & ~15):
        out, tot = encode_packed(caller, recs, b"chr3", {}, cap=cap)
        assert tot == ftot  # the full length and the full sums
        fit, at = 0, 0
        for t in tiles:  # every tile that fits whole is written, where it belongs; nothing of the others
            if at + t <= cap:
                assert out[at : at + t].tobytes() == full[at : at + t]
                fit += 1
            else:
                assert (out[at:cap] == PAD).all()
            at += t
        assert 0 < fit < len(tiles)


def test_errors_leave_the_context_usable(caller):
    L, h = caller._L, caller._h
    recs = random_records(np.random.default_rng(7700), 200, "all")
    d_recs, d_n = dev(recs), torch.tensor([200], dtype=torch.int64, device="cuda")
    d_out = torch.zeros(200 * 400, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(5, dtype=torch.int64, device="cuda")
    ok = _lib.MethParams()
    A = (d_recs.data_ptr(), d_n.data_ptr(), 200)
    Z = (C.byref(ok), d_out.data_ptr(), d_out.numel(), d_tot.data_ptr(), None)
    want = host_table(recs, b"c", {})[0]

    def refused(rc):
        assert rc == -1
        out, tot = encode_packed(caller, recs, b"c", {})
        assert out[: tot[0]].tobytes() == want

    for contig in (b"", b"a\tb", b"a\nb", b"y" * 256, None):
        refused(L.bsc_meth_cpg_block_device(h, *A, contig, *Z))
        refused(L.bsc_meth_cpg_sites_device(h, d_recs.data_ptr(), d_recs.data_ptr(), 100, contig, *Z))
    refused(L.bsc_meth_cpg_block_device(h, *A, b"c", None, *Z[1:]))
    refused(L.bsc_meth_cpg_block_device(h, *A, b"c", C.byref(_lib.MethParams(contexts=2)), *Z[1:]))
    rc = L.bsc_meth_cpg_block_device(h, *A, b"c", C.byref(_lib.MethParams(contexts=R_ALL)), *Z[1:])
    assert b"partner strand" in L.bsc_last_error()
    refused(rc)
    refused(L.bsc_meth_cpg_sites_device(h, d_recs.data_ptr(), d_recs.data_ptr(), 100, b"c", C.byref(_lib.MethParams(contexts=R_ALL)), *Z[1:]))
    rc = L.bsc_meth_cpg_block_device(h, *A, b"c", C.byref(ok), d_out.data_ptr() + 8, 1000, d_tot.data_ptr(), None)
    assert b"aligned" in L.bsc_last_error()
    refused(rc)
    refused(L.bsc_meth_cpg_block_device(h, *A, b"c", C.byref(ok), None, 1000, d_tot.data_ptr(), None))
    refused(L.bsc_meth_cpg_block_device(h, *A, b"c", C.byref(ok), d_out.data_ptr(), 1000, None, None))
    refused(L.bsc_meth_cpg_block_device(h, None, d_n.data_ptr(), 200, b"c", *Z))
    refused(L.bsc_meth_cpg_block_device(None, *A, b"c", *Z))
    nb, nl = C.c_uint64(0), C.c_uint64(0)
    with B.SiteCaller() as fresh:  # nothing kept
        assert L.bsc_block_meth_cpg_kept(fresh._h, b"c", C.byref(ok), 4096, C.byref(nb), C.byref(nl), None) == -1
        assert b"no single block" in L.bsc_last_error()


R_ALL = 1  # BSC_METH_ALL


# ---- 4. the block entry ----------------------------------------------------------------------------------------------------------------------
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
    """A BAM of three contigs: 6 000 positions at ~40x with CpGs read from both strands (pairs), one of 60 positions (a block shorter than a
    tile), and 30 000 positions covered thinly in several blocks — there most CpGs are read from one strand only (singles).  The CPU oracle
    chain over this file gives, by the Python rule at default parameters, 444 pairs, 286 single plus and 285 single minus halves."""
    d = tmp_path_factory.mktemp("methcpg_files")
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


def strands_of(table):
    col = [ln.split(b"\t")[5] for ln in table.split(b"\n") if ln]
    return {s: col.count(s.encode()) for s in (".", "+", "-")}


PARS = [{}, {"min_phred": 30}, {"min_cov": 12, "min_phred": 30, "pass_only": 1}]


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    n_blocks = n_short = 0
    seen = {tuple(sorted(p.items())): {".": 0, "+": 0, "-": 0} for p in PARS}
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            n_short += y - x + 1 < 64
            # the block without any table: its stream and its index entries
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
            ent0, r0 = caller.block_csi_kept(14)
            bcf1, n_rec1, _ = caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
            sites = [R.site_of_bcf_record(dec) for dec in R.bcf_records(bcf0)]  # what the file itself says of the block's records
            for par in PARS:
                table, lines, sums = caller.block_meth_kept(name, par, merge=True)
                want, wtot = R.table(name.encode(), sites, par)
                assert table == want and [len(table), lines, *sums] == wtot, (name, x, par)
                for s, k in strands_of(want).items():
                    seen[tuple(sorted(par.items()))][s] += k
                # the same parameters with min_cov = 1 against the per-cytosine table: the same counts, a line less per pair
                par1 = dict(par, min_cov=1)
                t1, l1, s1 = caller.block_meth_kept(name, par1, merge=True)
                tc, lc, sc = caller.block_meth_kept(name, par1)
                assert s1[:2] == sc and l1 == lc - s1[2], (name, x, par)
                rows = methbed.parse_bed(t1)
                assert s1[:2] == (int(rows["a"].sum()), int(rows["b"].sum())) and s1[2] == int((rows["strand"] == ".").sum()) if len(rows) else s1 == (0, 0, 0)
            assert kept_stream(caller, len(bcf0)) == bcf0 == bcf1 and n_rec1 == n_rec
            ent2, r2 = caller.block_csi_kept(14)
            assert ent0.tobytes() == ent2.tobytes() and r0 == r2 == n_rec
            # too little room, then the room asked for; the table is read and handed over like the per-cytosine one
            table, lines, _ = caller.block_meth_kept(name, merge=True)
            nb, nl = C.c_uint64(0), C.c_uint64(0)
            ok = _lib.MethParams()
            if table:
                assert L.bsc_block_meth_cpg_kept(h, name.encode(), C.byref(ok), len(table) - 1, C.byref(nb), C.byref(nl), None) == -1
                assert nb.value == len(table) and b"dev_cap" in L.bsc_last_error()
            sums = (C.c_uint64 * 3)()
            assert L.bsc_block_meth_cpg_kept(h, name.encode(), C.byref(ok), max(len(table), 1), C.byref(nb), C.byref(nl), sums) == 0
            out = np.zeros(len(table) + 1, np.uint8)
            assert L.bsc_meth_stream_read(h, 0, len(table), out.ctypes.data) == 0
            caller.synchronize()
            assert (nb.value, nl.value) == (len(table), lines) and out[:-1].tobytes() == table
            assert L.bsc_meth_stream_read(h, 1, len(table), out.ctypes.data) == -1
            assert L.bsc_block_meth_cpg_kept(h, name.encode(), C.byref(_lib.MethParams(contexts=R_ALL)), 1 << 20, C.byref(nb), C.byref(nl), None) == -1
            # behind the text encoder's keep call: the same table, the kept lines untouched
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, reg_stop=len(codes))
            table_v, lines_v, _ = caller.block_meth_kept(name, merge=True)
            assert table_v == table and lines_v == lines and n_txt == n_rec and kept_stream(caller, len(text)) == text
            n_blocks += 1
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes))
            assert L.bsc_block_meth_cpg_kept(h, name.encode(), C.byref(ok), 1 << 20, C.byref(nb), C.byref(nl), None) == -1
            assert b"no single block" in L.bsc_last_error() and nb.value == 0
    assert n_blocks > 3 and n_short >= 1
    for par, k in seen.items():  # the run holds pairs, single plus and single minus halves — at the default parameters already
        assert k["."] >= 1 and k["+"] >= 1 and k["-"] >= 1, (par, k)
    assert seen[()]["."] > 300 and seen[()]["+"] > 100 and seen[()]["-"] > 100


# ---- 5. file to file -------------------------------------------------------------------------------------------------------------------------
def run_exe(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


def test_bam2bcf_meth_merge_and_pipeline(small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    names = [r[0].encode() for r in refs]
    p = lambda s: str(d / ("g" + s))
    base = run_exe(bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    plain = open(p(".u.bcf"), "rb").read()
    want, wtot = R.of_bcf_file(plain, names)
    assert wtot[1] > 300 and strands_of(want)["."] == wtot[4] > 300 and strands_of(want)["+"] > 100 and strands_of(want)["-"] > 100
    # -O u and -O b, the main file and the report unchanged
    out_u = run_exe("--meth", p(".u.bed"), "--meth-merge", bam, fa, p(".um.bcf"), p(".um.json"), "S9")
    assert open(p(".u.bed"), "rb").read() == want and open(p(".um.bcf"), "rb").read() == plain
    assert open(p(".um.json")).read() == open(p(".u.json")).read() and out_u == base + "%d methylation table lines written\n" % wtot[1]
    run_exe("-O", "b", bam, fa, p(".b.bcf"), p(".b.json"), "S9")
    run_exe("-O", "b", "--meth-merge", "--meth", p(".b.bed.gz"), bam, fa, p(".bm.bcf"), p(".bm.json"), "S9")
    comp = open(p(".b.bed.gz"), "rb").read()
    assert comp.endswith(vcf.BGZF_EOF) and gzip.decompress(comp) == want
    assert open(p(".bm.bcf"), "rb").read() == open(p(".b.bcf"), "rb").read() and gzip.decompress(open(p(".b.bcf"), "rb").read()) == plain
    # start strictly increasing within each contig
    bed = methbed.read_bed(p(".u.bed"))
    assert len(bed) == wtot[1] and set(bed["name"]) == {"CG"} and set(bed["strand"]) == {"+", "-", "."}
    for nm in set(bed["chrom"]):
        st = bed["start"][bed["chrom"] == nm].astype(np.int64)
        assert (np.diff(st) > 0).all(), nm
    assert (bed["end"] == bed["start"] + 2).all()
    # the thresholds
    par = {"min_cov": 12, "min_phred": 30, "pass_only": 1}
    run_exe("--meth", p(".t.bed"), "--meth-merge", "--meth-min-cov", "12", "--meth-min-gq", "30", "--meth-pass", bam, fa, p(".t.bcf"), p(".t.json"))
    got = open(p(".t.bed"), "rb").read()
    assert got == R.of_bcf_file(plain, names, par)[0] and 0 < got.count(b"\n") < wtot[1]
    # --format vcf -O b --index -D with the combined table: the main file, the .csi and the report are those of the run without it
    import dbsnp_crafted as K

    idx = K.write(d / "methcpg.idx", {"chrA": K.random_sites(6_000, 40, 33)})
    opts = ["--format", "vcf", "-O", "b", "--index", "-D", idx]
    run_exe(*opts, bam, fa, p(".v.gz"), p(".v.json"), "S9")
    run_exe(*opts, "--meth", p(".v.bed.gz"), "--meth-merge", bam, fa, p(".vm.gz"), p(".vm.json"), "S9")
    assert open(p(".vm.gz"), "rb").read() == open(p(".v.gz"), "rb").read() and open(p(".vm.gz.csi"), "rb").read() == open(p(".v.gz.csi"), "rb").read()
    assert open(p(".vm.json")).read() == open(p(".v.json")).read() and gzip.decompress(open(p(".v.bed.gz"), "rb").read()) == want
    # pipeline.run(meth_merge=True) writes the same table, beside either format
    for text in (False, True):
        for compressed in (False, True):
            out = p(".pipe%d%d" % (text, compressed))
            s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, text=text, compressed=compressed, meth_path=out + ".bed",
                             meth_merge=True)
            got = open(out + ".bed", "rb").read()
            assert (gzip.decompress(got) if compressed else got) == want and s["meth_lines"] == wtot[1]
            if not text and not compressed:
                assert open(out, "rb").read() == plain
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, meth_merge=True)
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no2"), device_reader=True, meth_path=p(".no2.bed"), meth_merge=True, meth_params={"contexts": R_ALL})
    assert not os.path.exists(p(".no")) and not os.path.exists(p(".no2")) and not os.path.exists(p(".no2.bed"))
