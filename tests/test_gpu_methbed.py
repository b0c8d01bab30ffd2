"""The methylation table on the device (csrc/methdev.hip): the encoder against the host form (bsc_meth_format_rec) byte for byte — both
input forms, every phase of a tile's span, the parts path, capacity, the totals —, the block entry behind both _keep calls against the
Python formatter (tests/methbed_ref.py) over the DECODED BCF of the same block, against the report's own CpG counters, and file to file
(bam2bcf --meth, pipeline.run(meth_path=...))."""
import ctypes as C
import gzip
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

import bs_call_amd as B
import methbed_ref as R
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
PARAMS = [{}, {"contexts": R.ALL}]


@pytest.fixture(scope="module")
def caller():
    with B.SiteCaller() as c:
        yield c


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def host_lines(recs, contig, par):
    p = _lib.MethParams(**par)
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 128)
    return [methbed.format_recs(raw[i : i + 1], contig, p) for i in range(len(raw))]


def host_sums(recs, lines):
    """{lines, sum of a, sum of b} of the records that gave a line, read from the records."""
    a = b = 0
    for r, ln in zip(recs, lines):
        if ln:
            minus = int(r["core"]["gt"]) == 7
            a += int(r["counts"][6 if minus else 5])
            b += int(r["counts"][4 if minus else 7])
    return [sum(1 for ln in lines if ln), a, b]


def random_records(rng, n, present="some"):
    """Random bytes in every field; emit, gt, cg and the counts then drawn so that records give lines.  present: "some" (about a third,
    with stretches of none longer than a tile), "none", "all", "first" / "last" (only that record of every tile of 64)."""
    raw = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    recs = raw.view(VCF_REC).reshape(-1)
    if not n:
        return recs
    core = recs["core"]
    core["emit"] = rng.choice([0, 1, 1, 1, 1, 255], n)
    core["gt"] = rng.choice([4, 7, 4, 7, 0, 5, 36], n)
    core["flt"] = rng.choice([0, 0, 0, 1, 8, 128, 143], n)
    core["cg"] = rng.choice(list(b"CCHHN?"), n).astype(np.uint8).view("S1")
    scale = rng.choice([0, 1, 3, 30, 1000, 70000, 2**32 - 1], (n, 8))
    recs["counts"] = (rng.random((n, 8)) * (scale + 1)).astype(np.uint64).clip(0, 2**32 - 1).astype(np.uint32)
    if present != "some":
        core["emit"], core["gt"], core["cg"] = 1, rng.choice([4, 7], n), rng.choice(list(b"CH"), n).astype(np.uint8).view("S1")
        recs["counts"] = np.maximum(recs["counts"], 1)
        lane = np.arange(n) % 64
        off = {"none": np.ones(n, bool), "all": np.zeros(n, bool), "first": lane != 0, "last": (lane != 63) & (np.arange(n) != n - 1)}[present]
        core["emit"][off] = 0
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
    d_tot = torch.full((4,), 77, dtype=torch.int64, device="cuda")
    caller.meth_block_device(d_recs.data_ptr(), d_n.data_ptr(), len(recs), contig, d_out.data_ptr(), cap, d_tot.data_ptr(), params=par)
    torch.cuda.synchronize()
    tot = [int(v) for v in d_tot.cpu().numpy().view(np.uint64)]
    out = d_out.cpu().numpy()
    assert (out[cap:] == PAD).all()  # nothing behind the room given
    if tot[0] <= cap:
        assert (out[tot[0] : tot[0] + 16] == PAD).all() and (out[tot[0] : cap] == PAD).all()  # nothing behind the stream's end
    return out[:cap], tot


# ---- 1. the encoder against the host form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par", PARAMS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4096 + 17])
def test_packed_records_equal_the_host_lines(caller, n, par):
    rng = np.random.default_rng(5000 + n)
    for present in ("some", "none", "all", "first", "last") if n else ("some",):
        recs = random_records(rng, n, present)
        contig = [b"c", b"chr1", b"chrUn_KI270742v1"][n % 3]
        want = host_lines(recs, contig, par)
        out, tot = encode_packed(caller, recs, contig, par)
        stream = b"".join(want)
        assert tot == [len(stream)] + host_sums(recs, want), (present, tot)
        assert out[: tot[0]].tobytes() == stream, present
        if present == "all" and par:  # (CpG only: the 'H' records give no line)
            assert tot[1] == n
        if present in ("first", "last") and par:
            assert tot[1] == (n + 63) // 64
        if present == "none":
            assert tot == [0, 0, 0, 0]
    if n == 4096 + 17:  # the thresholds, on the device as on the host
        par2 = dict(par, min_cov=5, min_phred=100, pass_only=1)
        want = host_lines(recs, contig, par2)
        out, tot = encode_packed(caller, recs, contig, par2)
        assert 0 < tot[1] < n and out[: tot[0]].tobytes() == b"".join(want) and tot == [len(b"".join(want))] + host_sums(recs, want)


@pytest.mark.parametrize("which", ["first", "last"])
def test_a_tile_s_ragged_head_and_tail_at_every_phase(caller, which):
    """Two tiles with one line each, at the tile's first or its last record.  The contig's name grows by a byte 16 times: tile 1's span
    begins — and tile 0's ends — at every phase 0 .. 15 of a 16-byte piece; tile 1's end moves by two bytes a step, and by the odd ones
    with a GQ of one digit more in tile 0's line."""
    heads, tails = set(), set()
    for k in range(16):
        for gq in (5, 50):
            recs = random_records(np.random.default_rng(600), 128, which)
            recs["core"]["phred"][0 if which == "first" else 63] = gq
            contig = b"q" * (1 + k)
            want = [w for w in host_lines(recs, contig, {"contexts": R.ALL}) if w]
            out, tot = encode_packed(caller, recs, contig, {"contexts": R.ALL})
            assert tot[1] == 2 == len(want) and out[: tot[0]].tobytes() == b"".join(want)
            heads.add(len(want[0]) % 16)
            tails.add(tot[0] % 16)
    assert heads == set(range(16)) == tails


def test_tiles_of_the_longest_lines_go_out_in_eight_parts(caller):
    """the wave's image is 4 KB: 16 lines of 366 bytes do not fit it, 8 do — a tile of 64 of them goes out in eight parts of 8 lanes.  Tile 1
    mixes them with shorter lines, so that its parts differ in what they hold; tile 2 has 8 lines in every 16 lanes (four parts), tile 3 ten
    in every 32 (two parts), tile 4 eleven in all (4 026 bytes: one part)."""
    n, contig, m = 64 * 5, b"k" * 255, 2**32 - 1
    recs = np.zeros(n, dtype=VCF_REC)
    core = recs["core"]
    core["pos"] = m - np.arange(n, dtype=np.uint32)[::-1]
    core["emit"], core["gt"], core["flt"], core["phred"], core["cg"], core["cx_gt"] = 1, 7, 128, 255, b"H", b"NNNNN"
    recs["core"] = core
    recs["counts"] = m
    recs["counts"][:, 6] = m - 5
    recs["counts"][64 + 20 : 64 + 50] = 3
    recs["core"]["pos"][64 + 20 : 64 + 50] = 7
    lane = np.arange(n) % 64
    recs["core"]["emit"][(np.arange(n) // 64 == 2) & (lane % 16 >= 8)] = 0
    recs["core"]["emit"][(np.arange(n) // 64 == 3) & (lane % 32 >= 10)] = 0
    recs["core"]["emit"][(np.arange(n) // 64 == 4) & (lane >= 11)] = 0
    want = host_lines(recs, contig, {"contexts": R.ALL})
    sizes = np.array([len(w) for w in want])
    tile = sizes.reshape(5, 64)
    assert sizes.max() == 366 == sizes[0] and sizes[:16].sum() > 4096 >= sizes[:8].sum() and 0 < sizes[64 + 20] < 320
    assert tile[2].reshape(2, 32).sum(axis=1).min() > 4096 >= tile[2].reshape(4, 16).sum(axis=1).max()
    assert tile[3].sum() > 4096 >= tile[3].reshape(2, 32).sum(axis=1).max() and 4096 - 366 < tile[4].sum() <= 4096
    out, tot = encode_packed(caller, recs, contig, {"contexts": R.ALL})
    assert tot[:2] == [int(sizes.sum()), int((sizes > 0).sum())] and out[: tot[0]].tobytes() == b"".join(want)


def test_a_stream_longer_than_the_room_is_cut_at_a_tile(caller):
    recs = random_records(np.random.default_rng(5200), 4000, "all")
    lines = host_lines(recs, b"chr3", {})
    full = b"".join(lines)
    for cap in (len(full) - 1, (len(full) // 2) & ~15):
        out, tot = encode_packed(caller, recs, b"chr3", {}, cap=cap)
        assert tot == [len(full)] + host_sums(recs, lines)
        tiles = [sum(len(w) for w in lines[t : t + 64]) for t in range(0, len(lines), 64)]
        fit, at = 0, 0
        for t in tiles:  # every tile that fits whole is written, where it belongs; nothing of the others
            if at + t <= cap:
                assert out[at : at + t].tobytes() == full[at : at + t]
                fit += 1
            else:
                assert (out[at:cap] == PAD).all()
            at += t
        assert 0 < fit < len(tiles)
    out, tot = encode_packed(caller, recs, b"chr3", {}, n=333)  # the count on the device limits the records
    want = b"".join(lines[:333])
    assert tot[0] == len(want) and out[: tot[0]].tobytes() == want


# ---- 2. the per-position form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par", PARAMS)
def test_sites_form_on_split_arrays(caller, par):
    rng = np.random.default_rng(5300)
    n = 4096 + 17
    recs = random_records(rng, n, "some")
    raw = recs.view(np.uint8).reshape(-1, 128).copy()
    off = raw[:, 4] == 0
    raw[off] = rng.integers(0, 256, (int(off.sum()), 128), dtype=np.uint8)  # a position without a record: garbage but for its flag
    raw[off, 4] = 0
    recs = raw.view(VCF_REC).reshape(-1)
    want = b"".join(host_lines(recs, b"chrS", par))
    d_core, d_aux = dev(raw[:, :64]), dev(raw[:, 64:])
    cap = len(want) + 64
    d_out = torch.full((cap + 64,), PAD, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    caller.meth_sites_device(d_core.data_ptr(), d_aux.data_ptr(), n, b"chrS", d_out.data_ptr(), cap, d_tot.data_ptr(), params=par)
    torch.cuda.synchronize()
    tot = [int(v) for v in d_tot.cpu()]
    out = d_out.cpu().numpy()
    assert tot[0] == len(want) and tot[1] == want.count(b"\n") > 300 and out[: tot[0]].tobytes() == want and (out[tot[0] :] == PAD).all()
    packed, tot2 = encode_packed(caller, recs, b"chrS", par)
    assert tot2 == tot and packed[: tot2[0]].tobytes() == want


def test_errors_leave_the_context_usable(caller):
    L, h = caller._L, caller._h
    recs = random_records(np.random.default_rng(5400), 200, "all")
    d_recs, d_n = dev(recs), torch.tensor([200], dtype=torch.int64, device="cuda")
    d_out = torch.zeros(200 * 400, dtype=torch.uint8, device="cuda")
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    ok = _lib.MethParams()
    A = (d_recs.data_ptr(), d_n.data_ptr(), 200)
    Z = (C.byref(ok), d_out.data_ptr(), d_out.numel(), d_tot.data_ptr(), None)
    want = b"".join(host_lines(recs, b"c", {}))

    def refused(rc):
        assert rc == -1
        out, tot = encode_packed(caller, recs, b"c", {})
        assert out[: tot[0]].tobytes() == want

    for contig in (b"", b"a\tb", b"a\nb", b"y" * 256, None):
        refused(L.bsc_meth_block_device(h, *A, contig, *Z))
        refused(L.bsc_meth_sites_device(h, d_recs.data_ptr(), d_recs.data_ptr(), 100, contig, *Z))
    refused(L.bsc_meth_block_device(h, *A, b"c", None, *Z[1:]))
    refused(L.bsc_meth_block_device(h, *A, b"c", C.byref(_lib.MethParams(contexts=2)), *Z[1:]))
    rc = L.bsc_meth_block_device(h, *A, b"c", C.byref(ok), d_out.data_ptr() + 8, 1000, d_tot.data_ptr(), None)
    assert b"aligned" in L.bsc_last_error()
    refused(rc)
    refused(L.bsc_meth_block_device(h, *A, b"c", C.byref(ok), None, 1000, d_tot.data_ptr(), None))
    refused(L.bsc_meth_block_device(h, *A, b"c", C.byref(ok), d_out.data_ptr(), 1000, None, None))
    refused(L.bsc_meth_block_device(h, None, d_n.data_ptr(), 200, b"c", *Z))
    refused(L.bsc_meth_block_device(None, *A, b"c", *Z))
    nb, nl = C.c_uint64(0), C.c_uint64(0)
    with B.SiteCaller() as fresh:  # nothing kept
        assert L.bsc_block_meth_kept(fresh._h, b"c", C.byref(ok), 4096, C.byref(nb), C.byref(nl), None) == -1
        assert b"no single block" in L.bsc_last_error()
        out = np.zeros(16, np.uint8)
        assert L.bsc_meth_stream_read(fresh._h, 0, 1, out.ctypes.data) == -1
        p = C.c_void_p()
        assert L.bsc_meth_stream_detach(fresh._h, C.byref(p), C.byref(nb)) == -1


# ---- 3. the block entry, 4. the report's counters -------------------------------------------------------------------------------------------
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
    """A BAM of three contigs: 6 000 positions at ~40x with CpGs read from both strands, one of 60 positions (a block shorter than a tile),
    and 3 000 positions in several blocks (gaps between the reads)."""
    d = tmp_path_factory.mktemp("meth_files")
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


def vcf_table(text, par):
    """The table of a block's VCF lines: the same columns read from the text form of the same run."""
    out = []
    for ln in text.split(b"\n"):
        if not ln:
            continue
        f = ln.split(b"\t")
        keys, vals = f[8].split(b":"), f[9].split(b":")
        s = dict(zip(keys, vals))
        alleles = [f[3]] + ([] if f[4] == b"." else f[4].split(b","))
        bases = [alleles[int(i)] for i in s[b"GT"].split(b"/")]
        strand = "+" if bases == [b"C", b"C"] else ("-" if bases == [b"G", b"G"] else None)
        out.append(R.line(f[0], int(f[1]), strand, s[b"CG"][0], s[b"CX"], [int(v) for v in s[b"MC8"].split(b",")], int(s[b"GQ"]), f[6].decode(), par))
    return b"".join(out)


def test_block_entry_behind_both_keep_calls(caller, small):
    _, bam, _, refs, reference = small
    L, h = caller._L, caller._h
    n_blocks = n_lines = n_short = 0
    labels = set()
    with DeviceBamReader(caller, bam, threads=2) as rd:
        for blk in rd.device_blocks():
            name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
            x, y = int(blk.x), int(blk.y)
            ref = block_reference(codes, x, y)
            n_short += y - x + 1 < 64
            # the block without the table: its stream and its index entries
            bcf0, n_rec, _ = caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
            ent0, r0 = caller.block_csi_kept(14)
            # ... and with it: keep -> csi_kept -> meth_kept -> reads of both streams
            bcf1, n_rec1, _ = caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), keep=True)
            ent1, r1 = caller.block_csi_kept(14)
            for par in PARAMS + [{"contexts": R.ALL, "min_cov": 12, "min_phred": 30, "pass_only": 1}]:
                table, lines, sums = caller.block_meth_kept(name, par)
                want = R.of_bcf_stream(bcf0, name.encode(), par)
                assert table == want and lines == want.count(b"\n"), (name, x, par)
                rows = methbed.parse_bed(table)
                assert sums == (int(rows["a"].sum()), int(rows["b"].sum()))
                labels |= set(rows["name"])
            assert kept_stream(caller, len(bcf0)) == bcf0 == bcf1 and n_rec1 == n_rec
            ent2, r2 = caller.block_csi_kept(14)
            assert ent1.tobytes() == ent0.tobytes() == ent2.tobytes() and r0 == r1 == r2 == n_rec
            # too little room, then the room asked for
            table, lines, _ = caller.block_meth_kept(name)
            nb, nl = C.c_uint64(0), C.c_uint64(0)
            ok = _lib.MethParams()
            if table:
                assert L.bsc_block_meth_kept(h, name.encode(), C.byref(ok), len(table) - 1, C.byref(nb), C.byref(nl), None) == -1
                assert nb.value == len(table) and b"dev_cap" in L.bsc_last_error()
            sums = (C.c_uint64 * 2)()
            assert L.bsc_block_meth_kept(h, name.encode(), C.byref(ok), max(len(table), 1), C.byref(nb), C.byref(nl), sums) == 0
            out = np.zeros(len(table) + 1, np.uint8)
            assert L.bsc_meth_stream_read(h, 0, len(table), out.ctypes.data) == 0
            caller.synchronize()
            assert (nb.value, nl.value) == (len(table), lines) and out[:-1].tobytes() == table
            assert L.bsc_meth_stream_read(h, 1, len(table), out.ctypes.data) == -1
            # behind the text encoder's keep call: the same table, the kept lines untouched
            text, n_txt, _ = caller.block_vcf_rawdev(blk, ref, name, reg_stop=len(codes))
            table_v, lines_v, _ = caller.block_meth_kept(name)
            assert table_v == table == vcf_table(text, {}) and n_txt == n_rec and kept_stream(caller, len(text)) == text
            n_blocks += 1
            n_lines += lines
            # refused behind a call that kept nothing
            caller.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes))
            assert L.bsc_block_meth_kept(h, name.encode(), C.byref(ok), 1 << 20, C.byref(nb), C.byref(nl), None) == -1
            assert b"no single block" in L.bsc_last_error() and nb.value == 0
    assert n_blocks > 3 and n_short >= 1 and n_lines > 300 and labels >= {"CG", "CHG", "CHH"}


@pytest.mark.parametrize("pass_only", [0, 1])
def test_lines_equal_the_report_s_cpg_counters(small, pass_only):
    """Every site the table lists under the default parameters adds a posterior over 101 levels that sums to 1 to CpG_ref_meth or
    CpG_nonref_meth (src/print_vcf.c:491-514): their sum is the number of lines, up to the rounding of the additions."""
    _, bam, _, refs, reference = small
    lines = 0
    with B.SiteCaller() as c:
        c.reset_site_stats()
        with DeviceBamReader(c, bam, threads=2) as rd:
            for blk in rd.device_blocks():
                name, codes = refs[int(blk.tid)][0], reference[refs[int(blk.tid)][0]]
                ref = block_reference(codes, int(blk.x), int(blk.y))
                c.block_bcf_rawdev(blk, ref, int(blk.tid), reg_stop=len(codes), with_stats=True, keep=True)
                lines += c.block_meth_kept(name, {"pass_only": pass_only})[1]
        st = c.site_stats()
    total = float(np.sum(st["CpG_ref_meth"][pass_only]) + np.sum(st["CpG_nonref_meth"][pass_only]))
    print("lines %d, counters %.9f" % (lines, total))
    assert lines > 100 and lines == round(total) and abs(total - lines) <= 1e-6 * max(1, lines)


# ---- 5. file to file ----------------------------------------------------------------------------------------------------------------------
def run_exe(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


def file_table(plain_bcf, refs, par):
    """The table of a whole uncompressed BCF file, contig by contig, from its own records."""
    import struct

    from oracle import py_bcf

    (lt,) = struct.unpack_from("<I", plain_bcf, 5)
    at, out = 9 + lt, []
    while at < len(plain_bcf):
        ls, li = struct.unpack_from("<II", plain_bcf, at)
        d = py_bcf.decode_record(plain_bcf[at : at + 8 + ls + li])
        out.append(R.of_bcf_record(d, refs[d["rid"]][0].encode(), par))
        at += 8 + ls + li
    return b"".join(out)


def test_bam2bcf_meth_and_pipeline(small):
    assert os.path.exists(EXE), "run `make demo`"
    d, bam, fa, refs, reference = small
    p = lambda s: str(d / ("f" + s))
    base = run_exe(bam, fa, p(".u.bcf"), p(".u.json"), "S9")
    plain = open(p(".u.bcf"), "rb").read()
    want = file_table(plain, refs, {})
    assert want.count(b"\n") > 300
    # -O u and -O b, the main file and the report unchanged
    out_u = run_exe("--meth", p(".u.bed"), bam, fa, p(".um.bcf"), p(".um.json"), "S9")
    assert open(p(".u.bed"), "rb").read() == want and open(p(".um.bcf"), "rb").read() == plain
    assert open(p(".um.json")).read() == open(p(".u.json")).read() and out_u == base + "%d methylation table lines written\n" % want.count(b"\n")
    run_exe("-O", "b", bam, fa, p(".b.bcf"), p(".b.json"), "S9")
    run_exe("-O", "b", "--meth", p(".b.bed.gz"), bam, fa, p(".bm.bcf"), p(".bm.json"), "S9")
    comp = open(p(".b.bed.gz"), "rb").read()
    assert comp.endswith(vcf.BGZF_EOF) and gzip.decompress(comp) == want
    assert open(p(".bm.bcf"), "rb").read() == open(p(".b.bcf"), "rb").read() and gzip.decompress(open(p(".b.bcf"), "rb").read()) == plain
    # every context, the thresholds
    par = {"contexts": R.ALL, "min_cov": 12, "min_phred": 30, "pass_only": 1}
    run_exe("--meth", p(".all.bed"), "--meth-all", "--meth-min-cov", "12", "--meth-min-gq", "30", "--meth-pass", bam, fa, p(".all.bcf"), p(".all.json"))
    got = open(p(".all.bed"), "rb").read()
    assert got == file_table(plain, refs, par) and 0 < got.count(b"\n") and b"\tCHH\t" in got
    # --format vcf -O b --index -D with --meth: the main file, the .csi and the report are those of the run without it
    import dbsnp_crafted as K

    idx = K.write(d / "meth.idx", {"chrA": K.random_sites(6_000, 40, 33)})
    opts = ["--format", "vcf", "-O", "b", "--index", "-D", idx]
    run_exe(*opts, bam, fa, p(".v.gz"), p(".v.json"), "S9")
    run_exe(*opts, "--meth", p(".v.bed.gz"), bam, fa, p(".vm.gz"), p(".vm.json"), "S9")
    assert open(p(".vm.gz"), "rb").read() == open(p(".v.gz"), "rb").read() and open(p(".vm.gz.csi"), "rb").read() == open(p(".v.gz.csi"), "rb").read()
    assert open(p(".vm.json")).read() == open(p(".v.json")).read()
    assert gzip.decompress(open(p(".v.bed.gz"), "rb").read()) == vcf_table(gzip.decompress(open(p(".vm.gz"), "rb").read()).split(b"\tS9\n", 1)[1], {})
    # pipeline.run(meth_path=...) writes the same table, beside either format
    for text in (False, True):
        for compressed in (False, True):
            out = p(".pipe%d%d" % (text, compressed))
            s = pipeline.run(bam, reference, out, sample="S9", benchmark_mode=True, device_reader=True, text=text, compressed=compressed, meth_path=out + ".bed")
            got = open(out + ".bed", "rb").read()
            assert (gzip.decompress(got) if compressed else got) == want and s["meth_lines"] == want.count(b"\n")
    bed = methbed.read_bed(p(".pipe01.bed"))
    assert len(bed) == want.count(b"\n") and set(bed["name"]) == {"CG"} and set(bed["strand"]) == {"+", "-"}
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), meth_path=p(".no.bed"))
    with pytest.raises(ValueError):
        pipeline.run(bam, reference, p(".no"), device_reader=True, meth_path=p(".no.bed"), shard_rank=0, shard_world=2)
    assert not os.path.exists(p(".no")) and not os.path.exists(p(".no.bed"))
