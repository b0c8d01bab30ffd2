"""The methylation tables (bedMethyl): the host form of the per-cytosine line (bsc_meth_format_rec, csrc/methbed.c) and of the
combined-strand CpG table (bsc_meth_cpg_format_recs, csrc/methcpg.c) — the checkers of the device's encoders, csrc/methdev.hip — and a
reader of the files bam2bcf --meth [--meth-merge] / pipeline.run(meth_path=..., meth_merge=...) write.  include/bscall_amd.h has the rules
and the columns."""
import ctypes as C
import gzip

import numpy as np

from . import _lib

CPG, ALL = 0, 1  # BSC_METH_CPG, BSC_METH_ALL

BED = np.dtype([("chrom", "O"), ("start", "<u8"), ("end", "<u8"), ("name", "O"), ("score", "<u4"), ("strand", "O"), ("thick_start", "<u8"),
                ("thick_end", "<u8"), ("rgb", "O"), ("coverage", "<u8"), ("pct", "<u4"), ("a", "<u8"), ("b", "<u8"), ("gq", "<u4"), ("filter", "O")])


def params(contexts=CPG, min_cov=1, min_phred=0, pass_only=False):
    return _lib.MethParams(contexts, min_cov, min_phred, 1 if pass_only else 0)


def format_rec(rec, contig, p=None, cap=512):
    """The line of one packed record (a VCF_REC element, or its 128 bytes): bytes, b"" when the record gives none."""
    L = _lib.load()
    raw = rec if isinstance(rec, (bytes, bytearray)) else np.asarray(rec).tobytes()
    if len(raw) != 128:
        raise ValueError("a packed record has 128 bytes")
    p = params() if p is None else p
    buf = C.create_string_buffer(max(int(cap), 1))
    n = L.bsc_meth_format_rec(raw, contig if isinstance(contig, (bytes, bytearray)) else str(contig).encode(), C.byref(p), buf, int(cap))
    if n < 0:
        raise ValueError("bsc_meth_format_rec: bad argument")
    if n > cap:
        return format_rec(raw, contig, p, n)
    return buf.raw[:n]


def format_recs(recs, contig, p=None):
    """The table of packed records (VCF_REC[]): the lines of those that give one, concatenated."""
    L = _lib.load()
    rb = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 128)
    p = params() if p is None else p
    name = contig if isinstance(contig, (bytes, bytearray)) else str(contig).encode()
    buf = C.create_string_buffer(512)
    base, out = rb.ctypes.data, []
    for i in range(len(rb)):
        n = L.bsc_meth_format_rec(base + 128 * i, name, C.byref(p), buf, 512)
        if n < 0:
            raise ValueError("bsc_meth_format_rec: bad argument")
        out.append(buf.raw[:n])
    return b"".join(out)


def format_cpg_recs(recs, contig, p=None, totals=False):
    """The combined-strand CpG table of packed records (VCF_REC[]) in order: one line per CpG dinucleotide, both strands' counts added
    (bsc_meth_cpg_format_recs, csrc/methcpg.c — the checker of the device's combined encoder).  totals: return (bytes, [length, lines,
    sum of A, sum of B, pairs written]) instead of the bytes alone."""
    L = _lib.load()
    rb = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, 128)
    p = params() if p is None else p
    name = contig if isinstance(contig, (bytes, bytearray)) else str(contig).encode()
    tot = (C.c_uint64 * 5)()
    base = rb.ctypes.data if len(rb) else None
    n = L.bsc_meth_cpg_format_recs(base, len(rb), name, C.byref(p), None, 0, tot)
    if n < 0:
        raise ValueError("bsc_meth_cpg_format_recs: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    if L.bsc_meth_cpg_format_recs(base, len(rb), name, C.byref(p), buf, n, tot) != n:
        raise ValueError("bsc_meth_cpg_format_recs: the length changed between two calls")
    return (buf.raw[:n], [int(v) for v in tot]) if totals else buf.raw[:n]


REGION = np.dtype([("start", "<u4"), ("end", "<u4")])  # bsc_meth_region


def _regions(regions):
    r = np.asarray(regions)
    if not r.dtype.names:
        r = r.reshape(-1, 2)
        if len(r) and (r.min() < 0 or r.max() > 0xFFFFFFFF):
            raise ValueError("a region's coordinates are 0 .. 2^32 - 1")
        r = np.ascontiguousarray(r, dtype=np.uint32).view(REGION).reshape(-1)
    return np.ascontiguousarray(r, dtype=REGION)


def parse_regions(data):
    """BED text (bytes) -> {contig: (regions, names)}, the contigs in order of first appearance, each contig's regions (dtype REGION)
    stably sorted by (start, end), names = their fourth column or "." (bsc_meth_regions_parse_bed, csrc/methregions.c; include/bscall_amd.h
    says which lines are taken, skipped and refused).  ValueError with the line's number for a malformed line."""
    L = _lib.load()
    out = C.POINTER(_lib.MethBed)()
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))  # exactly the text: no terminator is promised
    if L.bsc_meth_regions_parse_bed(C.cast(buf, C.c_void_p) if len(data) else None, len(data), C.byref(out)) != 0:
        raise ValueError(L.bsc_last_error().decode(errors="replace"))
    try:
        b = out.contents
        res = {}
        for c in range(b.n_contigs):
            lo, hi = int(b.first[c]), int(b.first[c + 1])
            regs = np.zeros(hi - lo, dtype=REGION)
            if hi > lo:
                C.memmove(regs.ctypes.data, b.regions + 8 * lo, 8 * (hi - lo))
            res[b.contigs[c].decode()] = (regs, [b.names[k].decode() for k in range(lo, hi)])
        return res
    finally:
        L.bsc_meth_bed_free(out)


def read_regions(path):
    """A BED file of regions, plain or gzip, as parse_regions returns it."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    return parse_regions(data)


def window_regions(length, window):
    """The fixed tiles of a contig of `length` bases: [k window, min((k + 1) window, length)) (bam2bcf --meth-window)."""
    if window < 1:
        raise ValueError("a window has at least one base")
    starts = np.arange(0, int(length), int(window), dtype=np.uint64)
    out = np.zeros(len(starts), dtype=REGION)
    out["start"] = starts
    out["end"] = np.minimum(starts + np.uint64(window), np.uint64(length))
    return out


def region_summary(lines_or_records, regions, p=None):
    """The accumulators uint64[n, 4] = per region {sites, A, B, P} of ONE contig's cytosines: lines_or_records is either rows of a
    per-cytosine table (dtype BED: read_bed / parse_bed; every row is a site at pos = start + 1, with its a, b and pct) or packed records
    (VCF_REC[]; the rule of include/bscall_amd.h under the parameters p, by bsc_meth_regions_sum_recs).  regions: (start, end) pairs or
    dtype REGION, in any order."""
    regs = _regions(regions)
    acc = np.zeros((len(regs), 4), dtype=np.uint64)
    x = np.asarray(lines_or_records)
    if x.dtype == BED:
        start = x["start"].astype(np.uint64)
        order = np.argsort(start, kind="stable")
        start = start[order]
        a, b = x["a"][order].astype(np.uint64), x["b"][order].astype(np.uint64)
        cov = a + b
        pct = (np.uint64(200) * a + cov) // np.maximum(np.uint64(2) * cov, np.uint64(1))
        cum = np.zeros((len(start) + 1, 4), dtype=np.uint64)
        cum[1:, 0] = np.arange(1, len(start) + 1)
        cum[1:, 1], cum[1:, 2], cum[1:, 3] = np.cumsum(a), np.cumsum(b), np.cumsum(pct)
        lo = np.searchsorted(start, regs["start"].astype(np.uint64), "left")
        hi = np.maximum(np.searchsorted(start, regs["end"].astype(np.uint64), "left"), lo)
        return cum[hi] - cum[lo]
    L = _lib.load()
    rb = np.ascontiguousarray(x).view(np.uint8).reshape(-1, 128)
    p = params() if p is None else p
    if L.bsc_meth_regions_sum_recs(rb.ctypes.data if len(rb) else None, len(rb), C.byref(p), regs.ctypes.data if len(regs) else None, len(regs),
                                   acc.ctypes.data if len(regs) else None) != 0:
        raise ValueError(L.bsc_last_error().decode(errors="replace"))
    return acc


def format_regions(contig, regions, names, acc):
    """The summary's lines (bytes) of one contig: ten columns per region — chrom start end name sites A+B A B level mean
    (bsc_meth_regions_format).  names: a string per region, or None for "."."""
    L = _lib.load()
    regs = _regions(regions)
    acc = np.ascontiguousarray(acc, dtype=np.uint64).reshape(-1, 4)
    if len(acc) != len(regs) or (names is not None and len(names) != len(regs)):
        raise ValueError("as many accumulators and names as regions")
    name = contig if isinstance(contig, (bytes, bytearray)) else str(contig).encode()
    nm = None
    if names is not None:
        nm = (C.c_char_p * max(len(regs), 1))(*[(s if isinstance(s, (bytes, bytearray)) else str(s).encode()) for s in names])
    rp, ap = (regs.ctypes.data, acc.ctypes.data) if len(regs) else (None, None)
    n = L.bsc_meth_regions_format(name, rp, nm, ap, len(regs), None, 0)
    if n < 0:
        raise ValueError("bsc_meth_regions_format: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    if L.bsc_meth_regions_format(name, rp, nm, ap, len(regs), buf, n) != n:
        raise ValueError("bsc_meth_regions_format: the length changed between two calls")
    return buf.raw[:n]


def parse_bed(data):
    rows = [ln.split(b"\t") for ln in data.split(b"\n") if ln]
    out = np.zeros(len(rows), dtype=BED)
    for i, f in enumerate(rows):
        if len(f) != 15:
            raise ValueError("line %d has %d columns, not 15" % (i + 1, len(f)))
        s = [v.decode() for v in f]
        out[i] = (s[0], int(s[1]), int(s[2]), s[3], int(s[4]), s[5], int(s[6]), int(s[7]), s[8], int(s[9]), int(s[10]), int(s[11]), int(s[12]), int(s[13]), s[14])
    return out


def read_bed(path):
    """A table file, plain or BGZF, as a structured array (dtype BED)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    return parse_bed(data)


# ---- region queries through the table's index: what bam2bcf --meth-index / bsc_tbx_* / pipeline.run(meth_index=...) write beside a BGZF table --
def _inflate_all(blob):
    import zlib

    out, at = [], 0
    while at < len(blob):
        bsize = int.from_bytes(blob[at + 16 : at + 18], "little") + 1
        out.append(zlib.decompress(blob[at + 18 : at + bsize - 8], -15))
        at += bsize
    return b"".join(out)


def read_index(path):
    """A .tbi or .csi file of a table parsed: {"kind": "tbi" | "csi", "min_shift", "depth", "names", "refs": [{"bins": {bin: [(vbeg, vend)]},
    "loff": {bin: loffset} (csi), "ioff": [..] (tbi), "n_lines"}]} — the pseudo-bin is taken out of "bins" and gives "n_lines"."""
    import struct

    with open(path, "rb") as f:
        b = _inflate_all(f.read())
    kind = {b"TBI\x01": "tbi", b"CSI\x01": "csi"}.get(b[:4])
    if kind is None:
        raise ValueError("%s: neither a tabix nor a CSI index" % path)
    if kind == "tbi":
        n_ref, fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<8i", b, 4)
        min_shift, depth, at = 14, 5, 36
    else:
        min_shift, depth, l_aux = struct.unpack_from("<3i", b, 4)
        if l_aux < 28:
            raise ValueError("%s: a CSI index without the tabix block is not a table's" % path)
        fmt, cs, cb, ce, meta, skip, l_nm = struct.unpack_from("<7i", b, 16)
        (n_ref,) = struct.unpack_from("<i", b, 16 + l_aux)
        at = 44
    if (fmt, cs, cb, ce) != (0x10000, 1, 2, 3):
        raise ValueError("%s: not the index of a BED table (format %#x, columns %d %d %d)" % (path, fmt, cs, cb, ce))
    names = [n.decode() for n in b[at : at + l_nm].split(b"\0")[:-1]]
    at += l_nm + (4 if kind == "csi" else 0)
    pseudo = ((1 << (3 * (depth + 1))) - 1) // 7 + 1
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", b, at)
        at += 4
        r = {"bins": {}, "loff": {}, "ioff": [], "n_lines": 0}
        for _ in range(n_bin):
            (k,) = struct.unpack_from("<I", b, at)
            at += 4
            if kind == "csi":
                (r["loff"][k],) = struct.unpack_from("<Q", b, at)
                at += 8
            (n_chunk,) = struct.unpack_from("<i", b, at)
            at += 4
            ch = [struct.unpack_from("<QQ", b, at + 16 * i) for i in range(n_chunk)]
            at += 16 * n_chunk
            if k == pseudo:
                r["n_lines"] = ch[1][0]
                r["loff"].pop(k, None)
            else:
                r["bins"][k] = ch
        if kind == "tbi":
            (n_intv,) = struct.unpack_from("<i", b, at)
            r["ioff"] = list(struct.unpack_from("<%dQ" % n_intv, b, at + 4))
            at += 4 + 8 * n_intv
        refs.append(r)
    if at + 8 != len(b):
        raise ValueError("%s: %d bytes behind the last contig, not n_no_coor alone" % (path, len(b) - at))
    return {"kind": kind, "min_shift": min_shift, "depth": depth, "names": names, "refs": refs}


def reg2bins(beg, end, min_shift=14, depth=5):
    """The bins of every level that overlap [beg, end) (0-based, half open), ascending."""
    if end <= beg:
        return []
    out, first = [], 0
    for level in range(depth + 1):
        s = min_shift + 3 * (depth - level)
        out += range(first + (beg >> s), first + ((end - 1) >> s) + 1)
        first += 1 << (3 * level)
    return out


def index_chunks(index, tid, beg, end):
    """The chunks [(vbeg, vend)] a query of [beg, end) on contig number tid has to read, sorted, overlapping and touching ones joined; what
    ends at or before the linear index's offset of beg's window (tbi) cannot hold a line of the range and is left out."""
    r = index["refs"][tid]
    lo = 0
    if index["kind"] == "tbi":
        w = beg >> index["min_shift"]
        if w >= len(r["ioff"]):
            return []
        lo = r["ioff"][w]
    ch = sorted(c for k in reg2bins(beg, end, index["min_shift"], index["depth"]) for c in r["bins"].get(k, ()) if c[1] > lo)
    out = []
    for a, b in ch:
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(c) for c in out]


def _read_chunk(f, vbeg, vend):
    import zlib

    out, at = [], vbeg >> 16
    while at < (vend >> 16) or (at == (vend >> 16) and (vend & 0xFFFF)):
        f.seek(at)
        head = f.read(18)
        bsize = int.from_bytes(head[16:18], "little") + 1
        data = zlib.decompress(f.read(bsize - 18)[:-8], -15)
        a = (vbeg & 0xFFFF) if at == (vbeg >> 16) else 0
        out.append(data[a : (vend & 0xFFFF)] if at == (vend >> 16) else data[a:])
        at += bsize
    return b"".join(out)


def fetch(table_path, contig, beg, end, index_path=None):
    """The lines (bytes, each with its newline) of `contig` (name or number) that overlap [beg, end) (0-based, half open), in file order, read
    from the BGZF table through its index (default: table_path + ".tbi", else + ".csi"): only the chunks the index names are inflated."""
    import os

    if index_path is None:
        index_path = table_path + ".tbi" if os.path.exists(table_path + ".tbi") else table_path + ".csi"
    ix = index_path if isinstance(index_path, dict) else read_index(index_path)
    if isinstance(contig, str):
        if contig not in ix["names"]:
            return []
        tid = ix["names"].index(contig)
    else:
        tid = int(contig)
    if not 0 <= tid < len(ix["refs"]) or end <= beg:
        return []
    name, out = ix["names"][tid].encode(), []
    with open(table_path, "rb") as f:
        for vbeg, vend in index_chunks(ix, tid, int(beg), int(end)):
            for ln in _read_chunk(f, vbeg, vend).split(b"\n")[:-1]:
                c = ln.split(b"\t", 3)
                if c[0] == name and int(c[1]) < end and int(c[2]) > beg:
                    out.append(ln + b"\n")
    return out
