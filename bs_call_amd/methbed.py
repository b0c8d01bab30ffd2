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
