"""The per-read CpG pattern table (PAT) in Python: the rule of include/bscall_amd.h (COUNTS, SITE, BYTE, STATE of the read-level CpG table;
ORDINAL, PATTERN, PIECES, RECORD, TOTALS, LINE) with strings, `sorted` and a counter, written from the rule and calling nothing of the
library — the third form beside the kernels (csrc/patdev.hip) and the host form (csrc/pat.c), for tests and for users who hold templates in
numpy.  Also the reader of the table, the per-CpG counts a table implies, and the conversion between this table's per-contig indices and the
genome-wide ones of wgbstools.  The bytes are wgbstools-unpinned: no copy of that tool is at hand, the format is written from its description."""

import collections
import gzip

import numpy as np

from .abi import TEMPLATE

MAX_SITES = 64
REC = np.dtype([("idx", "<u4"), ("count", "<u4"), ("hi", "<u8"), ("lo", "<u8")])
N_TOTALS = 8
TOTAL_NAMES = ("records", "pieces", "templates", "c", "t", "dots", "templates_cut", "sites")
COLUMNS = ("chrom", "index", "pattern", "count")


def _params(params):
    p = {"min_sites": 1, "reserved": 0}
    if params is None:
        return p
    if isinstance(params, dict):
        unknown = set(params) - set(p)
        if unknown:
            raise ValueError("unknown PAT parameter(s): %s" % ", ".join(sorted(unknown)))
        p.update(params)
    else:  # a _lib.PatParams
        for k in p:
            p[k] = getattr(params, k)
    if int(p["reserved"]) != 0:
        raise ValueError("reserved must be 0")
    return p


def site_positions(x, y, ref):
    """SITE: the positions p of x .. y with ref(p) == 2 and ref(p + 1) == 3; ref holds the codes of x .. y + 2 (y + 1 at least)."""
    ref = np.asarray(ref, dtype=np.uint8)
    return [int(x) + i for i in range(int(y) - int(x) + 1) if ref[i] == 2 and ref[i + 1] == 3]


def _byte(t, seq, x, y, min_qual, q):
    """BYTE(t, q), or None."""
    if q < x or q > y:
        return None
    for k in range(2):
        ln, pos, off = int(t["len"][k]), int(t["pos"][k]), int(t["off"][k])
        if ln == 0 or off + ln > len(seq):
            continue
        if pos <= q < pos + ln:
            b = int(seq[off + q - pos])
            if min_qual <= (b >> 2) < 63:
                return b
    return None


def _char(t, seq, x, y, min_qual, p):
    """STATE(t, s) for the site at p, as the pattern's character."""
    bs = int(t["bs_strand"])
    if bs == 1:
        b = _byte(t, seq, x, y, min_qual, p)
        return "." if b is None else {1: "C", 3: "T"}.get(b & 3, ".")
    if bs == 2:
        b = _byte(t, seq, x, y, min_qual, p + 1)
        return "." if b is None else {2: "C", 0: "T"}.get(b & 3, ".")
    return "."


def patterns(tpl, seq, x, y, ref, min_qual, params=None):
    """The block's records as a sorted list of (idx, pattern, count) and the eight totals."""
    need = max(1, int(_params(params)["min_sites"]))
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    seq = np.asarray(seq, dtype=np.uint8)
    x, y, min_qual = int(x), int(y), int(min_qual)
    sp = site_positions(x, y, ref)
    spa = np.asarray(sp, dtype=np.int64)
    seen = collections.Counter()
    n_tpl = n_cut = 0
    for t in tpl:
        ends = [int(t["pos"][k]) + int(t["len"][k]) for k in range(2) if int(t["len"][k])]
        if not ends or int(t["bs_strand"]) not in (1, 2):
            continue
        lo = min(int(t["pos"][k]) for k in range(2) if int(t["len"][k]))
        k0 = int(np.searchsorted(spa, lo - 1))  # no site in front of lo - 1 or behind max(ends) - 1 has a byte
        k1 = int(np.searchsorted(spa, max(ends)))
        s = "".join(_char(t, seq, x, y, min_qual, p) for p in sp[k0:k1])
        if len(s) - s.count(".") < need:
            continue
        f = k0 + len(s) - len(s.lstrip("."))
        s = s.strip(".")
        n_tpl += 1
        n_cut += len(s) > MAX_SITES
        for a in range(0, len(s), MAX_SITES):
            piece = s[a : a + MAX_SITES]
            body = piece.lstrip(".")
            if body:
                seen[(f + a + len(piece) - len(body), body.rstrip("."))] += 1
    recs = [(i, s, n) for (i, s), n in sorted(seen.items())]  # (a str compares as its ASCII bytes: '.' < 'C' < 'T', a prefix first)
    if any(n > 0xFFFFFFFF for _, _, n in recs):
        raise OverflowError("a count exceeds 32 bits")
    every = "".join(s * n for _, s, n in recs)
    return recs, (len(recs), sum(n for _, _, n in recs), n_tpl, every.count("C"), every.count("T"), every.count("."), n_cut, len(sp))


_CODE = {".": 1, "C": 2, "T": 3}


def pack(recs):
    """(idx, pattern, count) tuples -> a REC array (RECORD: site j in bits 127 - 2j, 126 - 2j of hi:lo)."""
    out = np.zeros(len(recs), REC)
    for o, (i, s, n) in zip(out, recs):
        v = 0
        for j, c in enumerate(s):
            v |= _CODE[c] << (126 - 2 * j)
        o["idx"], o["count"], o["hi"], o["lo"] = i, n, v >> 64, v & 0xFFFFFFFFFFFFFFFF
    return out


def unpack(recs):
    """A REC array -> (idx, pattern, count) tuples."""
    out = []
    for r in np.asarray(recs, dtype=REC):
        v = int(r["hi"]) << 64 | int(r["lo"])
        s = ""
        for j in range(MAX_SITES):
            c = (v >> (126 - 2 * j)) & 3
            if not c:
                break
            s += ".CT"[c - 1]
        out.append((int(r["idx"]), s, int(r["count"])))
    return out


def check_contig(contig):
    c = contig.encode() if isinstance(contig, str) else bytes(contig)
    if not 1 <= len(c) <= 255 or b"\t" in c or b"\n" in c or b"\0" in c:
        raise ValueError("the contig's name must be 1 .. 255 bytes without tab or newline")
    return c


def format(contig, index_base, recs, params=None):  # noqa: A001 (the twin of cpgreads.format)
    """LINE: (the table's bytes, its lines) for (idx, pattern, count) tuples or a REC array."""
    _params(params)
    c = check_contig(contig)
    if not 0 <= int(index_base) <= 1 << 63:
        raise ValueError("index_base above 2^63")
    if isinstance(recs, np.ndarray):
        recs = unpack(recs)
    out = [b"%s\t%d\t%s\t%d\n" % (c, int(index_base) + i + 1, s.encode(), n) for i, s, n in recs]
    return b"".join(out), len(out)


def read_pat(data):
    """A table's lines back — bytes, or the path of a plain or gzip / BGZF file: a list of (chrom as bytes, index, pattern, count)."""
    if isinstance(data, str):
        with open(data, "rb") as f:
            data = f.read()
        if data[:2] == b"\x1f\x8b":
            data = gzip.decompress(data)
    rows = []
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        f = line.split(b"\t")
        if len(f) != 4:
            raise ValueError("a line of %d columns, not 4" % len(f))
        s = f[2].decode()
        if not s or set(s) - set(".CT") or s[0] == "." or s[-1] == ".":
            raise ValueError("a pattern is C / T / . and neither starts nor ends with '.'")
        rows.append((f[0], int(f[1]), s, int(f[3])))
    return rows


def site_counts(lines):
    """The per-CpG counts a table implies: {(chrom, index): [m, u]} over (chrom, index, pattern, count) lines."""
    out = {}
    for chrom, index, s, n in lines:
        for j, c in enumerate(s):
            if c != ".":
                out.setdefault((chrom, index + j), [0, 0])[c == "T"] += n
    return out


def contig_offsets(fasta):
    """The CpGs in front of every contig of a FASTA file (plain or gzip), in file order: {name as bytes: offset}.  wgbstools counts CpGs
    genome-wide: its index of a CpG is this table's index + the contig's offset."""
    out, name, count, last = {}, None, 0, b""
    with open(fasta, "rb") as f:
        zipped = f.read(2) == b"\x1f\x8b"
    with (gzip.open if zipped else open)(fasta, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                name, last = line[1:].split()[0], b""
                out[name] = count
                continue
            s = last + line.strip().upper()
            count += s.count(b"CG")
            last = s[-1:]
    return out


def shift(lines, offset):
    """(chrom, index, pattern, count) lines with `offset` added to the index; offset: a number, or {chrom: offset} as contig_offsets gives."""
    return [(c, i + (offset[c] if isinstance(offset, dict) else int(offset)), s, n) for c, i, s, n in lines]
