"""The epiallele table in Python: the rule of include/bscall_amd.h (COUNTS, SITE, BYTE, STATE of the read-level CpG table; WINDOW, PATTERN,
RECORD, TOTALS, LINE) on numpy arrays, written from the rule and calling nothing of the library — the third form beside the kernels
(csrc/epidev.hip) and the host form (csrc/epi.c), for tests and for users who hold templates in numpy.  Also the reader of the table and
the two statistics a reader derives from a window's sixteen counts: they are the only floats of the feature, and host Python only."""

import math

import numpy as np

from .abi import TEMPLATE

K = 4
WINDOW = np.dtype([("pos", "<u4"), ("span", "<u4"), ("c", "<u4", (16,))])
N_TOTALS = 8
TOTAL_NAMES = ("windows", "observations", "templates", "methylated", "templates_k4", "zero5", "zero6", "zero7")
COLUMNS = ("chrom", "start", "end", "n", "k") + tuple("c%d" % i for i in range(16))
NONE, M, U = 0, 1, 2


def _params(params):
    p = {"min_cov": 10, "reserved": 0}
    if params is None:
        return p
    if isinstance(params, dict):
        unknown = set(params) - set(p)
        if unknown:
            raise ValueError("unknown epiallele parameter(s): %s" % ", ".join(sorted(unknown)))
        p.update(params)
    else:  # a _lib.EpiParams
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


def _state(t, seq, x, y, min_qual, p):
    """STATE(t, s) for the site at p."""
    bs = int(t["bs_strand"])
    if bs == 1:
        b = _byte(t, seq, x, y, min_qual, p)
        return NONE if b is None else {1: M, 3: U}.get(b & 3, NONE)
    if bs == 2:
        b = _byte(t, seq, x, y, min_qual, p + 1)
        return NONE if b is None else {2: M, 0: U}.get(b & 3, NONE)
    return NONE


def windows(tpl, seq, x, y, ref, min_qual, params=None):
    """The block's records (a WINDOW array, one per window in position order) and the eight totals."""
    _params(params)
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    seq = np.asarray(seq, dtype=np.uint8)
    x, y, min_qual = int(x), int(y), int(min_qual)
    sp = site_positions(x, y, ref)
    spa = np.asarray(sp, dtype=np.int64)
    nw = max(len(sp) - (K - 1), 0)
    counts = np.zeros((nw, 16), np.int64)
    n_gave = n_bits = n_k4 = 0
    for t in tpl:
        ends = [int(t["pos"][k]) + int(t["len"][k]) for k in range(2) if int(t["len"][k])]
        if not ends or int(t["bs_strand"]) not in (1, 2):
            continue
        lo = min(int(t["pos"][k]) for k in range(2) if int(t["len"][k]))
        hi = max(ends)
        k0 = int(np.searchsorted(spa, lo - 1))  # no site in front of lo - 1 or behind hi - 1 has a byte
        k1 = int(np.searchsorted(spa, hi))
        st = [_state(t, seq, x, y, min_qual, p) for p in sp[k0:k1]]
        n_k4 += sum(s != NONE for s in st) >= K
        gave = False
        for i in range(len(st) - K + 1):
            w = st[i : i + K]
            if NONE in w:
                continue
            code = sum((w[j] == M) << j for j in range(K))
            counts[k0 + i, code] += 1
            n_bits += bin(code).count("1")
            gave = True
        n_gave += gave
    if counts.size and counts.max() > 0xFFFFFFFF:
        raise OverflowError("a counter exceeds 32 bits")
    recs = np.zeros(nw, WINDOW)
    for i in range(nw):
        recs[i]["pos"] = sp[i]
        recs[i]["span"] = sp[i + K - 1] - sp[i]
    recs["c"] = counts
    return recs, (nw, int(counts.sum()), n_gave, n_bits, n_k4, 0, 0, 0)


def check_contig(contig):
    c = contig.encode() if isinstance(contig, str) else bytes(contig)
    if not 1 <= len(c) <= 255 or b"\t" in c or b"\n" in c or b"\0" in c:
        raise ValueError("the contig's name must be 1 .. 255 bytes without tab or newline")
    return c


def format(contig, recs, params=None):  # noqa: A001 (the twin of cpgreads.format)
    """LINE: (the table's bytes, its lines) for a WINDOW array."""
    p = _params(params)
    c = check_contig(contig)
    need = max(1, int(p["min_cov"]))
    out = []
    for r in np.asarray(recs, dtype=WINDOW):
        cs = [int(v) for v in r["c"]]
        n = sum(cs)
        if n < need:
            continue
        cols = [int(r["pos"]) - 1, int(r["pos"]) + int(r["span"]) + 1, n, sum(v > 0 for v in cs)] + cs
        out.append(c + b"\t" + b"\t".join(b"%d" % v for v in cols) + b"\n")
    return b"".join(out), len(out)


def read_table(data):
    """The table's lines back: (contig names as a list of bytes, a WINDOW array with pos = start + 1 and span = end - start - 2)."""
    names, rows = [], []
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        f = line.split(b"\t")
        if len(f) != 21:
            raise ValueError("a line of %d columns, not 21" % len(f))
        v = [int(s) for s in f[1:]]
        cs = v[4:]
        if v[2] != sum(cs) or v[3] != sum(c > 0 for c in cs):
            raise ValueError("n or k does not fit the sixteen counts")
        if v[1] < v[0] + 2 + (K - 1) * 2:
            raise ValueError("end lies in front of the fourth CpG")
        names.append(f[0])
        rows.append((v[0] + 1, v[1] - v[0] - 2, cs))
    return names, np.array(rows, dtype=WINDOW) if rows else np.zeros(0, WINDOW)


def epipolymorphism(c):
    """1 - sum c^2 / n^2 of a window's sixteen counts (Landan et al.); nan for an empty window."""
    c = [int(v) for v in c]
    n = sum(c)
    return 1.0 - sum(v * v for v in c) / (n * n) if n else float("nan")


def entropy(c):
    """- sum (c / n) log2 (c / n) of a window's sixteen counts, in bits (0 .. 4; Xie et al. divide by 4); nan for an empty window."""
    c = [int(v) for v in c]
    n = sum(c)
    if not n:
        return float("nan")
    return -sum(v / n * math.log2(v / n) for v in c if v)
