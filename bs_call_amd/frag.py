"""The per-region fragment methylation summary in Python: the rule of include/bscall_amd.h (COUNTS, SITE, BYTE, STATE of the read-level CpG
table, REGION of the region summary; IN, the classes, SUMS, TOTALS, LINE) on numpy arrays, written from the rule and calling nothing of the
library — the third form beside the kernel (csrc/fragdev.hip) and the host form (csrc/frag.c), for tests and for users who hold templates in
numpy.  Also the table's writer and reader, the shares a reader derives from a row (the only floats of the feature, host Python only) and the
same sums made from a PAT table."""

import numpy as np

from .abi import TEMPLATE

N_SUMS = 8
N_TOTALS = 8
SUM_NAMES = ("frags", "U", "X", "M", "K", "Mm", "disc", "short")
TOTAL_NAMES = ("templates", "frags", "U", "X", "M", "K", "Mm", "disc")
COLUMNS = ("chrom", "start", "end", "name") + SUM_NAMES
NONE, M, U = 0, 1, 2
FRAGS, CU, CX, CM, K, MM, DISC, SHORT = range(8)


def _params(params):
    p = {"min_sites": 3, "u_max_pct": 25, "m_min_pct": 75, "reserved": 0}
    if params is None:
        return p
    if isinstance(params, dict):
        unknown = set(params) - set(p)
        if unknown:
            raise ValueError("unknown fragment parameter(s): %s" % ", ".join(sorted(unknown)))
        p.update(params)
    else:  # a _lib.FragParams
        for k in p:
            p[k] = getattr(params, k)
    p = {k: int(v) for k, v in p.items()}
    if p["min_sites"] == 0:
        raise ValueError("min_sites must be 1 at least")
    if p["u_max_pct"] > 100 or p["m_min_pct"] > 100:
        raise ValueError("a percentage above 100")
    if p["u_max_pct"] >= p["m_min_pct"]:
        raise ValueError("u_max_pct must be below m_min_pct")
    if p["reserved"] != 0:
        raise ValueError("reserved must be 0")
    return p


def _region_pairs(regions):
    r = np.asarray(regions)
    if r.dtype.names:
        return [(int(a), int(b)) for a, b in zip(r["start"], r["end"])]
    return [(int(a), int(b)) for a, b in r.reshape(-1, 2)]


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


def classify(k, m, p):
    """The class column (CU, CX or CM) of a fragment with k states, m of them M — integers alone."""
    if 100 * m <= p["u_max_pct"] * k:
        return CU
    if 100 * m >= p["m_min_pct"] * k:
        return CM
    return CX


def _add(acc, tot, r, k, m, p, count=1):
    if k == 0:
        return
    if k < p["min_sites"]:
        acc[r][SHORT] += count
        return
    cls = classify(k, m, p)
    for row, base in ((acc[r], 0), (tot, 1)):
        row[base + FRAGS] += count
        row[base + cls] += count
        row[base + K] += count * k
        row[base + MM] += count * m
        row[base + DISC] += count * (0 < m < k)


def region_frags(block, regions, params=None):
    """The rule on one block — a dict with tpl, seq, x, y, ref and min_qual, as the tests' case files make them — and (start, end) regions
    in any order: (uint64[n, 8] accumulators {frags, U, X, M, K, Mm, disc, short}, the call's eight totals)."""
    p = _params(params)
    regs = _region_pairs(regions)
    tpl = np.ascontiguousarray(block["tpl"], dtype=TEMPLATE)
    seq = np.asarray(block["seq"], dtype=np.uint8)
    x, y, min_qual = int(block["x"]), int(block["y"]), int(block["min_qual"])
    sp = site_positions(x, y, block["ref"])
    spa = np.asarray(sp, dtype=np.int64)
    acc = [[0] * N_SUMS for _ in regs]
    tot = [0] * N_TOTALS
    starts = np.asarray([a for a, _ in regs], dtype=np.int64)
    stops = np.asarray([b for _, b in regs], dtype=np.int64)
    for t in tpl:
        ends = [int(t["pos"][k]) + int(t["len"][k]) for k in range(2) if int(t["len"][k])]
        if not ends or int(t["bs_strand"]) not in (1, 2):
            continue
        lo = min(int(t["pos"][k]) for k in range(2) if int(t["len"][k]))
        k0 = int(np.searchsorted(spa, lo - 1))  # no site in front of lo - 1 or behind max(ends) - 1 has a byte
        k1 = int(np.searchsorted(spa, max(ends)))
        st = [(q, _state(t, seq, x, y, min_qual, q)) for q in sp[k0:k1]]
        st = [(q, s) for q, s in st if s != NONE]
        if not st:
            continue
        tot[0] += 1
        first, last = st[0][0], st[-1][0]
        for r in np.nonzero((starts < last) & (stops >= first))[0]:  # IN needs start < p <= end for one p of first .. last
            a, b = regs[r]
            inside = [s for q, s in st if a < q <= b]
            _add(acc, tot, r, len(inside), sum(s == M for s in inside), p)
    return np.array(acc, dtype=np.uint64).reshape(len(regs), N_SUMS), tuple(tot)


def from_pat(lines, site_positions, regions, params=None):  # noqa: A002 (the argument names the issue's)
    """The same accumulators from ONE contig's PAT table: lines as pat.read_pat gives them (chrom, index, pattern, count), site_positions
    the contig's CpG positions in ascending order (index i is site_positions[i - 1]).  A line is a template — or count identical ones —, so
    the sums are the rule's wherever no template covers more than 64 sites (the PAT table cuts a longer one into several lines) and the PAT
    table was written with min_sites 1.  Returns (uint64[n, 8], totals[8])."""
    p = _params(params)
    regs = _region_pairs(regions)
    sp = np.asarray(site_positions, dtype=np.int64)
    acc = [[0] * N_SUMS for _ in regs]
    tot = [0] * N_TOTALS
    starts = np.asarray([a for a, _ in regs], dtype=np.int64)
    stops = np.asarray([b for _, b in regs], dtype=np.int64)
    for _, index, pattern, count in lines:
        st = [(int(sp[index - 1 + j]), M if c == "C" else U) for j, c in enumerate(pattern) if c != "."]
        if not st:
            continue
        tot[0] += count
        first, last = st[0][0], st[-1][0]
        for r in np.nonzero((starts < last) & (stops >= first))[0]:
            a, b = regs[r]
            inside = [s for q, s in st if a < q <= b]
            _add(acc, tot, r, len(inside), sum(s == M for s in inside), p, count)
    return np.array(acc, dtype=np.uint64).reshape(len(regs), N_SUMS), tuple(tot)


def check_label(label):
    c = label.encode() if isinstance(label, str) else bytes(label)
    if not 1 <= len(c) <= 255 or b"\t" in c or b"\n" in c or b"\0" in c:
        raise ValueError("a contig's or a region's name must be 1 .. 255 bytes without tab or newline")
    return c


def format_regions(contig, regions, names, acc):
    """LINE: the table's bytes for one contig's regions (in the given order), their names (None, or None entries: ".") and accumulators."""
    c = check_label(contig)
    regs = _region_pairs(regions)
    acc = np.asarray(acc, dtype=np.uint64).reshape(-1, N_SUMS)
    if len(acc) != len(regs) or (names is not None and len(names) != len(regs)):
        raise ValueError("as many accumulators and names as regions")
    out = []
    for i, (a, b) in enumerate(regs):
        nm = check_label("." if names is None or names[i] is None else names[i])
        out.append(b"%s\t%d\t%d\t%s\t" % (c, a, b, nm) + b"\t".join(b"%d" % int(v) for v in acc[i]) + b"\n")
    return b"".join(out)


ROW = np.dtype([("chrom", "O"), ("start", "<u4"), ("end", "<u4"), ("name", "O")] + [(n, "<u8") for n in SUM_NAMES])


def read_table(data):
    """The table's lines back — bytes, or the path of a file: a ROW array (chrom and name as bytes)."""
    if isinstance(data, str):
        with open(data, "rb") as f:
            data = f.read()
    rows = []
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        f = line.split(b"\t")
        if len(f) != 12:
            raise ValueError("a line of %d columns, not 12" % len(f))
        v = [int(s) for s in f[4:]]
        if v[FRAGS] != v[CU] + v[CX] + v[CM] or v[MM] > v[K] or v[DISC] > v[FRAGS]:
            raise ValueError("the classes do not add up to the fragments, or Mm > K, or disc > frags")
        rows.append((f[0], int(f[1]), int(f[2]), f[3]) + tuple(v))
    out = np.zeros(len(rows), ROW)
    for o, r in zip(out, rows):
        for n, v in zip(ROW.names, r):
            o[n] = v
    return out


def fractions(row):
    """What a reader derives from a row (a ROW entry, or the eight sums): {"U", "X", "M"} the classes' shares of the fragments, "disc" =
    disc / frags, "level" = Mm / K, the mean level of the fragments' calls.  nan where the denominator is 0."""
    v = [int(row[n]) for n in SUM_NAMES] if getattr(row, "dtype", None) is not None and row.dtype.names else [int(x) for x in row]
    nan = float("nan")
    fr, kk = v[FRAGS], v[K]
    return {"U": v[CU] / fr if fr else nan, "X": v[CX] / fr if fr else nan, "M": v[CM] / fr if fr else nan, "disc": v[DISC] / fr if fr else nan,
            "level": v[MM] / kk if kk else nan}
