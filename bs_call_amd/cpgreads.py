"""The read-level CpG concordance table in Python: the rule of include/bscall_amd.h (COUNTS, SITE, BYTE, STATE, RECORD, TOTALS, LINE) as numpy
loops, written from the rule — the third form beside the kernels (csrc/cpgreadsdev.hip) and the host form (csrc/cpgreads.c), for tests and for
users who hold templates in numpy.  A template's bytes are laid over the block position by position (BYTE), the states are read off that
row at the sites, and the counters are added up site by site."""

import numpy as np

from .abi import TEMPLATE

SITE = np.dtype([("pos", "<u4"), ("dist", "<u4"), ("m", "<u4"), ("u", "<u4"), ("e", "<u4"), ("d", "<u4"), ("mm", "<u4"), ("mu", "<u4"),
                 ("um", "<u4"), ("uu", "<u4")])
N_TOTALS = 8
TOTAL_NAMES = ("sites", "m", "u", "pairs", "templates", "eligible", "discordant", "zero")
COLUMNS = ("chrom", "start", "end", "m", "u", "e", "d", "dist", "mm", "mu", "um", "uu")
NONE, M, U = 0, 1, 2


def _params(params):
    p = {"min_sites": 4, "min_cov": 1}
    if params is None:
        return p
    if isinstance(params, dict):
        unknown = set(params) - set(p)
        if unknown:
            raise ValueError("unknown cpg-reads parameter(s): %s" % ", ".join(sorted(unknown)))
        p.update(params)
    else:  # a _lib.CpgReadsParams
        for k in p:
            p[k] = getattr(params, k)
    if int(p["min_sites"]) == 0:
        raise ValueError("min_sites must not be 0")
    return p


def site_positions(x, y, ref):
    """SITE: the positions p of x .. y with ref(p) == 2 and ref(p + 1) == 3; ref holds the codes of x .. y + 2 (y + 1 at least)."""
    ref = np.asarray(ref, dtype=np.uint8)
    n = int(y) - int(x) + 1
    return (np.flatnonzero((ref[:n] == 2) & (ref[1 : n + 1] == 3)) + int(x)).astype(np.int64)


def template_bytes(t, seq, x, y, min_qual):
    """BYTE(t, q) for every q of the template's span within x .. y: (first position, int16 array; -1 = no byte), and how many positions
    hold a counting byte of BOTH reads."""
    seq = np.asarray(seq, dtype=np.uint8)
    spans = []
    for k in range(2):
        ln, pos, off = int(t["len"][k]), int(t["pos"][k]), int(t["off"][k])
        if ln == 0 or off + ln > len(seq):
            continue
        spans.append((pos, seq[off : off + ln]))
    if not spans:
        return int(x), np.zeros(0, np.int16), 0
    lo = min(p for p, _ in spans)
    hi = max(p + len(b) for p, b in spans)
    row = np.full(hi - lo, -1, np.int16)
    both = np.zeros(hi - lo, np.int8)
    for pos, b in reversed(spans):  # read 0 last: its counting bytes win
        q = b >> 2
        ok = (q >= int(min_qual)) & (q < 63)
        idx = np.flatnonzero(ok) + (pos - lo)
        row[idx] = b[ok]
        both[idx] += 1
    g = np.arange(lo, hi)
    out = (g < int(x)) | (g > int(y))
    row[out] = -1
    both[out] = 0
    return lo, row, int((both == 2).sum())


def double_covered(tpl, seq, x, y, min_qual):
    """How many templates have two counting bytes at one position of x .. y (the mates overlap there and both bytes pass)."""
    return sum(1 for t in np.asarray(tpl, dtype=TEMPLATE) if template_bytes(t, seq, x, y, min_qual)[2] > 0)


def sites(tpl, seq, x, y, ref, min_qual, params=None):
    """The block's records (a SITE array, one per site in position order) and the eight totals."""
    p = _params(params)
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    sp = site_positions(x, y, ref)
    recs = np.zeros(len(sp), SITE)
    recs["pos"] = sp
    if len(sp) > 1:
        recs["dist"][:-1] = np.diff(sp)
    cnt = {f: np.zeros(len(sp), np.int64) for f in ("m", "u", "e", "d", "mm", "mu", "um", "uu")}
    n_any = n_elig = n_disc = 0
    for t in tpl:
        bs = int(t["bs_strand"])
        if bs not in (1, 2):
            continue
        lo, row, _ = template_bytes(t, seq, x, y, min_qual)
        if not len(row):
            continue
        shift = 0 if bs == 1 else 1
        k0 = int(np.searchsorted(sp, lo - shift))
        k1 = int(np.searchsorted(sp, lo + len(row) - shift))
        if k1 <= k0:
            continue
        b = row[sp[k0:k1] + shift - lo]
        base = b & 3
        st = np.zeros(k1 - k0, np.int8)
        if bs == 1:
            st[(b >= 0) & (base == 1)] = M
            st[(b >= 0) & (base == 3)] = U
        else:
            st[(b >= 0) & (base == 2)] = M
            st[(b >= 0) & (base == 0)] = U
        kt = int((st != NONE).sum())
        if not kt:
            continue
        elig = kt >= int(p["min_sites"])
        disc = elig and bool((st == M).any()) and bool((st == U).any())
        n_any += 1
        n_elig += elig
        n_disc += disc
        k = np.arange(k0, k1)
        cnt["m"][k[st == M]] += 1
        cnt["u"][k[st == U]] += 1
        if elig:
            cnt["e"][k[st != NONE]] += 1
        if disc:
            cnt["d"][k[st != NONE]] += 1
        a, nx = st[:-1], st[1:]  # site k and its NEXT, both inside the visited range (a NEXT outside it has no state)
        for name, sa, sb in (("mm", M, M), ("mu", M, U), ("um", U, M), ("uu", U, U)):
            cnt[name][k[:-1][(a == sa) & (nx == sb)]] += 1
    for f, v in cnt.items():
        if len(v) and v.max() > 0xFFFFFFFF:
            raise OverflowError("a counter exceeds 32 bits")
        recs[f] = v
    pairs = sum(int(cnt[f].sum()) for f in ("mm", "mu", "um", "uu"))
    totals = (len(sp), int(cnt["m"].sum()), int(cnt["u"].sum()), pairs, n_any, n_elig, n_disc, 0)
    return recs, totals


def check_contig(contig):
    c = contig.encode() if isinstance(contig, str) else bytes(contig)
    if not 1 <= len(c) <= 255 or b"\t" in c or b"\n" in c or b"\0" in c:
        raise ValueError("the contig's name must be 1 .. 255 bytes without tab or newline")
    return c


def format(contig, recs, params=None):  # noqa: A001 (the issue's name)
    """LINE: (the table's bytes, its lines) for a SITE array."""
    p = _params(params)
    c = check_contig(contig)
    need = max(1, int(p["min_cov"]))
    out = []
    for r in np.asarray(recs, dtype=SITE):
        if int(r["m"]) + int(r["u"]) < need:
            continue
        cols = [int(r["pos"]) - 1, int(r["pos"]) + 1] + [int(r[f]) for f in ("m", "u", "e", "d", "dist", "mm", "mu", "um", "uu")]
        out.append(c + b"\t" + b"\t".join(b"%d" % v for v in cols) + b"\n")
    return b"".join(out), len(out)


def read_table(data):
    """The table's lines back: (contig names as a list of bytes, a SITE array with pos = start + 1)."""
    names, rows = [], []
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        f = line.split(b"\t")
        if len(f) != 12:
            raise ValueError("a line of %d columns, not 12" % len(f))
        v = [int(s) for s in f[1:]]
        if v[1] != v[0] + 2:
            raise ValueError("end is not start + 2")
        names.append(f[0])
        rows.append((v[0] + 1, v[6], v[2], v[3], v[4], v[5], v[7], v[8], v[9], v[10]))
    return names, np.array(rows, dtype=SITE) if rows else np.zeros(0, SITE)
