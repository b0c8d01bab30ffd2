"""The allele-specific methylation table in Python: the rule of include/bscall_amd.h (SNP, ALLELE, WINDOW, RECORD, AQ, TOTALS, LINE on top of
COUNTS, SITE, BYTE and STATE of the read-level CpG table) as numpy loops, written from the rule — the third form beside the kernels
(csrc/asmdev.hip) and the host form (csrc/asm.c), for tests and for users who hold templates in numpy.

Fisher's p is not restated a third time here: pairs() takes it as a function `fisher(c, lfact) -> p` of a table c = [m1, u1, m2, u2] and the
ln k! table.  The test suite passes its pure-Python model of the reference's Fisher test.  The rule's clamp (a point term exp(arg) is 0.0 for
arg < -700) needs no place in such a function: an unclamped term is below 1e-304, the terms behind it on the same walk are smaller still, and
a sum they reach is either below 1e-100 with or without them (aq = 1000 both ways) or unchanged by them in its last bit."""

import math

import numpy as np

from .abi import TEMPLATE, VCF_CORE
from .cpgreads import M, U, check_contig, site_positions, template_bytes

PAIR = np.dtype([("snp_pos", "<u4"), ("cpg_pos", "<u4"), ("m1", "<u4"), ("u1", "<u4"), ("m2", "<u4"), ("u2", "<u4"), ("aq", "<u4"), ("info", "<u4")])
N_TOTALS = 8
TOTAL_NAMES = ("snps", "records", "observations", "allele1", "adds", "deep", "zero6", "zero7")
COLUMNS = ("chrom", "start", "end", "snp_pos", "gt", "m1", "u1", "m2", "u2", "aq", "dist")
GENOTYPES = ("AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT")
HET = (1, 2, 3, 5, 6, 8)
OVERLAPPED, DEEP = 1, 2
DEEP_ABOVE = 46340
LN10 = 2.30258509299404568402


def _params(params):
    p = {"min_phred": 20, "pass_only": 0, "max_dist": 500, "min_cov": 2}
    if params is None:
        return p
    if isinstance(params, dict):
        unknown = set(params) - set(p)
        if unknown:
            raise ValueError("unknown asm parameter(s): %s" % ", ".join(sorted(unknown)))
        p.update(params)
    else:  # a _lib.AsmParams
        for k in p:
            p[k] = getattr(params, k)
    if not 1 <= int(p["max_dist"]) <= 65535:
        raise ValueError("max_dist must be 1 .. 65535")
    return p


def lfact_table():
    """ln k! for k = 0 .. 255 by the statements the context fills its table with (bsc_get_tables returns the same numbers)."""
    lf = np.zeros(256, np.float64)
    acc = 0.0
    for i in range(2, 256):
        acc += math.log(float(i))
        lf[i] = acc
    return lf


def snp_positions(x, core, emit, params=None):
    """SNP: the positions of the block that are one, ascending."""
    p = _params(params)
    core = np.asarray(core, dtype=VCF_CORE)
    ok = (core["emit"] != 0) & np.isin(core["gt"], HET) & (core["phred"] >= int(p["min_phred"]))
    if emit is not None:
        ok &= np.asarray(emit, dtype=np.uint8) != 0
    if int(p["pass_only"]):
        ok &= core["flt"] == 0
    return np.flatnonzero(ok).astype(np.int64) + int(x)


def allele(bs, gt, base):
    """ALLELE from the template's strand, the genotype and the base (0 .. 3) of BYTE(t, h)."""
    if bs not in (1, 2) or (bs == 1 and gt == 6) or (bs == 2 and gt == 2):
        return 0
    letter = "ACGT"[base]
    stands_for = {letter}
    if bs == 1 and letter == "T":
        stands_for.add("C")
    if bs == 2 and letter == "A":
        stands_for.add("G")
    a1, a2 = GENOTYPES[gt]
    in1, in2 = a1 in stands_for, a2 in stands_for
    return 0 if in1 == in2 else (1 if in1 else 2)


def aq_of(c, lfact, fisher):
    z = fisher([int(v) for v in c], lfact)
    return int(-(math.log(z) / LN10) * 10.0 + 0.5) if z >= 1e-100 else 1000


def pairs(tpl, seq, x, y, ref, core, emit, min_qual, fisher, lfact=None, params=None, cap=None):
    """The block's records (a PAIR array, one per (SNP, window site)) and the eight totals.  fisher(c, lfact) -> Fisher's two-sided p of the
    table c.  cap: the room (DEEP, aq and totals[5] exist for the stored records alone); default: every record."""
    p = _params(params)
    x, y, W = int(x), int(y), int(p["max_dist"])
    lfact = lfact_table() if lfact is None else lfact
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    core = np.ascontiguousarray(core, dtype=VCF_CORE)
    sp = site_positions(x, y, ref)
    hs = snp_positions(x, core, emit, p)
    first = [int(np.searchsorted(sp, max(x, h - W))) for h in hs]
    n_of = [int(np.searchsorted(sp, min(y, h + W) + 1)) - f for h, f in zip(hs, first)]
    off = np.concatenate([[0], np.cumsum(n_of)]).astype(np.int64)
    total = int(off[-1])
    if total > 0xFFFFFFFF:
        raise OverflowError("more than 2^32 - 1 records")
    recs = np.zeros(total, PAIR)
    cnt = np.zeros((total, 4), np.int64)
    for j, h in enumerate(hs):
        k = slice(off[j], off[j + 1])
        s = sp[first[j] : first[j] + n_of[j]]
        recs["snp_pos"][k] = h
        recs["cpg_pos"][k] = s
        recs["info"][k] = int(core["gt"][h - x]) | (((s == h) | (s + 1 == h)).astype(np.uint32) * OVERLAPPED) << 8
    n_obs = n_a1 = 0
    for t in tpl:
        bs = int(t["bs_strand"])
        if bs not in (1, 2):
            continue
        lo, row, _ = template_bytes(t, seq, x, y, min_qual)
        if not len(row):
            continue
        shift = 0 if bs == 1 else 1
        for j in range(int(np.searchsorted(hs, lo)), int(np.searchsorted(hs, lo + len(row)))):
            h = int(hs[j])
            b = int(row[h - lo])
            if b < 0:
                continue
            al = allele(bs, int(core["gt"][h - x]), b & 3)
            if not al:
                continue
            n_obs += 1
            n_a1 += al == 1
            s = sp[first[j] : first[j] + n_of[j]]
            q = s + shift - lo  # where the site's byte lies in the row
            inside = (q >= 0) & (q < len(row)) & (s != h) & (s + 1 != h)
            bb = np.where(inside, row[np.clip(q, 0, len(row) - 1)], -1)
            base = bb & 3
            st = np.zeros(len(s), np.int8)
            st[(bb >= 0) & (base == (1 if bs == 1 else 2))] = M
            st[(bb >= 0) & (base == (3 if bs == 1 else 0))] = U
            k = np.arange(off[j], off[j + 1])
            cnt[k[st == M], 2 * (al - 1)] += 1
            cnt[k[st == U], 2 * (al - 1) + 1] += 1
    if total and cnt.max() > 0xFFFFFFFF:
        raise OverflowError("a counter exceeds 32 bits")
    for c, f in enumerate(("m1", "u1", "m2", "u2")):
        recs[f] = cnt[:, c]
    stored = total if cap is None else min(total, int(cap))
    n_deep = 0
    for k in range(stored):
        if (int(recs["info"][k]) >> 8) & OVERLAPPED:
            continue
        if int(cnt[k].sum()) > DEEP_ABOVE:
            recs["info"][k] |= DEEP << 8
            n_deep += 1
        else:
            recs["aq"][k] = aq_of(cnt[k], lfact, fisher)
    totals = (len(hs), total, n_obs, n_a1, int(cnt.sum()), n_deep, 0, 0)
    return recs[:stored], totals


def gt_letters(gt):
    return GENOTYPES[gt] if gt <= 9 else "NN"


def format_pairs(contig, recs, params=None):
    """LINE: (the table's bytes, its lines) for a PAIR array."""
    p = _params(params)
    c = check_contig(contig)
    need = max(1, int(p["min_cov"]))
    out = []
    for r in np.asarray(recs, dtype=PAIR):
        m1, u1, m2, u2 = (int(r[f]) for f in ("m1", "u1", "m2", "u2"))
        if int(r["info"]) >> 8 or m1 + u1 < need or m2 + u2 < need:
            continue
        s, h = int(r["cpg_pos"]), int(r["snp_pos"])
        cols = [b"%d" % ((s - 1) & 0xFFFFFFFF), b"%d" % (s + 1), b"%d" % h, gt_letters(int(r["info"]) & 0xFF).encode()]
        cols += [b"%d" % v for v in (m1, u1, m2, u2, int(r["aq"]), s - h)]
        out.append(c + b"\t" + b"\t".join(cols) + b"\n")
    return b"".join(out), len(out)


def read_table(data):
    """The table's lines back: (contig names as a list of bytes, a PAIR array; the flags of a written line are 0)."""
    names, rows = [], []
    for line in bytes(data).split(b"\n"):
        if not line:
            continue
        f = line.split(b"\t")
        if len(f) != 11:
            raise ValueError("a line of %d columns, not 11" % len(f))
        start, end, h = int(f[1]), int(f[2]), int(f[3])
        if end != start + 2 or int(f[10]) != start + 1 - h:
            raise ValueError("end is not start + 2, or dist is not cpg_pos - snp_pos")
        names.append(f[0])
        rows.append((h, start + 1, int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9]), GENOTYPES.index(f[4].decode())))
    return names, np.array(rows, dtype=PAIR) if rows else np.zeros(0, PAIR)
