"""The per-region methylation summary in Python — written from the rule as include/bscall_amd.h states it (site, region, sums, line), not
from csrc/methregions.c or csrc/methregionsdev.hip, whose checker it is in tests/test_methregions_host.py and
tests/test_gpu_methregions.py.  Plain Python integers: nothing wraps here.

A site is (pos, a, b); a region is (start, end), 0-based and half-open; the sums of a region are [sites, A, B, P]."""
import struct

import numpy as np

DEFAULT = {"contexts": 0, "min_cov": 1, "min_phred": 0, "pass_only": 0}


def site_of_rec_bytes(raw, params=None, present=True):
    """None, or (pos, a, b) of the site the 128 bytes of a packed record give under the per-cytosine rule.  present: False for a position
    whose emit byte (the chain's array beside the records) is 0."""
    p = dict(DEFAULT, **(params or {}))
    pos, emit, gt, _ref, _enc, flt, phred, _ngl, cg = struct.unpack_from("<IBBBBBBBB", raw, 0)
    if not present or not emit or gt not in (4, 7):
        return None
    if cg != ord("C") and not (p["contexts"] == 1 and cg == ord("H")):
        return None
    counts = struct.unpack_from("<8I", raw, 64)
    a, b = (counts[5], counts[7]) if gt == 4 else (counts[6], counts[4])
    if a + b < max(1, p["min_cov"]) or phred < p["min_phred"] or (p["pass_only"] and flt):
        return None
    return (pos, a, b)


def sites_of_rec_bytes(raw, params=None, emit=None):
    """raw: n x 128 record bytes; emit: a byte per record or None."""
    out = []
    for i in range(len(raw) // 128):
        s = site_of_rec_bytes(raw[128 * i : 128 * i + 128], params, emit is None or emit[i] != 0)
        if s is not None:
            out.append(s)
    return out


def pct(a, n):
    return (200 * a + n) // (2 * n)


def summary(sites, regions, acc=None):
    """[[sites, A, B, P]] per region, added to acc where given."""
    acc = [[0, 0, 0, 0] for _ in regions] if acc is None else [list(map(int, v)) for v in acc]
    for pos, a, b in sites:
        if pos == 0:
            continue
        for k, (start, end) in enumerate(regions):
            assert start <= end
            if start < pos <= end:
                acc[k][0] += 1
                acc[k][1] += a
                acc[k][2] += b
                acc[k][3] += pct(a, a + b)
    return acc


def lines(contig, regions, names, acc):
    out = []
    for k, ((start, end), (n, A, B, P)) in enumerate(zip(regions, acc)):
        name = "." if names is None or names[k] is None else names[k]
        level, mean = (str(pct(A, A + B)), str((2 * P + n) // (2 * n))) if n else (".", ".")
        out.append("\t".join([contig, str(start), str(end), name, str(n), str(A + B), str(A), str(B), level, mean]) + "\n")
    return "".join(out).encode()


def sites_of_bcf_record(dec, params=None):
    """dec: a BCF2 record as oracle.py_bcf.decode_record returns it -> None or (pos, a, b), from the file's own fields."""
    p = dict(DEFAULT, **(params or {}))
    f = dec["fmt"]
    idx = [(g >> 1) - 1 for g in f["GT"]]
    bases = [dec["alleles"][i] if 0 <= i < len(dec["alleles"]) else b"?" for i in idx]
    strand = "+" if bases == [b"C", b"C"] else ("-" if bases == [b"G", b"G"] else None)
    cg = f["CG"][0] if len(f["CG"]) else 0
    if strand is None or (cg != ord("C") and not (p["contexts"] == 1 and cg == ord("H"))):
        return None
    mc8 = f["MC8"]
    a, b = (mc8[5], mc8[7]) if strand == "+" else (mc8[6], mc8[4])
    flt = dec["filter"][0] != "PASS"
    if a + b < max(1, p["min_cov"]) or f["GQ"][0] < p["min_phred"] or (p["pass_only"] and flt):
        return None
    return (dec["pos"], a, b)


# ---- what both test files draw their inputs from ---------------------------------------------------------------------------------------------
def random_records(rng, n, x0=1, wide=False):
    """Random bytes in every field at positions x0, x0 + 1, ..; emit, gt, cg, flt, phred and the counts then drawn so that most records are
    sites, some fail one condition each."""
    recs = rng.integers(0, 256, (n, 128), dtype=np.uint8).view(_vcf_rec()).reshape(-1)
    core = recs["core"]
    core["pos"] = (x0 + np.arange(n, dtype=np.uint64)).astype(np.uint32)
    core["emit"] = rng.choice([0, 1, 1, 1, 1, 1, 255], n)
    core["gt"] = rng.choice([4, 7, 4, 7, 4, 7, 0, 5], n)
    core["flt"] = rng.choice([0, 0, 0, 1, 8, 128, 143], n)
    core["phred"] = rng.choice([0, 19, 20, 99, 100, 255], n)
    core["cg"] = rng.choice(list(b"CCCCCCHN"), n).astype(np.uint8).view("S1")
    scale = rng.choice([0, 1, 3, 30, 1000, 70000, 2**32 - 1] if wide else [0, 1, 3, 30, 1000], (n, 8))
    recs["counts"] = (rng.random((n, 8)) * (scale + 1)).astype(np.uint64).clip(0, 2**32 - 1).astype(np.uint32)
    recs["core"] = core
    return recs


def region_sets(x0, n):
    """Sorted (start, end) lists over positions x0 .. x0 + n - 1 holding every relation: duplicates, nesting, staggered overlaps, empty
    regions, regions before, behind and across the records, one over everything."""
    lo, hi = x0 - 1, x0 - 1 + n  # the half-open interval of the records' bedMethyl starts
    regs = [(max(lo - 50, 0), hi + 50), (max(lo - 50, 0), hi + 50), (max(lo - 50, 0), lo), (max(lo - 50, 0), lo + 1), (lo, lo), (lo, lo + 1), (lo, hi)]
    regs += [(lo + s, min(lo + s + 40, hi + 9)) for s in range(0, n, 25)]  # staggered overlaps
    regs += [(lo + n // 4, lo + 3 * n // 4), (lo + n // 3, lo + n // 2), (lo + n // 3, lo + n // 2), (lo + n // 3 + 1, lo + n // 3 + 1)]  # nested, twice, empty
    regs += [(hi - 1, hi), (hi - 1, hi + 30), (hi, hi), (hi, hi + 30), (hi + 5, hi + 30)]
    top = 2**32 - 1  # (records at the top of the coordinate range: the regions end there)
    return sorted((min(s, top), min(e, top)) for s, e in regs)


def _vcf_rec():
    from bs_call_amd.abi import VCF_REC

    return VCF_REC
