"""The variant-only call set in Python: the rule of include/bscall_amd.h (VARIANT, PARAMS, SELECTED, TOTALS) over raw VCF_REC arrays and
over decoded records, written from the rule — the third form beside the kernels (csrc/variantsdev.hip) and the host form
(csrc/variants.c), for tests and for users who hold records in numpy."""

import numpy as np

from .abi import VCF_REC

N_TOTALS = 10
TOTAL_NAMES = ("records", "snp", "multi", "het", "pass", "known", "known_pass", "ts", "tv", "phred_sum")
HET_GT = (1, 2, 3, 5, 6, 8)
_TRANSITIONS = {("A", "G"), ("G", "A"), ("C", "T"), ("T", "C")}


def _params(params):
    p = {"min_phred": 0, "pass_only": 0, "known_only": 0, "reserved": 0}
    if params is None:
        return p
    if isinstance(params, dict):
        unknown = set(params) - set(p)
        if unknown:
            raise ValueError("unknown variant parameter(s): %s" % ", ".join(sorted(unknown)))
        p.update(params)
    else:  # a _lib.VarParams
        for k in p:
            p[k] = getattr(params, k)
    if int(p["reserved"]) != 0:
        raise ValueError("reserved must be 0")
    return p


def _bytes(recs):
    recs = np.ascontiguousarray(recs, dtype=VCF_REC)
    return recs, recs.view(np.uint8).reshape(-1, 128)


def select(recs, params=None, emit=None):
    """The indices (ascending: position order) of the selected records of a VCF_REC array.  emit: the per-position form's byte per entry
    (a record whose byte is 0 is no variant), or None."""
    p = _params(params)
    recs, b = _bytes(recs)
    m = (b[:, 4] != 0) & (b[:, 12] != 0)  # core.emit, core.alt[0]
    if emit is not None:
        m &= np.asarray(emit).reshape(-1) != 0
    m &= b[:, 9].astype(np.int64) >= int(p["min_phred"])  # core.phred
    if p["pass_only"]:
        m &= b[:, 8] == 0  # core.flt
    if p["known_only"]:
        m &= b[:, 113] != 0  # rs_found: byte 49 of the aux half
    return np.nonzero(m)[0]


def totals(recs):
    """The ten totals over records that ARE selected (a VCF_REC array: select's rows)."""
    recs, b = _bytes(recs)
    gt, ref_code, flt, phred, a0, a1, rs = b[:, 5], b[:, 6], b[:, 8], b[:, 9], b[:, 12], b[:, 13], b[:, 113]
    snp = a1 == 0
    tstv = snp & (ref_code >= 1) & (ref_code <= 4) & np.isin(a0, np.frombuffer(b"ACGT", np.uint8))
    ref_ch = np.frombuffer(b"NACGTNNN", np.uint8)[np.minimum(ref_code, 7)]
    ts = np.zeros(len(b), bool)
    for r, a in _TRANSITIONS:
        ts |= tstv & (ref_ch == ord(r)) & (a0 == ord(a))
    return (len(b), int(snp.sum()), int((~snp).sum()), int(np.isin(gt, HET_GT).sum()), int((flt == 0).sum()), int((rs != 0).sum()),
            int(((rs != 0) & (flt == 0)).sum()), int(ts.sum()), int((tstv & ~ts).sum()), int(phred.astype(np.uint64).sum()))


def select_decoded(records, params=None):
    """The rule over decoded records — dicts with "alt" (a list of ALT alleles, empty or ["."] for none), "qual" (the integer QUAL),
    "filter" ("PASS" or the failed filters) and "known" (the dbSNP flag the block was given): the indices of the selected ones."""
    p = _params(params)
    out = []
    for k, r in enumerate(records):
        alt = [a for a in r["alt"] if a not in (".", "")]
        if not alt or int(r["qual"]) < int(p["min_phred"]):
            continue
        if p["pass_only"] and r["filter"] != "PASS":
            continue
        if p["known_only"] and not r["known"]:
            continue
        out.append(k)
    return out


def totals_decoded(records):
    """The ten totals over decoded records that ARE selected: the keys of select_decoded plus "ref" (the REF base) and "gt" (the two allele
    indices of FORMAT GT)."""
    t = [0] * N_TOTALS
    for r in records:
        alt = [a for a in r["alt"] if a not in (".", "")]
        passed, known = r["filter"] == "PASS", bool(r["known"])
        t[0] += 1
        t[1 if len(alt) == 1 else 2] += 1
        t[3] += int(r["gt"][0] != r["gt"][1])
        t[4] += int(passed)
        t[5] += int(known)
        t[6] += int(known and passed)
        if len(alt) == 1 and r["ref"] in "ACGT" and alt[0] in ("A", "C", "G", "T"):
            t[7 if (r["ref"], alt[0]) in _TRANSITIONS else 8] += 1
        t[9] += int(r["qual"])
    return tuple(t)
