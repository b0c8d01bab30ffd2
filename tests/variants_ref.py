"""TEST INFRASTRUCTURE — the variant-only call set read back from a block's FULL stream, independently of the library: the stream is split
into its records (BCF2: l_shared / l_indiv; text: lines), the fields the rule of include/bscall_amd.h names are read from each — POS,
the alleles, QUAL, FILTER and FORMAT GT —, the rule is applied, and the selected records' byte ranges come back joined, with the ten
totals.  `known`: the positions (1-based) the dbSNP flag array the test gave the block is non-zero at.  Nothing here calls the library."""
import struct

N_TOTALS = 10
_TS = {(b"A", b"G"), (b"G", b"A"), (b"C", b"T"), (b"T", b"C")}
_ACGT = (b"A", b"C", b"G", b"T")


def _typed(b, o):
    """one BCF2 typed value at b[o]: (type, values or bytes, next offset)"""
    d = b[o]
    o += 1
    n, t = d >> 4, d & 15
    if n == 15:
        _, (n,), o = _typed(b, o)
    if t == 7:
        return t, b[o : o + n], o + n
    fmt = {0: "b", 1: "b", 2: "h", 3: "i", 5: "f"}[t]
    w = struct.calcsize(fmt) if t else 0
    return t, (list(struct.unpack_from("<%d%s" % (n, fmt), b, o)) if t else []), o + n * w


def bcf_records(stream):
    """[(begin, end, fields)] of a stream of whole BCF2 records"""
    out, at = [], 0
    while at < len(stream):
        l_shared, l_indiv, _rid, pos0, _rlen, qual, nai, _nfs = struct.unpack_from("<IIiiifII", stream, at)
        end = at + 8 + l_shared + l_indiv
        assert end <= len(stream)
        n_allele = nai >> 16
        o = at + 32
        _, _id, o = _typed(stream, o)
        alleles = []
        for _ in range(n_allele):
            _, a, o = _typed(stream, o)
            alleles.append(bytes(a))
        _, flt, o = _typed(stream, o)
        o = at + 8 + l_shared  # FORMAT: the first field is GT, two allele codes (allele + 1) << 1
        _, _key, o = _typed(stream, o)
        _, gt, o = _typed(stream, o)
        assert len(gt) == 2
        out.append((at, end, {"pos": pos0 + 1, "ref": alleles[0], "alt": alleles[1:], "qual": int(qual), "passed": flt == [0],
                              "gt": ((gt[0] >> 1) - 1, (gt[1] >> 1) - 1)}))
        assert float(int(qual)) == qual
        at = end
    return out


def text_records(stream):
    """[(begin, end, fields)] of a stream of whole VCF data lines: columns 2, 4, 5, 6, 7 and the GT field"""
    out, at = [], 0
    while at < len(stream):
        end = stream.index(b"\n", at) + 1
        f = stream[at : end - 1].split(b"\t")
        keys, vals = f[8].split(b":"), f[9].split(b":")
        gt = vals[keys.index(b"GT")].replace(b"|", b"/").split(b"/")
        out.append((at, end, {"pos": int(f[1]), "ref": f[3], "alt": [] if f[4] == b"." else f[4].split(b","), "qual": int(f[5]),
                              "passed": f[6] == b"PASS", "gt": (int(gt[0]), int(gt[1]))}))
        at = end
    return out


def select(stream, text, params=None, known=()):
    """(the selected records' bytes joined, records, totals[10]) of a block's full stream.  params: dict of min_phred / pass_only /
    known_only; known: a set of 1-based positions."""
    p = {"min_phred": 0, "pass_only": 0, "known_only": 0}
    p.update(params or {})
    known = set(int(k) for k in known)
    parts, t = [], [0] * N_TOTALS
    for beg, end, r in (text_records if text else bcf_records)(stream):
        if not r["alt"]:
            continue
        kn = r["pos"] in known
        if r["qual"] < p["min_phred"] or (p["pass_only"] and not r["passed"]) or (p["known_only"] and not kn):
            continue
        parts.append(stream[beg:end])
        t[0] += 1
        t[1 if len(r["alt"]) == 1 else 2] += 1
        t[3] += r["gt"][0] != r["gt"][1]
        t[4] += r["passed"]
        t[5] += kn
        t[6] += kn and r["passed"]
        if len(r["alt"]) == 1 and r["ref"] in _ACGT and r["alt"][0] in _ACGT:
            t[7 if (r["ref"], r["alt"][0]) in _TS else 8] += 1
        t[9] += r["qual"]
    return b"".join(parts), t[0], tuple(int(v) for v in t)

