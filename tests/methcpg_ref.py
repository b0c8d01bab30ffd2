"""The combined-strand CpG table in Python — written from the rule as include/bscall_amd.h states it (halves, pairs and singles, which
records give a line, the columns), not from csrc/methcpg.c or csrc/methdev.hip, whose checker it is in tests/test_methcpg_host.py and
tests/test_gpu_methcpg.py.

A site is what the rule reads of one record: (pos, strand, cg, mc8, gq, flt) — strand "+" for a written CC call, "-" for a written GG
call, anything else for a record that cannot be a half (not written, another call).  Sites are given in record order; "the next record"
is the next element."""
import struct

RGB = ["0,255,0", "55,255,0", "105,255,0", "155,255,0", "205,255,0", "255,255,0", "255,205,0", "255,155,0", "255,105,0", "255,55,0", "255,0,0"]
DEFAULT = {"contexts": 0, "min_cov": 1, "min_phred": 0, "pass_only": 0}
FLT_OF_TEXT = {"PASS": 0, "mac1": 128, "fail": 1}  # a file says which of the three; the chain sets mac1 only on a record without a fail bit


def _half(site, p):
    """None, or (minus, a, b) of a half."""
    pos, strand, cg, mc8, gq, flt = site
    if strand not in ("+", "-") or cg != ord("C") or gq < p["min_phred"] or (p["pass_only"] and flt):
        return None
    a, b = (mc8[5], mc8[7]) if strand == "+" else (mc8[6], mc8[4])
    return (strand == "-", a, b) if a + b >= 1 else None


def lines(contig, sites, params=None):
    """[(index of the record the line is placed at, line, A, B, is a pair)] in record order."""
    p = dict(DEFAULT, **(params or {}))
    assert p["contexts"] == 0, "only a CpG has a partner strand"
    halves = [_half(s, p) for s in sites]
    out = []
    for i, (s, h) in enumerate(zip(sites, halves)):
        if h is None:
            continue
        minus, A, B = h
        pos, gq, flt = s[0], s[4], s[5]
        if minus and i > 0 and halves[i - 1] is not None and not halves[i - 1][0] and sites[i - 1][0] + 1 == pos:
            continue  # the minus half of a pair: the line is the plus half's
        pair = not minus and i + 1 < len(sites) and halves[i + 1] is not None and halves[i + 1][0] and sites[i + 1][0] == pos + 1
        if pair:
            A, B, gq, flt = A + halves[i + 1][1], B + halves[i + 1][2], min(gq, sites[i + 1][4]), flt | sites[i + 1][5]
        cov = A + B
        if cov < max(1, p["min_cov"]):
            continue
        pct = (200 * A + cov) // (2 * cov)
        start = (pos - (2 if minus else 1)) & 0xFFFFFFFF
        ft = "fail" if flt & 127 else ("mac1" if flt & 128 else "PASS")
        cols = [start, start + 2, "CG", min(cov, 1000), "." if pair else ("-" if minus else "+"), start, start + 2, RGB[pct // 10], cov, pct, A, B, gq, ft]
        out.append((i, contig + b"\t" + "\t".join(str(v) for v in cols).encode() + b"\n", A, B, pair))
    return out


def table(contig, sites, params=None):
    """(the table's bytes, [length, lines, sum of A, sum of B, pairs written])."""
    ls = lines(contig, sites, params)
    data = b"".join(ln for _, ln, _, _, _ in ls)
    return data, [len(data), len(ls), sum(v[2] for v in ls), sum(v[3] for v in ls), sum(1 for v in ls if v[4])]


def site_of_rec_bytes(raw, present=True):
    """raw: the 128 bytes of a packed record (bsc_vcf_rec), whatever they hold.  present: False for a position whose emit byte (the
    chain's array beside the records) is 0."""
    pos, emit, gt, _ref, _enc, flt, phred, _ngl, cg = struct.unpack_from("<IBBBBBBBB", raw, 0)
    strand = {4: "+", 7: "-"}.get(gt) if emit and present else None
    return (pos, strand, cg, struct.unpack_from("<8I", raw, 64), phred, flt)


def of_rec_bytes(raw, contig, params=None, n=None, emit=None):
    """raw: n_max x 128 record bytes; n: how many of them exist (default all); emit: a byte per position or None."""
    rows = len(raw) // 128 if n is None else n
    sites = [site_of_rec_bytes(raw[128 * i : 128 * i + 128], emit is None or emit[i] != 0) for i in range(rows)]
    return table(contig, sites, params)


def site_of_bcf_record(dec):
    """dec: a BCF2 record as oracle.py_bcf.decode_record returns it — the file's own fields: POS, FILTER, GT with the alleles, GQ, CG, MC8."""
    f = dec["fmt"]
    idx = [(g >> 1) - 1 for g in f["GT"]]
    bases = [dec["alleles"][i] if 0 <= i < len(dec["alleles"]) else b"?" for i in idx]
    strand = "+" if bases == [b"C", b"C"] else ("-" if bases == [b"G", b"G"] else None)
    cg = f["CG"][0] if len(f["CG"]) else 0
    return (dec["pos"], strand, cg, f["MC8"], f["GQ"][0], FLT_OF_TEXT[dec["filter"][0]])


def bcf_records(blob, at=0):
    from oracle import py_bcf

    while at < len(blob):
        l_shared, l_indiv = struct.unpack_from("<II", blob, at)
        yield py_bcf.decode_record(blob[at : at + 8 + l_shared + l_indiv])
        at += 8 + l_shared + l_indiv


def of_bcf_stream(blob, contig, params=None):
    """The table of a stream of BCF2 records (no header) of one contig, as (bytes, totals)."""
    return table(contig, [site_of_bcf_record(d) for d in bcf_records(blob)], params)


def of_bcf_file(plain_bcf, names, params=None):
    """The table of a whole uncompressed BCF file: contig by contig (a pair never spans two), from its own records.  names[rid] = bytes."""
    (lt,) = struct.unpack_from("<I", plain_bcf, 5)
    by_rid, order = {}, []
    for d in bcf_records(plain_bcf, 9 + lt):
        if d["rid"] not in by_rid:
            by_rid[d["rid"]] = []
            order.append(d["rid"])
        by_rid[d["rid"]].append(site_of_bcf_record(d))
    parts = [table(names[r], by_rid[r], params) for r in order]
    return b"".join(t[0] for t in parts), [sum(t[1][k] for t in parts) for k in range(5)]
