"""The bedMethyl line of a record, in Python — written from the rule as include/bscall_amd.h states it, not from csrc/methbed.c or
csrc/methdev.hip, whose checker it is in tests/test_methbed_host.py and tests/test_gpu_methbed.py.

A record gives a line iff it is written (emit), called homozygous CC (strand +) or GG (strand -), its CG status is 'C' (or 'H' when
every context is asked for), a + b >= max(1, min_cov), GQ >= min_phred and, with pass_only, FILTER is PASS; a / b = the non-converted /
converted count of the strand: MC8[5], MC8[7] for +, MC8[6], MC8[4] for -."""
import struct

CPG, ALL = 0, 1
RGB = ["0,255,0", "55,255,0", "105,255,0", "155,255,0", "205,255,0", "255,255,0", "255,205,0", "255,155,0", "255,105,0", "255,55,0", "255,0,0"]
DEFAULT = {"contexts": CPG, "min_cov": 1, "min_phred": 0, "pass_only": 0}


def line(contig, pos, strand, cg, cx_gt, mc8, gq, filter_text, params=None):
    """strand: "+" for a CC call, "-" for a GG call, anything else: no line.  cg: the CG status byte (int).  cx_gt: the five bytes of the
    called context (shorter: padded with NUL).  filter_text: the FILTER column's text.  Returns bytes, b"" for no line."""
    p = dict(DEFAULT, **(params or {}))
    if strand not in ("+", "-"):
        return b""
    if cg != ord("C") and not (p["contexts"] == ALL and cg == ord("H")):
        return b""
    a, b = (mc8[5], mc8[7]) if strand == "+" else (mc8[6], mc8[4])
    cov = a + b
    if cov < max(1, p["min_cov"]) or gq < p["min_phred"] or (p["pass_only"] and filter_text != "PASS"):
        return b""
    if cg == ord("C"):
        name = "CG"
    else:
        cx = bytes(cx_gt).ljust(5, b"\0")
        n2 = cx[4] if strand == "+" else cx[0]
        if n2 == (ord("G") if strand == "+" else ord("C")):
            name = "CHG"
        elif n2 in b"ACGT":
            name = "CHH"
        else:
            name = "CHN"
    pct = (200 * a + cov) // (2 * cov)
    start = (pos - 1) & 0xFFFFFFFF
    cols = [start, pos, name, min(cov, 1000), strand, start, pos, RGB[pct // 10], cov, pct, a, b, gq, filter_text]
    return contig + b"\t" + "\t".join(str(v) for v in cols).encode() + b"\n"


def of_rec_bytes(raw, contig, params=None):
    """raw: the 128 bytes of a packed record (bsc_vcf_rec), whatever they hold."""
    pos, emit, gt, _ref, _enc, flt, phred, _ngl, cg = struct.unpack_from("<IBBBBBBBB", raw, 0)
    if not emit:
        return b""
    mc8 = struct.unpack_from("<8I", raw, 64)
    ft = "PASS" if flt == 0 else ("mac1" if flt & 128 else "fail")
    return line(contig, pos, {4: "+", 7: "-"}.get(gt), cg, raw[19:24], mc8, phred, ft, params)


def of_bcf_record(dec, contig, params=None):
    """dec: a BCF2 record as oracle.py_bcf.decode_record returns it — the file's own fields: POS, FILTER, GT with the alleles, GQ, CG, CX,
    MC8."""
    f = dec["fmt"]
    idx = [(g >> 1) - 1 for g in f["GT"]]
    bases = [dec["alleles"][i] if 0 <= i < len(dec["alleles"]) else b"?" for i in idx]
    strand = "+" if bases == [b"C", b"C"] else ("-" if bases == [b"G", b"G"] else None)
    cg = f["CG"][0] if len(f["CG"]) else 0
    return line(contig, dec["pos"], strand, cg, f["CX"], f["MC8"], f["GQ"][0], dec["filter"][0], params)


def of_bcf_stream(blob, contig, params=None):
    """The table of a stream of BCF2 records (no header) of one contig."""
    from oracle import py_bcf

    out, o = [], 0
    while o < len(blob):
        l_shared, l_indiv = struct.unpack_from("<II", blob, o)
        out.append(of_bcf_record(py_bcf.decode_record(blob[o : o + 8 + l_shared + l_indiv]), contig, params))
        o += 8 + l_shared + l_indiv
    return b"".join(out)
