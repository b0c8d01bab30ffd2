"""BAM alignment records for the pin of the record parser (tests/test_ref_pin_bam.py, tests/test_gpu_ref_pin.py,
tools/make_ref_align_vectors.py): what reaches get_next_align_details of the reference (src/input_sam.c) and its three forms here —
bd_parse / bd_misms_of / bd_base_byte (csrc/bamdev_core.h, the device reader), next_record / store_read (csrc/bamio.c, the host
reader), oracle/py_bam.py.  No test asserts here; no reference code is loaded here.

A group is a list of Case(name, raw, cpu_only): `raw` is the record as a BAM file holds it (block_size first), made by
tools/make_bam.encode_record.  The groups

  aux    the optional fields get_bs_strand walks: every value type as a skipped tag, every aligner's tag, wrong types, truncations,
         `B` arrays with counts inside, beyond and wrapped round the record
  cigar  every operation code 0..15, clips and indels at the ends, no CIGAR, no bases, 300 operations
  seq    every nibble code in both positions with the qualities round the clamp at 43; the lengths round the decode kernel's
         four-base lane, its tail and its 256-base round, on both strands
  mix    a seeded mix of the pieces above; one record in 25 is about 8 KB long (a 5003-base read, a `B` array of 4096 words)

are SINGLE-END records (flag 0 or 16, no mate position) at strictly increasing positions of one contig, names unique: written to a
file, one used record is one template of the readers, and nothing pairs or counts as a duplicate.  The query length of a CIGAR
equals l_seq everywhere except in the cases marked cpu_only: the readers here drop such a record before they look at it
(DESIGN.md section 3), the reference walks it, so it is held against the reference on the CPU alone — by oracle/py_bam.py in every
field (it walks the CIGAR as the reference does), by bd_parse in its status only (every other field of its descriptor is
computed after the drop) — and never written to a file for the GPU.

  fixed  the 32 fixed bytes: all 4096 flag values with the mate right and left of the record, and mate position, contig, insert
         size and MAPQ at their edges.  Records of ten bases; positions strictly increasing here too, so that the part of the group
         a reader accepts as a file (gpu_flag_file) keeps the one-record-one-template property.
"""
import collections
import importlib.util
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_bam_for_cases", os.path.join(ROOT, "tools", "make_bam.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

REFS = [("chr1", 50_000_000), ("chr2", 1_000_000)]
MAPQ_THRESH, MAX_TEMPLATE_LEN = 20, 1000
# (keep_unmatched, ignore_duplicates)
SETTINGS = [(False, False), (False, True), (True, False), (True, True)]
CODES = "=ACMGRSVTWYHKDBN"
QUALS = [0, 1, 42, 43, 44, 93, 254, 255]
LENGTHS = list(range(0, 9)) + list(range(251, 262)) + list(range(511, 518)) + [1023, 1025, 5003]

Case = collections.namedtuple("Case", "name raw cpu_only")


def setting_key(s):
    return "ku%d_id%d" % (int(s[0]), int(s[1]))


def _rec(name, flag=0, pos=0, mpos=-1, seq="ACGTACGTAC", cigar=None, mapq=60, tid=0, mtid=-1, tlen=0, qual=None, aux=b""):
    if cigar is None:
        cigar = [("M", len(seq))] if seq else []
    return W.encode_record(dict(name=name, flag=flag, tid=tid, pos=pos, mapq=mapq, cigar=cigar, mtid=mtid, mpos=mpos, tlen=tlen, seq=seq,
                                qual=[30] * len(seq) if qual is None else qual, aux=aux))


class _Placer:
    """gives every record of the file groups its own name and position: single-end, strictly increasing, far enough apart that a
    template's positions never equal another's"""

    def __init__(self, start):
        self.pos = start
        self.n = 0

    def __call__(self, group, name, cpu_only=False, reverse=False, span_hint=0, **kw):
        self.n += 1
        self.pos += 37 + span_hint // 64
        return Case("%s/%s" % (group, name), _rec("%s%05d" % (group[0], self.n), flag=16 if reverse else 0, pos=self.pos, **kw), cpu_only)


# ---- aux -----------------------------------------------------------------------------------------------------------------------------
XB_C = b"XBAC"
SUB_SIZE = {"c": 1, "C": 1, "A": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}


def _b_array(sub, count, payload=None, tag=b"ZZ"):
    size = SUB_SIZE.get(sub, 0)
    body = bytes((7 * i + 1) & 0xFF for i in range(count * size)) if payload is None else payload
    return tag + b"B" + sub.encode() + struct.pack("<I", count) + body


def aux_pieces():
    """[(name, aux bytes)]"""
    out = []
    skipped = {"A": b"q", "c": b"\x80", "C": b"\xff", "s": b"\x01\x80", "S": b"\xff\xff", "i": struct.pack("<i", -5), "I": struct.pack("<I", 0xFFFFFFFF),
               "f": struct.pack("<f", 1.5), "d": struct.pack("<d", -2.25), "Z": b"some text\0", "H": b"1AE301\0"}
    for ty, val in skipped.items():
        out.append(("skip %s then XB:A:C" % ty, b"ZZ" + ty.encode() + val + XB_C))
    out.append(("skip empty Z then XB:A:C", b"ZZZ\0" + XB_C))
    for sub in SUB_SIZE:
        for n in (0, 1, 3):
            out.append(("skip B%s x%d then XB:A:C" % (sub, n), _b_array(sub, n) + XB_C))
    for tag, ty, vals in (("XB", "A", "CGT"), ("XG", "Z", ("CT", "GA", "xx")), ("ZB", "Z", ("CT", "GA", "xx")), ("ZS", "Z", ("++", "+-", "-+", "--", "xx")),
                          ("YD", "Z", ("f", "r", "x"))):
        for v in vals:
            out.append(("%s:%s:%s" % (tag, ty, v), tag.encode() + ty.encode() + v.encode() + (b"\0" if ty == "Z" else b"")))
    out.append(("ZB:Z empty", b"ZBZ\0"))
    for tag, ty, v in (("XB", "Z", "C"), ("XG", "A", "C"), ("ZS", "A", "+"), ("YD", "A", "f"), ("ZB", "A", "G"), ("XB", "c", "C"), ("XG", "H", "47")):
        out.append(("wrong type %s:%s:%s" % (tag, ty, v), tag.encode() + ty.encode() + v.encode() + (b"\0" if ty in "ZH" else b"")))
    out.append(("two tags, the later decides", b"XBAC" + b"XBAG"))
    out.append(("two tags of two aligners", b"XGZGA\0" + b"ZSZ++\0"))
    out.append(("a later tag without a meaning", b"XBAG" + b"XBAT"))
    out.append(("a later Z tag without a meaning", b"YDZr\0" + b"NMi" + struct.pack("<i", 2) + b"XGZxx\0"))
    out.append(("unknown type letter consumes nothing", b"ZZ?" + XB_C))
    out.append(("unknown type letter, walk out of step", b"ZZ?q" + XB_C))
    out.append(("aux of 1 byte", b"X"))
    out.append(("aux of 2 bytes", b"XB"))
    out.append(("aux of 3 bytes", b"XBA"))
    out.append(("aux of 4 bytes", XB_C))
    out.append(("no aux", b""))
    out.append(("Z without its NUL", b"XGZCT"))
    out.append(("skipped Z without its NUL", b"XBAG" + b"ZZZabc"))
    out.append(("H without its NUL", b"XBAC" + b"ZZH00"))
    out.append(("s one byte short", b"XBAG" + b"ZZs\x01"))
    out.append(("i one byte short", b"XBAG" + b"ZZi\x01\x02\x03"))
    out.append(("f one byte short", b"XBAC" + b"ZZf\x01\x02\x03"))
    out.append(("d one byte short", b"XBAG" + b"ZZd" + bytes(7)))
    out.append(("d exactly to the end", b"ZZd" + bytes(8)))
    out.append(("B count beyond the end", b"XBAG" + _b_array("c", 100, payload=b"") + XB_C))
    out.append(("B count one beyond the end", _b_array("i", 2, payload=bytes(7))))
    out.append(("B count exactly to the end", b"XBAG" + _b_array("i", 2, payload=bytes(8))))
    out.append(("B count field cut", b"XBAG" + b"ZZBi\x01\x00"))
    out.append(("B subtype Z x1", b"ZZBZ" + struct.pack("<I", 1) + bytes(90) + XB_C))
    out.append(("B subtype Z x0", b"ZZBZ" + struct.pack("<I", 0) + XB_C))
    out.append(("B subtype H x1", b"ZZBH" + struct.pack("<I", 1) + bytes(72) + XB_C))
    out.append(("B subtype B x1", b"ZZBB" + struct.pack("<I", 1) + bytes(66) + XB_C))
    out.append(("B unknown subtype", b"XBAG" + b"ZZB?" + struct.pack("<I", 0) + XB_C))
    # the reference forms count * size in 32 bits: these products wrap to 0, 4, 0 and 0
    out.append(("B product wraps to 0", b"ZZBi" + struct.pack("<I", 0x40000000) + XB_C))
    out.append(("B product wraps to 4", b"ZZBi" + struct.pack("<I", 0x40000001) + bytes(4) + XB_C))
    out.append(("B product of s wraps to 0", b"ZZBs" + struct.pack("<I", 0x80000000) + b"XBAG"))
    out.append(("B product of subtype Z wraps to 0", b"ZZBZ" + struct.pack("<I", 0x80000000) + XB_C))
    out.append(("B product just below the wrap", b"XBAG" + b"ZZBi" + struct.pack("<I", 0x3FFFFFFF) + XB_C))
    out.append(("B array of 8 KB", _b_array("C", 8192) + XB_C))
    return out


def aux_cases(place):
    return [place("aux", n, aux=a, reverse=bool(i & 1)) for i, (n, a) in enumerate(aux_pieces())]


# ---- CIGAR ---------------------------------------------------------------------------------------------------------------------------
QUERY_OPS = {"M", "I", "S", "=", "X", 0, 1, 4, 7, 8}


def _qlen(cigar):
    return sum(n for op, n in cigar if op in QUERY_OPS)


def cigar_lists():
    """[(name, cigar, l_seq or None = the CIGAR's query length)]"""
    out = []
    for op in list("MIDNSHP=X") + list(range(9, 16)):
        out.append(("5M 3%s 5M" % op, [("M", 5), (op, 3), ("M", 5)], None))
        out.append(("%s alone" % op, [(op, 6)], None))
    out += [("H and S at both ends", [("H", 2), ("S", 3), ("M", 10), ("S", 2), ("H", 1)], None), ("I first", [("I", 2), ("M", 8)], None),
            ("D first", [("D", 3), ("M", 10)], None), ("I next to D", [("M", 4), ("I", 2), ("D", 3), ("M", 4)], None),
            ("D next to I", [("M", 4), ("D", 3), ("I", 2), ("M", 4)], None), ("two deletions", [("M", 3), ("D", 2), ("M", 3), ("D", 4), ("M", 4)], None),
            ("S first and last, I and D inside", [("S", 3), ("M", 4), ("I", 2), ("M", 3), ("D", 5), ("M", 2), ("S", 1)], None),
            ("no CIGAR, ten bases", [], 10), ("a CIGAR, no bases", [("M", 10)], 0), ("no CIGAR, no bases", [], 0),
            ("300 operations", [("M", 1), ("I", 1)] * 150, None), ("300 operations with deletions", [("M", 2), ("D", 1), ("S", 1)] * 100, None),
            ("5M2P5M", [("M", 5), ("P", 2), ("M", 5)], None), ("N between", [("M", 6), ("N", 1000), ("M", 6)], None),
            ("= and X", [("=", 4), ("X", 1), ("=", 5)], None), ("a length of 2^28 - 1 that consumes nothing", [("M", 10), ("H", (1 << 28) - 1)], None)]
    # query length != l_seq: cpu_only
    out += [("CIGAR longer than the bases", [("M", 14)], 10), ("CIGAR shorter than the bases", [("M", 6)], 10),
            ("clip and match shorter than the bases", [("S", 3), ("M", 4)], 10), ("insertion beyond the bases", [("M", 8), ("I", 5), ("D", 2)], 10)]
    return out


def cigar_cases(place):
    out = []
    for i, (name, cig, l_seq) in enumerate(cigar_lists()):
        q = _qlen(cig)
        n = q if l_seq is None else l_seq
        seq = ("ACGTTGCAN" * (n // 9 + 1))[:n]
        out.append(place("cigar", name, cpu_only=bool(n and cig and q != n), cigar=cig, seq=seq, qual=[(11 * k) % 50 for k in range(n)], reverse=bool(i % 3 == 1),
                         aux=b"XBAG" if i & 1 else b""))
    return out


# ---- sequence ------------------------------------------------------------------------------------------------------------------------
def seq_cases(place, lengths=LENGTHS):
    out = []
    for q in QUALS:
        out.append(place("seq", "16 codes, quality %d" % q, seq=CODES, qual=[q] * 16))
        out.append(place("seq", "16 codes in the other nibble, quality %d" % q, seq="A" + CODES, qual=[q] * 17, reverse=True))
    out.append(place("seq", "16 codes x 8 qualities", seq=CODES * 8 + CODES[1:] * 8, qual=[QUALS[(k // 16) % 8] for k in range(16 * 8 + 15 * 8)]))
    out.append(place("seq", "missing qualities", seq="ACGTNACGTA", qual=[255] * 10))
    rng = np.random.default_rng(20261101)
    letters = np.array(list(CODES))
    p = np.array([1, 20, 20, 1, 20, 1, 1, 1, 20, 1, 1, 1, 1, 1, 1, 6], dtype=float)
    p /= p.sum()
    for ln in lengths:
        for rev in (False, True):
            seq = "".join(rng.choice(letters, ln, p=p))
            qual = [int(v) for v in rng.choice(QUALS + list(range(2, 60)), ln)]
            out.append(place("seq", "length %d %s" % (ln, "reverse" if rev else "forward"), seq=seq, qual=qual, reverse=rev, span_hint=ln,
                             aux=b"XBAC" if ln & 1 else b"XGZGA\0"))
    return out


# ---- a seeded mix --------------------------------------------------------------------------------------------------------------------
def mix_cases(place, n=2000, seed=20261102):
    rng = np.random.default_rng(seed)
    pieces = [a for _, a in aux_pieces() if len(a) < 200]
    letters = np.array(list(CODES))
    p = np.array([1, 20, 20, 1, 20, 1, 1, 1, 20, 1, 1, 1, 1, 1, 1, 6], dtype=float)
    p /= p.sum()
    ops = list("MIDNSHP=X") + list(range(9, 16))
    op_p = np.array([30, 8, 8, 2, 6, 3, 2, 4, 4] + [0.5] * 7)
    op_p /= op_p.sum()
    out = []
    for i in range(n):
        k = int(rng.integers(0, 8))
        cig = [] if k == 0 else [(ops[int(rng.choice(len(ops), p=op_p))], int(rng.integers(1, 12))) for _ in range(k)]
        ln = _qlen(cig) if cig else int(rng.integers(0, 30))
        if rng.random() < 0.03:  # a long read: the decode kernel's second round
            extra = int(rng.integers(240, 300))
            cig = cig + [("M", extra)]
            ln = _qlen(cig)
        aux = b"".join(pieces[int(j)] for j in rng.integers(0, len(pieces), int(rng.integers(0, 4))))
        if i % 50 == 24:  # records of about 8 KB: in a reader whose slabs are small they lie across the slabs' ends
            cig, ln = cig + [("=", 5003)], _qlen(cig) + 5003
        elif i % 50 == 49:
            aux = _b_array("S", 4096) + aux
        seq = "".join(rng.choice(letters, ln, p=p))
        qual = [int(v) for v in rng.choice(QUALS + list(range(2, 60)), ln)]
        out.append(place("mix", "%d" % i, cigar=cig, seq=seq, qual=qual, aux=aux, reverse=bool(rng.integers(0, 2)), span_hint=ln,
                         mapq=int(rng.choice([20, 21, 60, 255]))))
    return out


# ---- fixed fields --------------------------------------------------------------------------------------------------------------------
def fixed_cases(flag_sample=None, seed=20261103):
    """flag_sample: None = all 4096 flag values, else how many of them (seeded) — the recorded fixture's reduction"""
    flags = list(range(4096))
    if flag_sample is not None:
        flags = sorted(int(v) for v in np.random.default_rng(seed).choice(4096, flag_sample, replace=False))
    out = []
    pos = [1000]

    def add(name, flag, d_mpos=None, **kw):
        pos[0] += 31
        mpos = kw.pop("mpos", None)
        if mpos is None:
            mpos = pos[0] + d_mpos
        kw.setdefault("mtid", 0)
        kw.setdefault("tlen", 0 if not d_mpos else (17 if d_mpos > 0 else -17))
        out.append(Case("fixed/%s" % name, _rec("f%05d" % len(out), flag=flag, pos=pos[0], mpos=mpos, aux=b"XBAC", **kw), False))

    for f in flags:
        add("flag %d, mate to the right" % f, f, 7)
        add("flag %d, mate to the left" % f, f, -7)
    M = MAX_TEMPLATE_LEN
    beside = (0, 16, 1, 3, 65, 67, 83, 99, 115, 129, 131, 147, 163, 179, 97, 145, 1024 | 99, 1024 | 147)
    for f in beside if flag_sample is None else (0, 16, 83, 99, 147, 163, 1024, 1024 | 99):
        add("flag %d, mate at the same position" % f, f, 0)
        add("flag %d, mate on another contig" % f, f, 7, mtid=1)
        add("flag %d, mate on another contig to the left" % f, f, -7, mtid=1)
        add("flag %d, no mate contig" % f, f, 7, mtid=-1)
        add("flag %d, no mate position" % f, f, mpos=-1)
        for isz in (0, M, -M, M + 1, -(M + 1), -(2**31) + 1, 2**31 - 1):
            add("flag %d, insert size %d, mate to the right" % (f, isz), f, 7, tlen=isz)
            add("flag %d, insert size %d, mate to the left" % (f, isz), f, -7, tlen=isz)
        for q in (0, MAPQ_THRESH - 1, MAPQ_THRESH, 255):
            add("flag %d, MAPQ %d, mate to the right" % (f, q), f, 7, mapq=q)
            add("flag %d, MAPQ %d, mate to the left" % (f, q), f, -7, mapq=q)
        add("flag %d, MAPQ 19 and another contig and a long insert" % f, f, 7, mapq=19, mtid=1, tlen=5000)
    return out


# ---- the groups -------------------------------------------------------------------------------------------------------------------------
FILE_GROUPS = ("aux", "cigar", "seq", "mix")


def groups(reduced=False):
    """group name -> [Case].  reduced: the recorded fixture's set — every aux and CIGAR case and every length; a sample of the flag
    sweep and a shorter mix."""
    place = _Placer(1000)
    g = collections.OrderedDict()
    g["aux"] = aux_cases(place)
    g["cigar"] = cigar_cases(place)
    g["seq"] = seq_cases(place)
    g["mix"] = mix_cases(place, 60 if reduced else 2000)
    g["fixed"] = fixed_cases(60 if reduced else None)
    return g


def pack(cases):
    """-> (the records' bytes, their offsets)"""
    offs, at = [], 0
    for c in cases:
        offs.append(at)
        at += len(c.raw)
    return np.frombuffer(b"".join(c.raw for c in cases), dtype=np.uint8).copy(), np.array(offs, dtype=np.uint64)


def unpack(records, offsets):
    """-> [raw record bytes]"""
    out = []
    for o in [int(v) for v in offsets]:
        bs = int.from_bytes(records[o : o + 4].tobytes(), "little")
        out.append(records[o : o + 4 + bs].tobytes())
    return out


def parse_record(raw):
    """a raw record as oracle/py_bam.py's record dict (what its parse_bam makes of the same bytes in a file)"""
    bs = struct.unpack_from("<I", raw, 0)[0]
    tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHIiii", raw, 4)
    p = 36
    name = raw[p : p + l_name]
    p += l_name
    cigar = [(c & 15, c >> 4) for c in struct.unpack_from("<%dI" % n_cig, raw, p)]
    p += 4 * n_cig
    seq4 = raw[p : p + (l_seq + 1) // 2]
    p += (l_seq + 1) // 2
    qual = raw[p : p + l_seq]
    p += l_seq
    return dict(tid=tid, pos=pos, name=name, mapq=mapq, cigar=cigar, flag=flag, l_seq=l_seq, mtid=mtid, mpos=mpos, tlen=tlen, seq4=seq4, qual=qual,
                aux=raw[p : 4 + bs])


def write_bam_raw(path, raws, refs=REFS, block=0xFF00):
    """a BAM file of raw records, in the order given"""
    text = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)).encode()
    data = bytearray(b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<i", len(refs)))
    for name, ln in refs:
        data += struct.pack("<I", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", ln)
    for r in raws:
        data += r
    with open(path, "wb") as f:
        for o in range(0, len(data), block):
            f.write(W.bgzf_block(bytes(data[o : o + block])))
        f.write(W.BGZF_EOF)


# ---- what the reference's results say a reader must hand over --------------------------------------------------------------------------
class RefSet:
    """One group with the reference's results: names, cpu_only, raws (raw records), res[setting_key] = (ALIGN_OUT[n], MISMS[], read bytes)"""

    def __init__(self, group, names, cpu_only, raws, res):
        self.group, self.names, self.cpu_only, self.raws, self.res = group, list(names), [bool(v) for v in cpu_only], list(raws), res

    def __len__(self):
        return len(self.raws)

    def misms(self, key, i):
        a, ms, _ = self.res[key]
        o, n = int(a["misms_off"][i]), int(a["n_misms"][i])
        return [[int(m["type"]), int(m["position"]), int(m["size"])] for m in ms[o : o + n]]

    def read(self, key, i):
        a, _, seq = self.res[key]
        o, n = int(a["read_off"][i]), int(a["read_len"][i])
        return seq[o : o + n].tolist()


def template_of(rs, key, i):
    """reference record i (ret = 0) as the one template a reader makes of it, in the shape tests/test_bam.py's c_blocks gives"""
    a = rs.res[key][0][i]
    ix = int(a["reverse"])
    n = int(a["read_len"])
    t = {"pos": [int(a["forward_position"]), int(a["reverse_position"])], "span": [0, 0], "reads": [None, None], "misms": [[], []], "mapq": [0, 0],
         "orientation": int(a["orientation"]), "bs_strand": int(a["bs_strand"])}
    t["span"][ix] = int(a["reference_span"]) if n else 0
    t["reads"][ix] = rs.read(key, i) if n else None
    t["misms"][ix] = rs.misms(key, i)
    t["mapq"][ix] = int(a["mapq"])
    return t


def tally(rs, key, keep):
    """the reader's fifteen filter counters and base sums over records `keep` (indices): one count and l_seq bases per record the
    reference does not use (ret = 1), under its reason"""
    a = rs.res[key][0]
    cts, bases = [0] * 15, [0] * 15
    for i in keep:
        if int(a["ret"][i]) == 1:
            cts[int(a["filtered"][i])] += 1
            bases[int(a["filtered"][i])] += struct.unpack_from("<I", rs.raws[i], 20)[0]
    return cts, bases


def file_records(rs, key):
    """indices of a file group's records that go into a file: everything but the cpu_only cases"""
    return [i for i in range(len(rs)) if not rs.cpu_only[i]]


def gpu_flag_file(rs, key):
    """(indices kept, indices left out) of the fixed group for a file a reader accepts: the records the reference filters (ret = 1)
    and those it uses with PAIRED cleared (alignment_flag); left out are the records it uses as one mate of a pair — a file of
    arbitrary lone mates is what read_input asserts on."""
    a = rs.res[key][0]
    keep, out = [], []
    for i in range(len(rs)):
        (keep if (int(a["ret"][i]) == 1 or not (int(a["alignment_flag"][i]) & 1)) else out).append(i)
    return keep, out


def sweep_share(rs, left_out):
    """(records of the flag sweep proper — every flag value with the mate right and left of it, without the edge cases beside them —
    that were left out, records of the sweep)"""
    import re

    sweep = [i for i, n in enumerate(rs.names) if re.fullmatch(r"fixed/flag \d+, mate to the (right|left)", n)]
    return len(set(sweep) & set(left_out)), len(sweep)


def flatten_blocks(blocks):
    """the templates of all blocks in file order"""
    return [t for _, _, ts in blocks for t in ts]


def live_sets(results_fn, reduced=False, only=None):
    """group -> RefSet with the reference's results from results_fn(records, offsets, keep_unmatched, ignore_dup) -> (ALIGN_OUT[n], MISMS[],
    read bytes): the file groups under the default setting, the fixed group under all four"""
    out = collections.OrderedDict()
    for name, cases in groups(reduced).items():
        if only is not None and name not in only:
            continue
        records, offsets = pack(cases)
        res = {setting_key(s): results_fn(records, offsets, s[0], s[1]) for s in (SETTINGS if name == "fixed" else SETTINGS[:1])}
        out[name] = RefSet(name, [c.name for c in cases], [c.cpu_only for c in cases], [c.raw for c in cases], res)
    return out


# ---- the recorded fixture: tests/golden/ref_align_details.json / .bin (tools/make_ref_align_vectors.py) -----------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_align_details.json")
# ALIGN_OUT (oracle/ref_loader.py) without its offsets, which are running sums, and in the narrowest types that hold the values
ALIGN_PACKED = np.dtype([("ret", "i1"), ("filtered", "u1"), ("reverse", "u1"), ("orientation", "u1"), ("mapq", "u1"), ("bs_strand", "u1"),
                         ("alignment_flag", "<u2"), ("align_length", "<u4"), ("forward_position", "<u4"), ("reverse_position", "<u4"),
                         ("reference_span", "<u4"), ("n_misms", "<u4"), ("read_len", "<u4")])
ALIGN_FIELDS = [("ret", "<i4"), ("filtered", "<u4"), ("reverse", "<u4"), ("alignment_flag", "<u4"), ("align_length", "<u4"), ("orientation", "<u4"),
                ("forward_position", "<u4"), ("reverse_position", "<u4"), ("mapq", "<u4"), ("reference_span", "<u4"), ("bs_strand", "<u4"),
                ("n_misms", "<u4"), ("misms_off", "<u8"), ("read_len", "<u4"), ("_pad", "<u4"), ("read_off", "<u8")]
MISMS_T = np.dtype([("type", "<u4"), ("position", "<u4"), ("size", "<u4")])


def pack_align(a):
    out = np.zeros(len(a), dtype=ALIGN_PACKED)
    for f in ALIGN_PACKED.names:
        out[f] = a[f]
        assert (out[f] == a[f]).all(), f
    return out


def unpack_align(p):
    out = np.zeros(len(p), dtype=np.dtype(ALIGN_FIELDS))
    for f in ALIGN_PACKED.names:
        out[f] = p[f]
    out["misms_off"] = np.concatenate([[0], np.cumsum(p["n_misms"], dtype=np.uint64)[:-1]]) if len(p) else 0
    out["read_off"] = np.concatenate([[0], np.cumsum(p["read_len"], dtype=np.uint64)[:-1]]) if len(p) else 0
    return out


def golden_sets(path=GOLDEN):
    """group -> RefSet from the recorded fixture (the reduced case set)"""
    import json

    with open(path) as f:
        G = json.load(f)
    with open(os.path.splitext(path)[0] + ".bin", "rb") as f:
        blob = f.read()

    def arr(v, dtype):
        off, nbytes = v["bin"]
        return np.frombuffer(blob[off : off + nbytes], dtype=dtype).copy()

    out = collections.OrderedDict()
    for name, g in G["sets"].items():
        raws = unpack(arr(g["records"], np.uint8), arr(g["offsets"], "<u8"))
        res = {k: (unpack_align(arr(r["align"], ALIGN_PACKED)), arr(r["misms"], MISMS_T), arr(r["reads"], np.uint8)) for k, r in g["results"].items()}
        out[name] = RefSet(name, g["names"], [i in set(g["cpu_only"]) for i in range(len(raws))], raws, res)
    return out
