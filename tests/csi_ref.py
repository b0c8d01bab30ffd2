"""The CSI index of a BGZF-compressed BCF / VCF file, built in plain Python from the file alone — the checker of bsc_csi_* and of
bam2bcf --index, written from the CSIv1 layout and the rule of include/bscall_amd.h, not from the library's code:

  walk the file member by member (each one's file offset and inflated bytes), parse every record of the inflated stream with the
  virtual offset of its first byte and of the byte behind it, and build: header "CSI\\1", min_shift, depth, l_aux, aux, n_ref; per
  contig the leaf bins that hold records, ascending (bin = ((1 << 3 depth) - 1) / 7 + (pos0 >> min_shift), loffset = the chunk's
  begin, one chunk [first record's start, last record's end]), then the pseudo-bin ((1 << 3 (depth + 1)) - 1) / 7 + 1 with loffset
  0 and the chunks (contig's first record, behind its last) and (records, 0); a contig without records n_bin = 0; n_no_coor 0.

A virtual offset is (file offset of the member that holds the byte) << 16 | (offset inside the member's inflated bytes): class Voff.
"""
import re
import struct
import zlib


def members(blob):
    """[(file offset, inflated bytes)] of every member, the end-of-file marker included."""
    out, at = [], 0
    while at < len(blob):
        assert blob[at : at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12 : at + 14] == b"BC", at
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        data = zlib.decompress(blob[at + 18 : at + bsize - 8], -15)
        assert struct.unpack_from("<I", blob, at + bsize - 4)[0] == len(data)
        out.append((at, data))
        at += bsize
    assert at == len(blob)
    return out


def inflate(blob):
    return b"".join(d for _, d in members(blob))


class Voff:
    """u, an offset into the inflated stream -> the virtual offset.  The writers cut a member every 0xFF00 bytes (checked here against the
    file), so member u // 0xFF00 holds byte u; an offset at such a boundary is the first byte of the NEXT member — behind the last
    full member that is the end-of-file marker —, the end of a short last member stays inside it."""

    def __init__(self, blob):
        ms = members(blob)
        assert ms and ms[-1][1] == b"" and all(len(d) == 0xFF00 for _, d in ms[:-2]) and (len(ms) < 2 or 0 < len(ms[-2][1]) <= 0xFF00)
        self.coff = [c for c, _ in ms]
        self.data = b"".join(d for _, d in ms)

    def __call__(self, u):
        assert 0 <= u <= len(self.data)
        return self.coff[u // 0xFF00] << 16 | (u % 0xFF00)


def records(data):
    """(format, contig names, lengths, [(tid, pos0, u_beg, u_end)]) of an inflated BCF or VCF text file."""
    recs = []
    if data[:5] == b"BCF\x02\x02":
        (l_text,) = struct.unpack_from("<I", data, 5)
        text = data[9 : 9 + l_text].decode()
        ctg = re.findall(r"^##contig=<ID=([^,>]+),length=(\d+)", text, flags=re.M)
        at = 9 + l_text
        while at < len(data):
            l_shared, l_indiv, rid, pos = struct.unpack_from("<IIii", data, at)
            end = at + 8 + l_shared + l_indiv
            recs.append((rid, pos, at, end))
            at = end
        assert at == len(data)
        return "bcf", [c[0] for c in ctg], [int(c[1]) for c in ctg], recs
    at = 0
    names, lens = [], []
    while at < len(data):
        e = data.index(b"\n", at) + 1
        line = data[at:e]
        if line[:1] == b"#":
            m = re.match(rb"##contig=<ID=([^,>]+),length=(\d+)", line)
            if m:
                names.append(m.group(1).decode())
                lens.append(int(m.group(2)))
        else:
            c = line.split(b"\t", 2)
            recs.append((names.index(c[0].decode()), int(c[1]) - 1, at, e))
        at = e
    return "vcf", names, lens, recs


def depth_of(min_shift, lens):
    d, s = 0, 1 << min_shift
    while s < max(lens, default=0) + 256:
        s <<= 3
        d += 1
    return d


def build(blob, min_shift=14):
    """The inflated bytes of the .csi file that belongs to the BGZF file `blob`."""
    v = Voff(blob)
    fmt, names, lens, recs = records(v.data)
    depth = depth_of(min_shift, lens)
    out = bytearray(b"CSI\x01" + struct.pack("<ii", min_shift, depth))
    if fmt == "vcf":
        nm = b"".join(n.encode() + b"\0" for n in names)
        out += struct.pack("<i", 28 + len(nm)) + struct.pack("<7i", 2, 1, 2, 0, ord("#"), 0, len(nm)) + nm
    else:
        out += struct.pack("<i", 0)
    out += struct.pack("<i", len(names))
    leaf0 = ((1 << (3 * depth)) - 1) // 7
    pseudo = ((1 << (3 * (depth + 1))) - 1) // 7 + 1
    for tid in range(len(names)):
        mine = [r for r in recs if r[0] == tid]
        bins = {}
        for _, pos, ub, ue in mine:
            b = bins.setdefault(leaf0 + (pos >> min_shift), [ub, ue])
            b[0], b[1] = min(b[0], ub), max(b[1], ue)
        out += struct.pack("<i", len(bins) + 1 if bins else 0)
        for k in sorted(bins):
            out += struct.pack("<IQiQQ", k, v(bins[k][0]), 1, v(bins[k][0]), v(bins[k][1]))
        if bins:
            out += struct.pack("<IQiQQQQ", pseudo, 0, 2, v(mine[0][2]), v(mine[-1][3]), len(mine), 0)
    out += struct.pack("<Q", 0)
    return bytes(out)


def parse(blob):
    """(inflated bytes, contig names, [(tid, pos0, u_beg, u_end)]) of a BGZF file, once for many linear() calls."""
    data = inflate(blob)
    _, names, _, recs = records(data)
    return data, names, recs


def linear(parsed, contig, beg, end):
    """What vcf.fetch must return: the records of `contig` (name) with beg <= pos0 < end, by a scan of the whole file."""
    data, names, recs = parsed
    if contig not in names:
        return []
    tid = names.index(contig)
    return [data[ub:ue] for t, pos, ub, ue in recs if t == tid and beg <= pos < end]


def member_sizes(blob):
    """The compressed sizes of the data members (the end-of-file marker left out), from the members' own BSIZE fields."""
    out, at = [], 0
    while at < len(blob):
        out.append(struct.unpack_from("<H", blob, at + 16)[0] + 1)
        at += out[-1]
    assert out[-1] == 28
    return out[:-1]


def sweep(names_lens, min_shift, rng, n_random=200):
    """The ranges of the fetch tests: n_random random ones and, for every window edge e of every contig, [e - 1, e), [e, e + 1),
    [e - 1, e + 1) and the window [e, next edge)."""
    out = []
    for name, ln in names_lens:
        for e in range(0, ln + (1 << min_shift), 1 << min_shift):
            out += [(name, max(e - 1, 0), e), (name, e, e + 1), (name, max(e - 1, 0), e + 1), (name, e, e + (1 << min_shift))]
    for _ in range(n_random):
        name, ln = names_lens[int(rng.integers(0, len(names_lens)))]
        a = int(rng.integers(0, ln + 10))
        out.append((name, a, a + int(rng.choice([1, 2, 50, 1000, 1 << min_shift, ln]))))
    return [(n, a, b) for n, a, b in out if a < b]


def entries_of(stream, fmt, min_shift, sync=None):
    """The Python walk the device scan is compared with: [(window, n_records, u_beg)] of a block's stream, runs cut where the window
    changes and at every offset of `sync` (the interval boundaries)."""
    pos_at = []
    at = 0
    while at < len(stream):
        if fmt == "bcf":
            l_shared, l_indiv, _, pos = struct.unpack_from("<IIii", stream, at)
            nxt = at + 8 + l_shared + l_indiv
        else:
            nxt = stream.index(b"\n", at) + 1
            pos = int(stream[at:nxt].split(b"\t", 2)[1]) - 1
        pos_at.append((at, pos))
        at = nxt
    cuts = set(sync or [])
    out = []
    for at, pos in pos_at:
        w = pos >> min_shift
        if out and out[-1][0] == w and at not in cuts:
            out[-1][1] += 1
        else:
            out.append([w, 1, at])
    return [tuple(e) for e in out]


def merged(entries):
    """Adjacent entries with one window become one (what bsc_csi_add does with them)."""
    out = []
    for w, n, u in entries:
        if out and out[-1][0] == w:
            out[-1][1] += n
        else:
            out.append([w, n, u])
    return [tuple(e) for e in out]
