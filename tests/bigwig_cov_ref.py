"""The coverage bigWig file in Python — written from the coverage rule as include/bscall_amd.h states it (value, summary, stream, pyramid,
file), not from csrc/bigwig.c, whose checker it is in tests/test_bigwig_cov_host.py and tests/test_gpu_bigwig_cov.py.  The container's parts
that do not depend on the track (chromosome tree, R-trees, windows, pyramid over exact Python integers) are tests/bigwig_ref.py's, imported.
Every float is rounded ONCE from the exact integer, in integer arithmetic: rounded(v, bits) picks the neighbour with `bits` significant bits
(ties to the even one), and only that integer — exactly representable — is handed to struct.pack.

build(refs, blocks, S, reduction): refs = [(name, length)]; blocks = [(tid, [(start, c), ...])] in the order they are added.
check_z(got, ...): the compressed file, around its own blobs, each of which must inflate to the block build() holds in its place."""
import struct
import zlib

import bigwig_ref as R
import bigwig_z_ref as Z

CAP = 2**32 - 1


def rounded(v, bits):
    """The integer with at most `bits` significant bits nearest to v >= 0; a tie goes to the one whose last kept bit is 0."""
    drop = v.bit_length() - bits
    if drop <= 0:
        return v
    below = (v >> drop) << drop
    above = below + (1 << drop)
    if 2 * v < below + above:
        return below
    if 2 * v > below + above:
        return above
    return below if (below >> drop) % 2 == 0 else above


def f32(v):
    return struct.pack("<f", float(rounded(v, 24)))  # (24 significant bits, below 2^128: the conversion and the pack are exact)


def f64(v):
    return struct.pack("<d", float(rounded(v, 53)))


def cov_of(a, b):
    return min(a + b, CAP)


def block_stream(tid, sites, S):
    """(bytes, [summary per section]) of a block's (start, c) sites."""
    out, secs = [], []
    for k in range(0, len(sites), S):
        part = sites[k : k + S]
        out.append(struct.pack("<IIIIIBBH", tid, part[0][0], part[-1][0] + 1, 0, 1, 2, 0, len(part)))
        for s, c in part:
            out.append(struct.pack("<I", s) + f32(c))
        secs.append(R.summary(part))
    return b"".join(out), secs


def sum_tuple(s):
    """A summary dict as the bsc_bw_sum fields (start, end, count, min_m, max_m, _pad, sum_m, sum_m2): the sum of squares is 96 bits."""
    assert s["sum"] < 2**64 and s["sum2"] < 2**96
    return (s["start"], s["end"], s["count"], s["min"], s["max"], s["sum2"] >> 64, s["sum"], s["sum2"] % 2**64)


def block_entries(tid, sites, S, reduction):
    """(stream bytes, [section tuples], [zoom0 tuples]): what a block call reports for the coverage track."""
    raw, secs = block_stream(tid, sites, S)
    return raw, [sum_tuple(s) for s in secs], [sum_tuple(w) for w in R.windows(sites, reduction)]


def zoom_blocks(records):
    """The raw zoom blocks of a level's [(tid, summary)]: up to 512 records, never two contigs; [(tid, start, end, bytes)]."""
    out, k = [], 0
    while k < len(records):
        j = k
        while j < len(records) and j - k < R.ZBLOCK and records[j][0] == records[k][0]:
            j += 1
        raw = b"".join(struct.pack("<IIII", tid, r["start"], r["end"], r["count"]) + f32(r["min"]) + f32(r["max"]) + f32(r["sum"]) + f32(r["sum2"])
                       for tid, r in records[k:j])
        out.append((records[k][0], records[k][1]["start"], records[j - 1][1]["end"], raw))
        k = j
    return out


def build(refs, blocks, S=1024, reduction=1024, blobs=None):
    """The plain file; with blobs = {"sections": [bytes], "zoom": [[bytes] per level]} the compressed file around those blobs."""
    tree = R.chrom_tree(refs, 296)
    data_at = 296 + len(tree)
    data, items, pos, every, largest = [], [], data_at + 8, [], 0
    for tid, sites in blocks:
        raw, secs = block_stream(tid, sites, S)
        for k, s in enumerate(secs):
            one = raw[k * (24 + 8 * S) : (k + 1) * (24 + 8 * S)]
            largest = max(largest, len(one))
            if blobs is not None:
                one = blobs["sections"][len(items)]
                items.append((tid, s["start"], tid, s["end"], pos, len(one)))
                data.append(one)
                pos += len(one)
            else:
                items.append((tid, s["start"], tid, s["end"], pos + k * (24 + 8 * S), 24 + 8 * s["count"]))
        every += secs
        if blobs is None:
            data.append(raw)
            pos += len(raw)
    index_at = pos
    tail = [R.rtree(items, index_at, index_at)]
    pos += len(tail[0])
    zoom_headers = []
    for l, (width, records) in enumerate(R.pyramid(blocks, reduction)):
        level_at, at, zitems, body = pos, pos + 4, [], [struct.pack("<I", len(records))]
        for k, (tid, start, end, raw) in enumerate(zoom_blocks(records)):
            largest = max(largest, len(raw))
            one = raw if blobs is None else blobs["zoom"][l][k]
            zitems.append((tid, start, tid, end, at, len(one)))
            body.append(one)
            at += len(one)
        body.append(R.rtree(zitems, at, at))
        zoom_headers.append(struct.pack("<IIQQ", min(width, 2**32 - 1), 0, level_at, at))
        tail.append(b"".join(body))
        pos += len(tail[-1])
    n_levels = len(zoom_headers)
    zoom_headers += [bytes(24)] * (R.LEVELS - n_levels)
    if every:
        total = (struct.pack("<Q", sum(s["count"] for s in every)) + f64(min(s["min"] for s in every)) + f64(max(s["max"] for s in every))
                 + f64(sum(s["sum"] for s in every)) + f64(sum(s["sum2"] for s in every)))
    else:
        total = bytes(40)
    header = struct.pack("<IHHQQQHHQQIQ", R.MAGIC, 4, n_levels, 296, data_at, index_at, 0, 0, 0, 256, largest if blobs is not None and every else 0, 0)
    return b"".join([header] + zoom_headers + [total, tree, struct.pack("<Q", len(items))] + data + tail + [struct.pack("<I", R.MAGIC)])


def check_z(got, refs, blocks, S=1024, reduction=1024):
    """A compressed coverage file: its blobs, taken by the R-trees' leaves, inflate (Adler-32 verified) to the blocks of the plain file, and
    the file is the layout around them.  Returns the blobs."""
    hdr = struct.unpack_from("<IHHQQQHHQQIQ", got, 0)
    assert hdr[0] == R.MAGIC and hdr[1] == 4
    levels = R.pyramid(blocks, reduction)
    assert hdr[2] == len(levels)
    raw_secs = []
    for tid, sites in blocks:
        raw, secs = block_stream(tid, sites, S)
        raw_secs += [raw[k * (24 + 8 * S) : (k + 1) * (24 + 8 * S)] for k in range(len(secs))]
    sec_leaves = Z.leaves(got, hdr[5])
    assert len(sec_leaves) == len(raw_secs)
    blobs = {"sections": [got[off : off + size] for *_, off, size in sec_leaves], "zoom": []}
    for blob, raw in zip(blobs["sections"], raw_secs):
        Z.inflate(blob, raw)
    for l, (_, records) in enumerate(levels):
        _, _, data_at, idx = struct.unpack_from("<IIQQ", got, 64 + 24 * l)
        zl, want = Z.leaves(got, idx), zoom_blocks(records)
        assert len(zl) == len(want) and struct.unpack_from("<I", got, data_at)[0] == len(records)
        blobs["zoom"].append([got[off : off + size] for *_, off, size in zl])
        for blob, (_, _, _, raw) in zip(blobs["zoom"][-1], want):
            Z.inflate(blob, raw)
    want = build(refs, blocks, S, reduction, blobs)
    assert len(got) == len(want)
    assert got == want, "the file is not the layout around its blobs"
    return blobs


def z_sections(raw, S, level=1):
    """(zdata, z_sizes) of a block's plain stream: every section through zlib.compress."""
    parts = [zlib.compress(raw[k : k + 24 + 8 * S], level) for k in range(0, len(raw), 24 + 8 * S)]
    return b"".join(parts), [len(p) for p in parts]
