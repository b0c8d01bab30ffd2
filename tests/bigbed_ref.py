"""The whole bedMethyl bigBed file in Python — written from the FILE and COMPRESSED FILE rules as include/bscall_amd.h states them (header,
autoSql text, chromosome B+ tree, item count, blocks, R-tree with itemsPerSlot = B, the pyramid of counts, zoom blocks), not from
csrc/bigbed.c, whose checker it is in tests/test_bigbed_host.py and tests/test_gpu_bigbed.py.  The chromosome tree is the bigWig file's
(tests/bigwig_ref.py: the same layout by the same rule).  This file carries its own copy of the autoSql text.

build(refs, adds, B, reduction, compress): refs = [(name, length)] in the BAM header's order; adds = [(tid, [(start, item bytes), ...])] in
the order they are added — the cuts matter: a block never spans two adds.  compress: None for a plain file, else a function bytes -> zlib
stream for the data blocks (the zoom blocks are zlib.compress at the default level)."""
import struct
import zlib

from bigwig_ref import LEVELS, NODE, ZBLOCK, chrom_tree, chunks

MAGIC = 0x8789F2EB
AUTOSQL = b"""table bedMethyl
"Methylation level per cytosine"
(
string chrom; "Reference sequence"
uint chromStart; "Start, 0-based"
uint chromEnd; "End"
string name; "Context: CG, CHG, CHH or CHN"
uint score; "Coverage, capped at 1000"
char[1] strand; "+ or -"
uint thickStart; "Start"
uint thickEnd; "End"
uint reserved; "Colour by level (itemRgb)"
bigint coverage; "Informative reads: non-converted + converted"
uint percent; "Methylation level, percent, rounded half up"
uint nonConverted; "Non-converted reads"
uint converted; "Converted reads"
uint gq; "Phred-scaled genotype quality"
string filter; "FILTER of the call"
)
"""


def rtree(items, at, end_off, per_slot):
    """items: [(chrom0, start, chrom1, end, offset, size)]."""
    levels = [[items[lo:hi] for lo, hi in chunks(len(items))]]
    bound = lambda node: (min((i[0], i[1]) for i in node) + max((i[2], i[3]) for i in node)) if node else (0, 0, 0, 0)
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([[bound(below[c]) + (c,) for c in range(lo, hi)] for lo, hi in chunks(len(below))])
    start, pos = {}, at + 48
    for l in range(len(levels) - 1, -1, -1):
        start[l] = []
        for node in levels[l]:
            start[l].append(pos)
            pos += 4 + (32 if l == 0 else 24) * len(node)
    out = [struct.pack("<IIQIIIIQII", 0x2468ACE0, NODE, len(items), *bound(levels[-1][0]), end_off, per_slot, 0)]
    for l in range(len(levels) - 1, -1, -1):
        for node in levels[l]:
            out.append(struct.pack("<BBH", 1 if l == 0 else 0, 0, len(node)))
            for it in node:
                out.append(struct.pack("<IIIIQQ", *it) if l == 0 else struct.pack("<IIIIQ", *it[:4], start[l - 1][it[4]]))
    return b"".join(out)


def pyramid(adds, reduction):
    """[(width, [[tid, start, end, count]])] per level: counts add, the earlier start, the later end."""
    level0 = []
    for tid, items in adds:
        for s, _ in items:
            if level0 and level0[-1][0] == tid and level0[-1][1] // reduction == s // reduction:
                level0[-1][2], level0[-1][3] = s + 1, level0[-1][3] + 1
            else:
                level0.append([tid, s, s + 1, 1])
    levels, width = [(reduction, level0)], reduction
    while len(levels) < LEVELS and len(levels[-1][1]) > 256:
        width *= 4
        nxt = []
        for tid, s, e, c in levels[-1][1]:
            if nxt and nxt[-1][0] == tid and nxt[-1][1] // width == s // width:
                nxt[-1][2], nxt[-1][3] = e, nxt[-1][3] + c
            else:
                nxt.append([tid, s, e, c])
        levels.append((width, nxt))
    return levels


def zoom_level(records, at, compressed):
    """(bytes, the R-tree's offset, the largest raw block) of a level at file offset `at`."""
    out, items, pos, biggest = [struct.pack("<I", len(records))], [], at + 4, 0
    k = 0
    while k < len(records):
        j = k
        while j < len(records) and j - k < ZBLOCK and records[j][0] == records[k][0]:
            j += 1
        raw = b"".join(struct.pack("<IIIIffff", tid, s, e, c, 1.0, 1.0, float(c), float(c)) for tid, s, e, c in records[k:j])
        biggest = max(biggest, len(raw))
        blob = zlib.compress(raw) if compressed else raw
        items.append((records[k][0], records[k][1], records[k][0], records[j - 1][2], pos, len(blob)))
        out.append(blob)
        pos += len(blob)
        k = j
    return b"".join(out) + rtree(items, pos, pos, 1), pos, biggest


def build(refs, adds, B=512, reduction=1024, compress=None):
    tree_at = 296 + len(AUTOSQL) + 1
    tree = chrom_tree(refs, tree_at)
    data_at = tree_at + len(tree)
    data, leaves, pos, n_items, biggest = [], [], data_at + 8, 0, 0
    for tid, items in adds:
        for k in range(0, len(items), B):
            part = items[k : k + B]
            raw = b"".join(it for _, it in part)
            blob = compress(raw) if compress else raw
            if compress:
                biggest = max(biggest, len(raw))
            leaves.append((tid, part[0][0], tid, part[-1][0] + 1, pos, len(blob)))
            data.append(blob)
            pos += len(blob)
            n_items += len(part)
    index_at = pos
    tail = [rtree(leaves, index_at, index_at, B)]
    pos += len(tail[0])
    zoom_headers = []
    for width, records in pyramid(adds, reduction):
        raw, idx, big = zoom_level(records, pos, compress is not None and n_items > 0)
        if compress and n_items:
            biggest = max(biggest, big)
        zoom_headers.append(struct.pack("<IIQQ", min(width, 2**32 - 1), 0, pos, idx))
        tail.append(raw)
        pos += len(raw)
    n_levels = len(zoom_headers)
    zoom_headers += [bytes(24)] * (LEVELS - n_levels)
    total = struct.pack("<Qdddd", n_items, 1.0, 1.0, float(n_items), float(n_items)) if n_items else bytes(40)
    header = struct.pack("<IHHQQQHHQQIQ", MAGIC, 4, n_levels, tree_at, data_at, index_at, 15, 9, 296, 256, biggest, 0)
    assert len(header) == 64
    return b"".join([header] + zoom_headers + [total, AUTOSQL + b"\0", tree, struct.pack("<Q", n_items)] + data + tail + [struct.pack("<I", MAGIC)])
