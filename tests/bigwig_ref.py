"""The whole methylation bigWig file in Python — written from the layout as include/bscall_amd.h states it (stream, summaries, pyramid,
header, chromosome B+ tree, R-trees, zoom blocks), not from csrc/bigwig.c, whose checker it is in tests/test_bigwig_host.py and
tests/test_gpu_bigwig.py.  Plain Python integers until struct.pack writes a float.

build(refs, blocks, S, reduction): refs = [(name, length)] in the BAM header's order; blocks = [(tid, [(start, m), ...])] in the order
they are added — the block cuts matter: a section never spans two blocks."""
import struct

MAGIC = 0x888FFC26
NODE, ZBLOCK, LEVELS = 256, 512, 8


def f32(x):
    return struct.pack("<f", x)


def summary(sites):
    """{start, end, count, min, max, sum, sum2} of a run of (start, m)."""
    ms = [m for _, m in sites]
    return dict(start=sites[0][0], end=sites[-1][0] + 1, count=len(ms), min=min(ms), max=max(ms), sum=sum(ms), sum2=sum(m * m for m in ms))


def merged(a, b):
    return dict(start=min(a["start"], b["start"]), end=max(a["end"], b["end"]), count=a["count"] + b["count"], min=min(a["min"], b["min"]),
                max=max(a["max"], b["max"]), sum=a["sum"] + b["sum"], sum2=a["sum2"] + b["sum2"])


def block_stream(tid, sites, S):
    """(bytes, [summary per section])."""
    out, secs = [], []
    for k in range(0, len(sites), S):
        part = sites[k : k + S]
        out.append(struct.pack("<IIIIIBBH", tid, part[0][0], part[-1][0] + 1, 0, 1, 2, 0, len(part)))
        for s, m in part:
            out.append(struct.pack("<I", s) + f32(m / 10.0))
        secs.append(summary(part))
    return b"".join(out), secs


def windows(sites, width):
    out = []
    for s, m in sites:
        one = summary([(s, m)])
        if out and out[-1]["start"] // width == s // width:
            out[-1] = merged(out[-1], one)
        else:
            out.append(one)
    return out


def chunks(n):
    """The item ranges of the nodes over n items; one empty node where there is none."""
    return [(lo, min(lo + NODE, n)) for lo in range(0, n, NODE)] or [(0, 0)]


def chrom_tree(refs, at):
    key = max([len(n) for n, _ in refs] + [0])
    enc = lambda n: n.encode().ljust(key, b"\0")
    order = sorted(range(len(refs)), key=lambda i: (enc(refs[i][0]), i))
    item = key + 8
    # levels bottom-up: each a list of nodes, a node a list of (key bytes, payload or child index)
    levels = [[[(enc(refs[i][0]), ("leaf", i, refs[i][1])) for i in order[lo:hi]] for lo, hi in chunks(len(order))]]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([[(below[c][0][0], ("child", c)) for c in range(lo, hi)] for lo, hi in chunks(len(below))])
    # offsets, root first
    start, pos = {}, at + 32
    for l in range(len(levels) - 1, -1, -1):
        start[l] = []
        for node in levels[l]:
            start[l].append(pos)
            pos += 4 + item * len(node)
    out = [struct.pack("<IIIIQQ", 0x78CA8C91, NODE, key, 8, len(refs), 0)]
    for l in range(len(levels) - 1, -1, -1):
        for node in levels[l]:
            out.append(struct.pack("<BBH", 1 if l == 0 else 0, 0, len(node)))
            for k, v in node:
                out.append(k + (struct.pack("<II", v[1], v[2]) if v[0] == "leaf" else struct.pack("<Q", start[l - 1][v[1]])))
    return b"".join(out)


def rtree(items, at, end_off):
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
    top = bound(levels[-1][0])
    out = [struct.pack("<IIQIIIIQII", 0x2468ACE0, NODE, len(items), *top, end_off, 1, 0)]
    for l in range(len(levels) - 1, -1, -1):
        for node in levels[l]:
            out.append(struct.pack("<BBH", 1 if l == 0 else 0, 0, len(node)))
            for it in node:
                out.append(struct.pack("<IIIIQQ", *it) if l == 0 else struct.pack("<IIIIQ", *it[:4], start[l - 1][it[4]]))
    return b"".join(out)


def pyramid(blocks, reduction):
    """[(width, [(tid, summary)])] per level."""
    level0 = []
    for tid, sites in blocks:
        for w in windows(sites, reduction):
            if level0 and level0[-1][0] == tid and level0[-1][1]["start"] // reduction == w["start"] // reduction:
                level0[-1] = (tid, merged(level0[-1][1], w))
            else:
                level0.append((tid, w))
    levels, width = [(reduction, level0)], reduction
    while len(levels) < LEVELS and len(levels[-1][1]) > 256:
        width *= 4
        nxt = []
        for tid, r in levels[-1][1]:
            if nxt and nxt[-1][0] == tid and nxt[-1][1]["start"] // width == r["start"] // width:
                nxt[-1] = (tid, merged(nxt[-1][1], r))
            else:
                nxt.append((tid, r))
        levels.append((width, nxt))
    return levels


def zoom_level(records, at):
    """(bytes, the R-tree's offset) of a level at file offset `at`."""
    out, items, pos = [struct.pack("<I", len(records))], [], at + 4
    k = 0
    while k < len(records):
        j = k
        while j < len(records) and j - k < ZBLOCK and records[j][0] == records[k][0]:
            j += 1
        items.append((records[k][0], records[k][1]["start"], records[k][0], records[j - 1][1]["end"], pos, 32 * (j - k)))
        for tid, r in records[k:j]:
            out.append(struct.pack("<IIII", tid, r["start"], r["end"], r["count"]) + f32(r["min"] / 10.0) + f32(r["max"] / 10.0) + f32(r["sum"] / 10.0)
                       + f32(r["sum2"] / 100.0))
        pos += 32 * (j - k)
        k = j
    return b"".join(out) + rtree(items, pos, pos), pos


def build(refs, blocks, S=1024, reduction=1024):
    tree = chrom_tree(refs, 296)
    data_at = 296 + len(tree)
    data, items, pos, every = [], [], data_at + 8, []
    for tid, sites in blocks:
        raw, secs = block_stream(tid, sites, S)
        for k, s in enumerate(secs):
            items.append((tid, s["start"], tid, s["end"], pos + k * (24 + 8 * S), 24 + 8 * s["count"]))
        every += secs
        data.append(raw)
        pos += len(raw)
    index_at = pos
    tail = [rtree(items, index_at, index_at)]
    pos += len(tail[0])
    zoom_headers = []
    for width, records in pyramid(blocks, reduction):
        raw, idx = zoom_level(records, pos)
        zoom_headers.append(struct.pack("<IIQQ", min(width, 2**32 - 1), 0, pos, idx))
        tail.append(raw)
        pos += len(raw)
    n_levels = len(zoom_headers)
    zoom_headers += [bytes(24)] * (LEVELS - n_levels)
    if every:
        total = struct.pack("<Qdddd", sum(s["count"] for s in every), min(s["min"] for s in every) / 10.0, max(s["max"] for s in every) / 10.0,
                            sum(s["sum"] for s in every) / 10.0, sum(s["sum2"] for s in every) / 100.0)
    else:
        total = bytes(40)
    header = struct.pack("<IHHQQQHHQQIQ", MAGIC, 4, n_levels, 296, data_at, index_at, 0, 0, 0, 256, 0, 0)
    assert len(header) == 64
    return b"".join([header] + zoom_headers + [total, tree, struct.pack("<Q", len(items))] + data + tail + [struct.pack("<I", MAGIC)])


# ---- what both test files draw their inputs from ---------------------------------------------------------------------------------------------
def records_of(pos_a_b):
    """Packed records (VCF_REC) that are CpG sites under the default parameters: [(pos, a, b)], alternating strands."""
    import numpy as np
    from bs_call_amd.abi import VCF_REC

    recs = np.zeros(len(pos_a_b), dtype=VCF_REC)
    core = recs["core"]
    core["pos"] = [p for p, _, _ in pos_a_b]
    core["emit"], core["cg"] = 1, b"C"
    core["gt"] = np.where(np.arange(len(recs)) % 2 == 0, 4, 7)
    recs["core"] = core
    for i, (_, a, b) in enumerate(pos_a_b):
        if i % 2 == 0:
            recs["counts"][i, 5], recs["counts"][i, 7] = a, b
        else:
            recs["counts"][i, 6], recs["counts"][i, 4] = a, b
    return recs


def sum_rows(arr):
    """A BW_SUM array as a list of tuples of Python integers."""
    return [tuple(int(v) for v in r) for r in arr.tolist()]
