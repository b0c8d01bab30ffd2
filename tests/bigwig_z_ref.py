"""The compressed methylation bigWig file pinned in Python, around tests/bigwig_ref.py (the plain file's builder, imported, not edited): the
section and zoom-block blobs are taken out of the file under test by its R-trees' leaves, each must inflate (zlib, Adler-32 verified) to
the bytes bigwig_ref builds for the same sites, and the whole file is rebuilt around the blobs from the layout as include/bscall_amd.h
states it — header with uncompressBufSize, trees, offsets, closing magic — and must equal the file under test byte for byte.

check(got, refs, blocks, S, reduction) -> {"sections": [blob], "zoom": [[blob] per level], "uncompress_buf_size": n}"""
import struct
import zlib

import bigwig_ref as R


def leaves(raw, index_at):
    """[(chrom0, start, chrom1, end, offset, size)] of an R-tree's leaf items in tree order (= file order here), by the child offsets."""
    magic, node, n_items = struct.unpack_from("<IIQ", raw, index_at)
    assert magic == 0x2468ACE0 and node == R.NODE

    def walk(at):
        leaf, _, count = struct.unpack_from("<BBH", raw, at)
        out = []
        for k in range(count):
            if leaf:
                out.append(struct.unpack_from("<IIIIQQ", raw, at + 4 + 32 * k))
            else:
                out += walk(struct.unpack_from("<IIIIQ", raw, at + 4 + 24 * k)[4])
        return out

    out = walk(index_at + 48)
    assert len(out) == n_items
    return out


def zoom_blocks(records):
    """The raw zoom blocks of a level's [(tid, summary)]: up to 512 records, never two contigs; [(tid, start, end, bytes)]."""
    out, k = [], 0
    while k < len(records):
        j = k
        while j < len(records) and j - k < R.ZBLOCK and records[j][0] == records[k][0]:
            j += 1
        raw = b"".join(struct.pack("<IIII", tid, r["start"], r["end"], r["count"]) + R.f32(r["min"] / 10.0) + R.f32(r["max"] / 10.0) + R.f32(r["sum"] / 10.0)
                       + R.f32(r["sum2"] / 100.0) for tid, r in records[k:j])
        out.append((records[k][0], records[k][1]["start"], records[j - 1][1]["end"], raw))
        k = j
    return out


def inflate(blob, want):
    d = zlib.decompressobj()
    out = d.decompress(blob)
    assert d.eof and not d.unused_data and out == want, "a blob does not inflate to the bytes of its block"


def check(got, refs, blocks, S=1024, reduction=1024):
    hdr = struct.unpack_from("<IHHQQQHHQQIQ", got, 0)
    assert hdr[0] == R.MAGIC and hdr[1] == 4
    n_levels, index_at = hdr[2], hdr[5]
    # what the plain file holds for the same sites
    raw_secs, every = [], []
    for tid, sites in blocks:
        raw, secs = R.block_stream(tid, sites, S)
        raw_secs += [(tid, s, raw[k * (24 + 8 * S) : (k + 1) * (24 + 8 * S)]) for k, s in enumerate(secs)]
        every += secs
    levels = R.pyramid(blocks, reduction)
    assert n_levels == len(levels)
    # the blobs, by the leaves
    sec_leaves = leaves(got, index_at)
    assert len(sec_leaves) == len(raw_secs)
    sec_blobs = [got[off : off + size] for *_, off, size in sec_leaves]
    for blob, (_, _, raw) in zip(sec_blobs, raw_secs):
        inflate(blob, raw)
    zoom_blobs = []
    for l, (_, records) in enumerate(levels):
        _, _, data_at, idx = struct.unpack_from("<IIQQ", got, 64 + 24 * l)
        zl = leaves(got, idx)
        want = zoom_blocks(records)
        assert len(zl) == len(want) and struct.unpack_from("<I", got, data_at)[0] == len(records)
        blobs = [got[off : off + size] for *_, off, size in zl]
        for blob, (_, _, _, raw) in zip(blobs, want):
            inflate(blob, raw)
        zoom_blobs.append(blobs)
    largest = max([len(r) for _, _, r in raw_secs] + [len(b[3]) for _, records in levels for b in zoom_blocks(records)] + [0])
    # the whole file around the blobs
    tree = R.chrom_tree(refs, 296)
    data_at = 296 + len(tree)
    items, pos = [], data_at + 8
    for blob, (tid, s, _) in zip(sec_blobs, raw_secs):
        items.append((tid, s["start"], tid, s["end"], pos, len(blob)))
        pos += len(blob)
    index_pos = pos
    tail = [R.rtree(items, index_pos, index_pos)]
    pos += len(tail[0])
    zoom_headers = []
    for (width, records), blobs in zip(levels, zoom_blobs):
        level_at, at, zitems, body = pos, pos + 4, [], [struct.pack("<I", len(records))]
        for blob, (tid, start, end, _) in zip(blobs, zoom_blocks(records)):
            zitems.append((tid, start, tid, end, at, len(blob)))
            body.append(blob)
            at += len(blob)
        body.append(R.rtree(zitems, at, at))
        zoom_headers.append(struct.pack("<IIQQ", min(width, 2**32 - 1), 0, level_at, at))
        tail.append(b"".join(body))
        pos += len(tail[-1])
    zoom_headers += [bytes(24)] * (R.LEVELS - len(levels))
    if every:
        total = struct.pack("<Qdddd", sum(s["count"] for s in every), min(s["min"] for s in every) / 10.0, max(s["max"] for s in every) / 10.0,
                            sum(s["sum"] for s in every) / 10.0, sum(s["sum2"] for s in every) / 100.0)
    else:
        total = bytes(40)
    header = struct.pack("<IHHQQQHHQQIQ", R.MAGIC, 4, len(levels), 296, data_at, index_pos, 0, 0, 0, 256, largest if every else 0, 0)
    want = b"".join([header] + zoom_headers + [total, tree, struct.pack("<Q", len(items))] + sec_blobs + tail + [struct.pack("<I", R.MAGIC)])
    assert len(got) == len(want)
    assert got == want, "the file is not the layout around its blobs"
    return {"sections": sec_blobs, "zoom": zoom_blobs, "uncompress_buf_size": hdr[10]}
