"""The bedMethyl table as bigBed items (include/bscall_amd.h has the rule): the Python form of the rule over packed records
(blocks_of_recs), the C host form (blocks_recs_host: bsc_bigbed_blocks_recs), the way back from a stream of items to the table's lines
(lines_of_stream), the writer of the file over the C ABI (Writer: bsc_bigbed_open / _add / _add_z / _finish / _close) and a reader that
follows the file's own offsets (read: header, autoSql, chromosomes, total summary, zoom levels; entries through the R-tree, inflating where
uncompressBufSize is not 0; lines: the table's text back).  The bytes are UCSC-unpinned: no UCSC reader has seen them."""
import ctypes as C
import os
import struct

import numpy as np

from . import _lib
from .abi import BB_ITEM_MAX as ITEM_MAX, BB_ITEM_MIN as ITEM_MIN, BB_SUM  # noqa: F401
from .bigwig import BigWig

Z_ITEMS_MAX = 0xFF00 // ITEM_MAX  # the most items a block of a compressed file may hold
_METH = {"contexts": 0, "min_cov": 1, "min_phred": 0, "pass_only": 0}
_RGB = ("0,255,0", "55,255,0", "105,255,0", "155,255,0", "205,255,0", "255,255,0", "255,205,0", "255,155,0", "255,105,0", "255,55,0", "255,0,0")


def _as_dict(p, default):
    if p is None:
        return dict(default)
    if isinstance(p, dict):
        return dict(default, **p)
    return {k: int(getattr(p, k)) for k in default}


def item_of_rec(rec, chrom_id, meth_params=None):
    """None, or (start, item bytes) of the site a packed record (a VCF_REC element) gives: the per-cytosine rule, then the 12-byte head,
    columns 4 .. 15 of the bedMethyl line and a NUL."""
    p = _as_dict(meth_params, _METH)
    c = rec["core"]
    gt, cg = int(c["gt"]), bytes(c["cg"])
    if not int(c["emit"]) or gt not in (4, 7):
        return None
    if cg != b"C" and not (p["contexts"] == 1 and cg == b"H"):
        return None
    cnt = [int(v) for v in rec["counts"]]
    a, b = (cnt[5], cnt[7]) if gt == 4 else (cnt[6], cnt[4])
    phred, flt, pos = int(c["phred"]), int(c["flt"]), int(c["pos"])
    if a + b < max(1, p["min_cov"]) or phred < p["min_phred"] or (p["pass_only"] and flt):
        return None
    start, cov = (pos - 1) & 0xFFFFFFFF, a + b
    pct = (200 * a + cov) // (2 * cov)
    if cg == b"C":
        name = "CG"
    else:
        cx = bytes(c["cx_gt"]).ljust(5, b"\0")  # numpy strips trailing NULs of an S5
        n2 = cx[0:1] if gt == 7 else cx[4:5]
        name = "CHG" if n2 == (b"C" if gt == 7 else b"G") else ("CHH" if n2 in (b"A", b"C", b"G", b"T") else "CHN")
    cols = [name, str(min(cov, 1000)), "-" if gt == 7 else "+", str(start), str(pos), _RGB[pct // 10], str(cov), str(pct), str(a), str(b), str(phred),
            "PASS" if flt == 0 else ("mac1" if flt & 128 else "fail")]
    return start, struct.pack("<III", chrom_id, start, pos) + "\t".join(cols).encode() + b"\0"


def blocks_of_items(items, items_per_block=512, reduction=1024):
    """A call's (start, item bytes) in order -> (the stream's bytes, blocks, zoom0): the two summaries as BB_SUM arrays."""
    B, out, blocks, zoom, at = int(items_per_block), [], [], [], 0
    for k in range(0, len(items), B):
        part = items[k : k + B]
        blocks.append((part[0][0], part[-1][0] + 1, len(part), 0, at))
        at += sum(len(it) for _, it in part)
        out.extend(it for _, it in part)
    for s, _ in items:
        if zoom and zoom[-1][0] // reduction == s // reduction:
            zoom[-1] = (zoom[-1][0], s + 1, zoom[-1][2] + 1, 0, 0)
        else:
            zoom.append((s, s + 1, 1, 0, 0))
    return b"".join(out), np.array(blocks, dtype=BB_SUM).reshape(-1), np.array(zoom, dtype=BB_SUM).reshape(-1)


def blocks_of_recs(recs, chrom_id, meth_params=None, items_per_block=512, reduction=1024):
    """The Python form of the rule over packed records (a VCF_REC array): (bytes, blocks, zoom0)."""
    items = [it for it in (item_of_rec(r, chrom_id, meth_params) for r in recs) if it is not None]
    return blocks_of_items(items, items_per_block, reduction)


def items_of_stream(data):
    """The stream's items as (chromId, start, end, text bytes without the NUL); a ValueError where the stream is not whole items."""
    out, at = [], 0
    while at < len(data):
        end = data.find(b"\0", at + 12)
        if end < 0:
            raise ValueError("an item without its NUL at byte %d" % at)
        out.append(struct.unpack_from("<III", data, at) + (data[at + 12 : end],))
        at = end + 1
    return out


def lines_of_stream(data, contigs):
    """The table's lines back from a stream of items: contigs[chromId] "\\t" start "\\t" end "\\t" + the item's text + "\\n"."""
    return b"".join(b"%s\t%d\t%d\t%s\n" % (contigs[cid], s, e, text) for cid, s, e, text in items_of_stream(data))


def blocks_recs_host(recs, chrom_id, meth_params=None, bb_params=None, room=None):
    """bsc_bigbed_blocks_recs, the C host form: (bytes, blocks, zoom0).  room: (bytes, blocks, windows) to offer instead of asking first; a
    BscError where it is too small."""
    from .caller import _check

    L = _lib.load()
    recs = np.ascontiguousarray(recs)
    mp = meth_params if isinstance(meth_params, _lib.MethParams) else _lib.MethParams(**(meth_params or {}))
    bp = bb_params if isinstance(bb_params, _lib.BbParams) else _lib.BbParams(**(bb_params or {}))
    nb, nk, nz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    ptr = recs.ctypes.data if len(recs) else None
    if room is None:
        rc = L.bsc_bigbed_blocks_recs(ptr, len(recs), chrom_id, C.byref(mp), C.byref(bp), None, 0, C.byref(nb), None, C.byref(nk), None, C.byref(nz))
        if rc == 0:  # nothing at all
            return b"", np.zeros(0, dtype=BB_SUM), np.zeros(0, dtype=BB_SUM)
        if rc != -1 or not nb.value:
            _check(rc)
        room = (nb.value, nk.value, nz.value)
    out = np.zeros(max(room[0], 1) + 8, np.uint8)
    out[room[0] :] = 0xA5
    blk, zoom = np.zeros(room[1] + 1, dtype=BB_SUM), np.zeros(room[2] + 1, dtype=BB_SUM)
    blk[room[1] :], zoom[room[2] :] = (0xA5A5A5A5,) * 5, (0xA5A5A5A5,) * 5
    nk.value, nz.value = room[1], room[2]
    rc = L.bsc_bigbed_blocks_recs(ptr, len(recs), chrom_id, C.byref(mp), C.byref(bp), out.ctypes.data, room[0], C.byref(nb), blk.ctypes.data,
                                  C.byref(nk), zoom.ctypes.data, C.byref(nz))
    assert (out[room[0] :] == 0xA5).all() and blk[room[1]]["off"] == 0xA5A5A5A5 and zoom[room[2]]["off"] == 0xA5A5A5A5
    if rc:
        assert not out[: room[0]].any() and not blk[: room[1]]["end"].any() and not zoom[: room[2]]["end"].any(), "written into a room too small"
        _check(rc)
    return out[: nb.value].tobytes(), blk[: nk.value].copy(), zoom[: nz.value].copy()


class Writer:
    """bsc_bigbed_open / _add / _add_z / _finish / _close on a file of its own.  refs: [(name, length)] in the BAM header's order.  compress:
    the file's blocks come as zlib streams through add_z, and finish deflates the zoom blocks."""

    def __init__(self, path, refs, items_per_block=512, reduction=1024, compress=False):
        from .caller import _check

        self._check, self._L = _check, _lib.load()
        self.compress = bool(compress)
        self._f = open(path, "wb")
        names = (C.c_char_p * max(len(refs), 1))(*[n.encode() if isinstance(n, str) else bytes(n) for n, _ in refs])
        lens = np.array([l for _, l in refs], dtype=np.uint32)
        bp = _lib.BbParams(items_per_block, reduction)
        self._h = C.c_void_p(None)
        try:
            _check(self._L.bsc_bigbed_open(self._f.fileno(), len(refs), names, lens.ctypes.data if len(refs) else None, C.byref(bp), C.byref(self._h)))
        except Exception:
            self._f.close()
            os.remove(path)
            raise

    def add(self, tid, data, blocks, zoom0):
        blocks, zoom0 = np.ascontiguousarray(blocks, dtype=BB_SUM), np.ascontiguousarray(zoom0, dtype=BB_SUM)
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        self._check(self._L.bsc_bigbed_add(self._h, tid, buf.ctypes.data if len(data) else None, len(data), blocks.ctypes.data if len(blocks) else None,
                                           len(blocks), zoom0.ctypes.data if len(zoom0) else None, len(zoom0)))

    def add_z(self, tid, zdata, z_sizes, raw_bytes, blocks, zoom0):
        """A call's blocks as zlib streams back to back (zdata) with their lengths (z_sizes, uint32); raw_bytes: the plain stream's length."""
        blocks, zoom0 = np.ascontiguousarray(blocks, dtype=BB_SUM), np.ascontiguousarray(zoom0, dtype=BB_SUM)
        z_sizes = np.ascontiguousarray(z_sizes, dtype=np.uint32)
        if len(z_sizes) != len(blocks):
            raise ValueError("one size per block")
        buf = np.frombuffer(zdata, dtype=np.uint8) if len(zdata) else np.zeros(1, np.uint8)
        self._check(self._L.bsc_bigbed_add_z(self._h, tid, buf.ctypes.data if len(zdata) else None, len(zdata), z_sizes.ctypes.data if len(z_sizes) else None,
                                             raw_bytes, blocks.ctypes.data if len(blocks) else None, len(blocks), zoom0.ctypes.data if len(zoom0) else None,
                                             len(zoom0)))

    def finish(self):
        self._check(self._L.bsc_bigbed_finish(self._h))

    def close(self):
        if self._h:
            self._L.bsc_bigbed_close(self._h)
            self._h = C.c_void_p(None)
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


MAGIC = 0x8789F2EB


class BigBed(BigWig):
    """A .bb file read back by its own offsets: the container is bigwig.BigWig's (header, chromosome tree, R-trees, zoom levels, inflation
    under uncompressBufSize); item_count is the u64 fullDataOffset names, autosql the NUL-terminated text autoSqlOffset names."""

    FILE_MAGIC = MAGIC

    def __init__(self, raw):
        super().__init__(raw)
        self.item_count = self.section_count
        at = self.header["autoSqlOffset"]
        self.autosql = raw[at : raw.index(b"\0", at)].decode() if at else ""
        self.items_per_slot = struct.unpack_from("<I", raw, self.header["fullIndexOffset"] + 40)[0]

    def entries(self, chrom, start=0, end=None):
        """[(start, end, rest)] of the items of `chrom` that overlap [start, end), through the R-tree; rest: columns 4 .. 15 as bytes."""
        if chrom not in self.chroms:
            return []
        cid, size = self.chroms[chrom]
        end = size if end is None else end
        out = []
        for off, size_ in self._rtree_hits(self.header["fullIndexOffset"], cid, start, end):
            for c, s, e, text in items_of_stream(self._block(off, size_)):
                if c == cid and s < end and start < e:
                    out.append((s, e, text))
        return out

    def all_items(self):
        """Every item in file order, block by block through the R-tree's leaves: (chromId, start, end, rest)."""
        out = []
        for off, size_ in self._rtree_hits(self.header["fullIndexOffset"], None, 0, 0):
            out.extend(items_of_stream(self._block(off, size_)))
        return out

    def lines(self):
        """The table's text back: contig TAB start TAB end TAB rest NEWLINE per item."""
        return b"".join(b"%s\t%d\t%d\t%s\n" % (self.ids[c].encode(), s, e, text) for c, s, e, text in self.all_items())


def read(path):
    with open(path, "rb") as f:
        return BigBed(f.read())


def lines(path):
    """The bedMethyl table a .bb file holds, plain or compressed."""
    return read(path).lines()
