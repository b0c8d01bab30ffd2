"""The methylation bigWig track and the coverage track beside it (include/bscall_amd.h has the rules and the file's layout; track="level" or
"coverage" throughout): the Python form of the rule over packed records (sections_of_recs), the writer of the file over the C ABI (Writer: bsc_bigwig_open / _add / _finish / _close), and a reader that follows the
file's own offsets (read: header, chromosomes, total summary, zoom levels; intervals through the R-tree; zoom_records).  The bytes are
UCSC-unpinned: no UCSC or pyBigWig reader has seen them; this reader is written from the same published layout.  A file whose
uncompressBufSize is not 0 holds every section and zoom block as a zlib stream (Writer(compress=True) with add_z): the reader inflates
them, and refuses a block that inflates to more than that size."""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import _lib

BW_SUM = np.dtype([("start", "<u4"), ("end", "<u4"), ("count", "<u4"), ("min_m", "<u4"), ("max_m", "<u4"), ("_pad", "<u4"), ("sum_m", "<u8"),
                   ("sum_m2", "<u8")])
MAGIC, CHROM_MAGIC, RTREE_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
_METH = {"contexts": 0, "min_cov": 1, "min_phred": 0, "pass_only": 0}


def _as_dict(p, default):
    if p is None:
        return dict(default)
    if isinstance(p, dict):
        return dict(default, **p)
    return {k: int(getattr(p, k)) for k in default}


def value_bytes(m):
    """The four bytes written for m tenths of a percent: (float)(m / 10.0)."""
    return struct.pack("<f", m / 10.0)


TRACKS = {"level": _lib.BW_LEVEL, "coverage": _lib.BW_COVERAGE}


def int_float_bits(v, mant, bias):
    """The bits of the non-negative integer v as a binary float of `mant` significand bits, rounded once, to nearest, ties to even, in
    integer arithmetic (v below the format's range)."""
    if not v:
        return 0
    top = v.bit_length() - 1
    if top < mant:
        q = v << (mant - 1 - top)
    else:
        sh = top - (mant - 1)
        q, rem, half = v >> sh, v & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
        if q >> mant:
            q, top = q >> 1, top + 1
    return ((top + bias) << (mant - 1)) | (q & ((1 << (mant - 1)) - 1))


def cov_value_bytes(c):
    """The four bytes written for a coverage c (0 .. 2^32 - 1): the unsigned integer as binary32, rounded once to nearest even."""
    return struct.pack("<I", int_float_bits(int(c), 24, 127))


def site_of_rec(rec, meth_params=None, track="level"):
    """None, or (start, m) of the site a packed record (a VCF_REC element) gives: the per-cytosine rule, start = pos - 1,
    m = (2000 a + (a + b)) / (2 (a + b)); track="coverage": (start, c), c = min(a + b, 2^32 - 1)."""
    p = _as_dict(meth_params, _METH)
    c = rec["core"]
    gt, cg = int(c["gt"]), bytes(c["cg"])
    if not int(c["emit"]) or gt not in (4, 7):
        return None
    if cg != b"C" and not (p["contexts"] == 1 and cg == b"H"):
        return None
    cnt = [int(v) for v in rec["counts"]]
    a, b = (cnt[5], cnt[7]) if gt == 4 else (cnt[6], cnt[4])
    if a + b < max(1, p["min_cov"]) or int(c["phred"]) < p["min_phred"] or (p["pass_only"] and int(c["flt"])):
        return None
    if TRACKS[track] == _lib.BW_COVERAGE:
        return ((int(c["pos"]) - 1) & 0xFFFFFFFF, min(a + b, 0xFFFFFFFF))
    return ((int(c["pos"]) - 1) & 0xFFFFFFFF, (2000 * a + (a + b)) // (2 * (a + b)))


def summary_of(sites):
    """The bsc_bw_sum of a run of (start, m) sites — or (start, c) sites: the sum of squares is 96 bits, its top 32 in _pad —, as a tuple in
    BW_SUM's field order."""
    ms = [m for _, m in sites]
    sq = sum(m * m for m in ms)
    return (sites[0][0], sites[-1][0] + 1, len(sites), min(ms), max(ms), sq >> 64, sum(ms), sq & 0xFFFFFFFFFFFFFFFF)


def sections_of_sites(sites, chrom_id, items_per_section=1024, reduction=1024, track="level"):
    """A block's (start, m) sites in order -> (the data stream's bytes, sections, zoom0): the two summaries as BW_SUM arrays.
    track="coverage": (start, c) sites."""
    S, out, secs, zoom = int(items_per_section), [], [], []
    vb = cov_value_bytes if TRACKS[track] == _lib.BW_COVERAGE else value_bytes
    for k in range(0, len(sites), S):
        part = sites[k : k + S]
        out.append(struct.pack("<IIIIIBBH", chrom_id, part[0][0], part[-1][0] + 1, 0, 1, 2, 0, len(part)))
        out.extend(struct.pack("<I", s) + vb(m) for s, m in part)
        secs.append(summary_of(part))
    run = []
    for s, m in sites:
        if run and run[0][0] // reduction != s // reduction:
            zoom.append(summary_of(run))
            run = []
        run.append((s, m))
    if run:
        zoom.append(summary_of(run))
    return b"".join(out), np.array(secs, dtype=BW_SUM).reshape(-1), np.array(zoom, dtype=BW_SUM).reshape(-1)


def sections_of_recs(recs, chrom_id, meth_params=None, items_per_section=1024, reduction=1024, track="level"):
    """The Python form of the rule over packed records (a VCF_REC array): (bytes, sections, zoom0)."""
    sites = [s for s in (site_of_rec(r, meth_params, track) for r in recs) if s is not None]
    return sections_of_sites(sites, chrom_id, items_per_section, reduction, track)


def sections_recs_host(recs, chrom_id, meth_params=None, bw_params=None, room=None, track="level"):
    """bsc_bigwig_sections_recs (track="coverage": bsc_bigwig_cov_sections_recs), the C host form: (bytes, sections, zoom0).  room: (bytes,
    sections, windows) to offer instead of asking first; a BscError where it is too small."""
    from .caller import _check

    L = _lib.load()
    host_form = L.bsc_bigwig_cov_sections_recs if TRACKS[track] == _lib.BW_COVERAGE else L.bsc_bigwig_sections_recs
    recs = np.ascontiguousarray(recs)
    mp = meth_params if isinstance(meth_params, _lib.MethParams) else _lib.MethParams(**(meth_params or {}))
    bp = bw_params if isinstance(bw_params, _lib.BwParams) else _lib.BwParams(**(bw_params or {}))
    nb, ns, nz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    ptr = recs.ctypes.data if len(recs) else None
    if room is None:
        rc = host_form(ptr, len(recs), chrom_id, C.byref(mp), C.byref(bp), None, 0, C.byref(nb), None, C.byref(ns), None, C.byref(nz))
        if rc == 0:  # nothing at all
            return b"", np.zeros(0, dtype=BW_SUM), np.zeros(0, dtype=BW_SUM)
        if rc != -1 or not nb.value:
            _check(rc)
        room = (nb.value, ns.value, nz.value)
    out = np.zeros(max(room[0], 1) + 8, np.uint8)
    out[room[0] :] = 0xA5
    sec, zoom = np.zeros(room[1] + 1, dtype=BW_SUM), np.zeros(room[2] + 1, dtype=BW_SUM)
    ns.value, nz.value = room[1], room[2]
    _check(host_form(ptr, len(recs), chrom_id, C.byref(mp), C.byref(bp), out.ctypes.data, room[0], C.byref(nb), sec.ctypes.data, C.byref(ns),
                     zoom.ctypes.data, C.byref(nz)))
    assert (out[room[0] :] == 0xA5).all()
    return out[: nb.value].tobytes(), sec[: ns.value].copy(), zoom[: nz.value].copy()


class Writer:
    """bsc_bigwig_open / _add / _finish / _close on a file of its own.  refs: [(name, length)] in the BAM header's order.  compress: the
    file's sections come as zlib streams through add_z (bsc_bigwig_add_z), and finish deflates the zoom blocks.  track="coverage": a coverage
    writer (bsc_bigwig_open_track)."""

    def __init__(self, path, refs, items_per_section=1024, reduction=1024, compress=False, track="level"):
        from .caller import _check

        self._check, self._L = _check, _lib.load()
        self.compress = bool(compress)
        if track not in TRACKS:
            raise ValueError("track is 'level' or 'coverage'")
        self._f = open(path, "wb")
        names = (C.c_char_p * max(len(refs), 1))(*[n.encode() if isinstance(n, str) else bytes(n) for n, _ in refs])
        lens = np.array([l for _, l in refs], dtype=np.uint32)
        bp = _lib.BwParams(items_per_section, reduction)
        self._h = C.c_void_p(None)
        try:
            _check(self._L.bsc_bigwig_open_track(self._f.fileno(), len(refs), names, lens.ctypes.data if len(refs) else None, C.byref(bp), TRACKS[track],
                                                 C.byref(self._h)))
        except Exception:
            self._f.close()
            os.remove(path)
            raise

    def add(self, tid, data, sections, zoom0):
        sections, zoom0 = np.ascontiguousarray(sections, dtype=BW_SUM), np.ascontiguousarray(zoom0, dtype=BW_SUM)
        buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        self._check(self._L.bsc_bigwig_add(self._h, tid, buf.ctypes.data if len(data) else None, len(data), sections.ctypes.data if len(sections) else None,
                                           len(sections), zoom0.ctypes.data if len(zoom0) else None, len(zoom0)))

    def add_z(self, tid, zdata, z_sizes, sections, zoom0):
        """A block's sections as zlib streams back to back (zdata) with their lengths (z_sizes, uint32)."""
        sections, zoom0 = np.ascontiguousarray(sections, dtype=BW_SUM), np.ascontiguousarray(zoom0, dtype=BW_SUM)
        z_sizes = np.ascontiguousarray(z_sizes, dtype=np.uint32)
        if len(z_sizes) != len(sections):
            raise ValueError("one size per section")
        buf = np.frombuffer(zdata, dtype=np.uint8) if len(zdata) else np.zeros(1, np.uint8)
        self._check(self._L.bsc_bigwig_add_z(self._h, tid, buf.ctypes.data if len(zdata) else None, len(zdata), z_sizes.ctypes.data if len(z_sizes) else None,
                                             sections.ctypes.data if len(sections) else None, len(sections), zoom0.ctypes.data if len(zoom0) else None,
                                             len(zoom0)))

    def finish(self):
        self._check(self._L.bsc_bigwig_finish(self._h))

    def close(self):
        if self._h:
            self._L.bsc_bigwig_close(self._h)
            self._h = C.c_void_p(None)
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BigWig:
    """A file read back by its own offsets.  header: the 64-byte header's fields; chroms: name -> (chromId, size), found by walking the B+
    tree; summary: the total summary; zooms: [(reductionLevel, dataOffset, indexOffset)]."""

    FILE_MAGIC = MAGIC  # (bigbed.BigBed reads the same container under its own magic)

    def __init__(self, raw):
        self.raw = raw
        h = struct.unpack_from("<IHHQQQHHQQIQ", raw, 0)
        keys = ("magic", "version", "zoomLevels", "chromosomeTreeOffset", "fullDataOffset", "fullIndexOffset", "fieldCount", "definedFieldCount",
                "autoSqlOffset", "totalSummaryOffset", "uncompressBufSize", "extensionOffset")
        self.header = dict(zip(keys, h))
        if self.header["magic"] != self.FILE_MAGIC or struct.unpack_from("<I", raw, len(raw) - 4)[0] != self.FILE_MAGIC:
            raise ValueError("not a %s file" % type(self).__name__)
        self.zooms = []
        for l in range(self.header["zoomLevels"]):
            red, _, d, i = struct.unpack_from("<IIQQ", raw, 64 + 24 * l)
            self.zooms.append((red, d, i))
        s = struct.unpack_from("<Qdddd", raw, self.header["totalSummaryOffset"])
        self.summary = dict(zip(("basesCovered", "minVal", "maxVal", "sumData", "sumSquares"), s))
        self.section_count = struct.unpack_from("<Q", raw, self.header["fullDataOffset"])[0]
        self.chroms = {}
        at = self.header["chromosomeTreeOffset"]
        magic, _, self._key, val, self.chrom_count, _ = struct.unpack_from("<IIIIQQ", raw, at)
        if magic != CHROM_MAGIC or val != 8:
            raise ValueError("bad chromosome tree")
        self._chrom_walk(at + 32)
        self.ids = {v[0]: k for k, v in self.chroms.items()}

    def _chrom_walk(self, at):
        leaf, _, count = struct.unpack_from("<BBH", self.raw, at)
        for k in range(count):
            o = at + 4 + k * (self._key + 8)
            key = self.raw[o : o + self._key].rstrip(b"\0").decode()
            if leaf:
                self.chroms[key] = struct.unpack_from("<II", self.raw, o + self._key)
            else:
                self._chrom_walk(struct.unpack_from("<Q", self.raw, o + self._key)[0])

    def chrom_lookup(self, name):
        """(chromId, size) found as a reader searches the tree: by key comparison from the root; None where the name is not there."""
        key = name.encode().ljust(self._key, b"\0")
        at = self.header["chromosomeTreeOffset"] + 32
        while True:
            leaf, _, count = struct.unpack_from("<BBH", self.raw, at)
            step = self._key + 8
            items = [self.raw[at + 4 + k * step : at + 4 + k * step + self._key] for k in range(count)]
            if leaf:
                for k, it in enumerate(items):
                    if it == key:
                        return struct.unpack_from("<II", self.raw, at + 4 + k * step + self._key)
                return None
            pick = 0
            for k, it in enumerate(items):
                if it <= key:
                    pick = k
            at = struct.unpack_from("<Q", self.raw, at + 4 + pick * step + self._key)[0]

    def _block(self, off, size):
        """The raw bytes of the section or zoom block a leaf item names: as they lie in a plain file, inflated in a compressed one."""
        blob = self.raw[off : off + size]
        room = self.header["uncompressBufSize"]
        if not room:
            return blob
        d = zlib.decompressobj()
        out = d.decompress(blob, room + 1)
        if len(out) > room or d.unconsumed_tail:
            raise ValueError("a block inflates to more than uncompressBufSize = %d bytes" % room)
        if not d.eof or d.unused_data:
            raise ValueError("a block is not one whole zlib stream")
        return out

    def _rtree_hits(self, index_at, cid, start, end):
        """(dataOffset, dataSize) of the leaf items that overlap [start, end) on chromosome cid (cid None: of all leaf items)."""
        magic, _, n_items = struct.unpack_from("<IIQ", self.raw, index_at)
        if magic != RTREE_MAGIC:
            raise ValueError("bad R-tree")
        out, todo = [], [index_at + 48]
        while todo:
            at = todo.pop()
            leaf, _, count = struct.unpack_from("<BBH", self.raw, at)
            for k in range(count):
                o = at + 4 + k * (32 if leaf else 24)
                c0, s0, c1, e1 = struct.unpack_from("<IIII", self.raw, o)
                if cid is None or ((c0, s0) < (cid, end) and (cid, start) < (c1, e1)):
                    if leaf:
                        out.append(struct.unpack_from("<QQ", self.raw, o + 16))
                    else:
                        todo.append(struct.unpack_from("<Q", self.raw, o + 16)[0])
        return sorted(out)

    def intervals(self, chrom, start=0, end=None):
        """[(start, end, value)] of the sites of `chrom` inside [start, end), through the R-tree."""
        if chrom not in self.chroms:
            return []
        cid, size = self.chroms[chrom]
        end = size if end is None else end
        out = []
        for off, size_ in self._rtree_hits(self.header["fullIndexOffset"], cid, start, end):
            sec = self._block(off, size_)
            c, _s, _e, _step, span, typ, _, count = struct.unpack_from("<IIIIIBBH", sec, 0)
            assert typ == 2 and c == cid and len(sec) == 24 + 8 * count
            for k in range(count):
                s, v = struct.unpack_from("<If", sec, 24 + 8 * k)
                if start <= s < end:
                    out.append((s, s + span, v))
        return out

    def zoom_records(self, level, chrom=None, start=0, end=None):
        """The records of a zoom level as dicts {chromId, start, end, validCount, minVal, maxVal, sumData, sumSquares}; with `chrom`, those
        that overlap [start, end) there, through the level's R-tree."""
        _, data_at, index_at = self.zooms[level]
        n = struct.unpack_from("<I", self.raw, data_at)[0]
        keys = ("chromId", "start", "end", "validCount", "minVal", "maxVal", "sumData", "sumSquares")
        if chrom is None:
            if not self.header["uncompressBufSize"]:
                return [dict(zip(keys, struct.unpack_from("<IIIIffff", self.raw, data_at + 4 + 32 * k))) for k in range(n)]
            out = []
            for off, size_ in self._rtree_hits(index_at, None, 0, 0):  # (sorted by offset: the records' order)
                blk = self._block(off, size_)
                out.extend(dict(zip(keys, struct.unpack_from("<IIIIffff", blk, 32 * k))) for k in range(len(blk) // 32))
            if len(out) != n:
                raise ValueError("zoom level %d: %d records in its blocks, recordCount %d" % (level, len(out), n))
            return out
        if chrom not in self.chroms:
            return []
        cid, size = self.chroms[chrom]
        end = size if end is None else end
        out = []
        for off, size_ in self._rtree_hits(index_at, cid, start, end):
            blk = self._block(off, size_)
            for k in range(len(blk) // 32):
                r = dict(zip(keys, struct.unpack_from("<IIIIffff", blk, 32 * k)))
                if r["chromId"] == cid and r["start"] < end and start < r["end"]:
                    out.append(r)
        return out


def read(path):
    with open(path, "rb") as f:
        return BigWig(f.read())
