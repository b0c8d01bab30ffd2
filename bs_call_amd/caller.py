"""Host-side mirror of bs_call's calc API over the C ABI (include/bscall_amd.h).

`SiteCaller` plays the role of the reference's calc-thread pool: create it once (init_calc_threads +
fill_base_prob_table, src/process.c:165-166), feed it blocks of pile-ups (the call_thread loop,
src/call_genotypes.c:43-115), close it at the end (join_calc_threads).  Everything is computed by the
gfx950 kernels; nothing here computes on the CPU or uses the CPU checker.
"""
import ctypes as C

import numpy as np

from . import _lib
from .abi import GT_METH, PILEUP, SITE_STATS, TEMPLATE, VCF_CORE, VCF_REC

SYNTH_NRUNS = 1


class BscError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bscall_amd error %d: %s" % (code, msg))
        self.code = code


class BscInexactWarning(UserWarning):
    """Some pile-up sums left the range where the reference's float sums are exact (BSC_WARN_INEXACT)."""


def _check(rc):
    if rc == 1:  # BSC_WARN_INEXACT: results are written
        import warnings

        warnings.warn(_lib.load().bsc_last_error().decode("utf-8", "replace"), BscInexactWarning, stacklevel=3)
        return
    if rc != 0:
        raise BscError(rc, _lib.load().bsc_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _check_dest(name, a, nbytes):
    """A caller-supplied destination the library writes `nbytes` bytes into: the C ABI takes a bare pointer, so an
    undersized or strided array would be a host heap overflow."""
    if not isinstance(a, np.ndarray) or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
        raise ValueError("%s must be a writable C-contiguous numpy array" % name)
    if a.nbytes != nbytes:
        raise ValueError("%s has %d bytes, the call writes %d" % (name, a.nbytes, nbytes))


class DeviceBgzf:
    """BGZF on the device (bsc_bgzf_*): write host bytes (bytes-like) or device bytes (a pointer and a length), take the members
    completed so far, close for the last member and the end-of-file marker.  take() / close() return bytes."""

    def __init__(self, caller):
        self._c = caller
        self._L = caller._L
        h = C.c_void_p()
        _check(self._L.bsc_bgzf_open(caller._h, C.byref(h)))
        self._h = h

    def write(self, data):
        a = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
        _check(self._L.bsc_bgzf_write(self._h, _ptr(a), len(data)))

    def write_device(self, d_ptr, n):
        _check(self._L.bsc_bgzf_write_device(self._h, C.c_void_p(int(d_ptr)), int(n)))

    def _hand_over(self, fn, h):
        """bsc_bgzf_take / _close: the device buffer read out (bsc_detached_read) and given back to the context's pool."""
        d, n = C.c_void_p(), C.c_uint64()
        _check(fn(h, C.byref(d), C.byref(n)))
        if not d.value:
            return b""
        out = np.empty(n.value, np.uint8)
        try:
            _check(self._L.bsc_detached_read(self._c._h, d, 0, n.value, _ptr(out)))
            _check(self._L.bsc_detached_wait(self._c._h))
        finally:
            _check(self._L.bsc_detached_free(self._c._h, d))
        return out.tobytes()

    def take(self):
        return self._hand_over(self._L.bsc_bgzf_take, self._h)

    def tell(self):
        """(bytes written into the logical stream so far, members completed so far): bsc_bgzf_tell."""
        n, m = C.c_uint64(), C.c_uint64()
        _check(self._L.bsc_bgzf_tell(self._h, C.byref(n), C.byref(m)))
        return int(n.value), int(m.value)

    def close(self):
        """The last member and the end-of-file marker; the writer is gone afterwards (a second close returns b"")."""
        if self._h is None:
            return b""
        h, self._h = self._h, None
        return self._hand_over(self._L.bsc_bgzf_close, h)


CSI_BCF, CSI_VCF = 0, 1
CSI_ENTRY = np.dtype([("window", "<u4"), ("n_records", "<u4"), ("u_beg", "<u8")])  # bsc_csi_entry


class CsiIndex:
    """A CSI index made beside a compressed file (bsc_csi_*).  writer: the DeviceBgzf that writes the file — or None with header_bytes:
    the file is compressed elsewhere with members cut every 0xFF00 bytes, and members() hands their compressed sizes over.
    add() the entries of a block BEFORE its stream is written; finish() after the writer's close() returns the .csi file's bytes."""

    def __init__(self, writer, fmt, contigs, min_shift=14, header_bytes=0):
        self._L = _lib.load()
        names = (C.c_char_p * max(1, len(contigs)))(*[c[0].encode() if isinstance(c[0], str) else bytes(c[0]) for c in contigs])
        lens = (C.c_uint32 * max(1, len(contigs)))(*[int(c[1]) for c in contigs])
        h = C.c_void_p()
        if writer is None:
            _check(self._L.bsc_csi_open_detached(fmt, min_shift, len(contigs), names, lens, int(header_bytes), C.byref(h)))
        else:
            _check(self._L.bsc_csi_open(writer._h, fmt, min_shift, len(contigs), names, lens, C.byref(h)))
        self._h = h
        self.min_shift = min_shift

    def add(self, tid, entries, n_bytes):
        e = np.ascontiguousarray(entries, dtype=CSI_ENTRY)
        _check(self._L.bsc_csi_add(self._h, int(tid), _ptr(e) if len(e) else None, len(e), int(n_bytes)))

    def members(self, sizes):
        a = np.ascontiguousarray(sizes, dtype=np.uint64)
        _check(self._L.bsc_csi_members(self._h, _ptr(a) if len(a) else None, len(a)))

    def finish(self):
        need = self._L.bsc_csi_finish(self._h, None, 0)
        if need < 0:
            _check(int(need))
        out = np.empty(need, np.uint8)
        got = self._L.bsc_csi_finish(self._h, _ptr(out), need)
        if got < 0:
            _check(int(got))
        return out[:got].tobytes()

    def close(self):
        if self._h is not None:
            self._L.bsc_csi_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


TBX_TBI, TBX_CSI = 0, 1
BED_ENTRY = np.dtype([("win_beg", "<u4"), ("win_last", "<u4"), ("n_lines", "<u4"), ("zero", "<u4"), ("u_beg", "<u8")])  # bsc_bed_entry


def bed_entries_host(stream, sync=None, min_shift=14, cap_entries=None):
    """bsc_bed_entries_host, the host form of the BED index scan: (entries BED_ENTRY[], entries there are, lines, error bits) of a table's
    bytes; sync: the interval offsets (n_sync + 1 of them) or None for one interval."""
    L = _lib.load()
    data = np.frombuffer(bytes(stream), dtype=np.uint8)
    sy = None if sync is None else np.ascontiguousarray(sync, dtype=np.uint64)
    if cap_entries is None:
        cap_entries = len(data) // 6 + (0 if sy is None else len(sy)) + 2
    ent = np.zeros(max(1, cap_entries), dtype=BED_ENTRY)
    tot = np.zeros(3, dtype=np.uint64)
    _check(L.bsc_bed_entries_host(_ptr(data) if len(data) else None, len(data), None if sy is None else _ptr(sy), 0 if sy is None else max(len(sy) - 1, 0),
                                  int(min_shift), _ptr(ent) if cap_entries else None, int(cap_entries), _ptr(tot)))
    return ent[: min(int(tot[0]), cap_entries)].copy(), int(tot[0]), int(tot[1]), int(tot[2])


class TabixIndex:
    """A tabix (.tbi) or CSI (.csi) index made beside a compressed methylation table (bsc_tbx_*).  writer: the DeviceBgzf that writes the
    table — or None with header_bytes: the table is compressed elsewhere with members cut every 0xFF00 bytes, and members() hands their
    compressed sizes over.  add() the entries of a block BEFORE its table is written; finish() after the writer's close() returns the
    index file's bytes.  kind: TBX_TBI (min_shift 14) or TBX_CSI."""

    def __init__(self, writer, kind, contigs, min_shift=14, header_bytes=0):
        self._L = _lib.load()
        names = (C.c_char_p * max(1, len(contigs)))(*[c[0].encode() if isinstance(c[0], str) else bytes(c[0]) for c in contigs])
        lens = (C.c_uint32 * max(1, len(contigs)))(*[int(c[1]) for c in contigs])
        h = C.c_void_p()
        if writer is None:
            _check(self._L.bsc_tbx_open_detached(kind, min_shift, len(contigs), names, lens, int(header_bytes), C.byref(h)))
        else:
            _check(self._L.bsc_tbx_open(writer._h, kind, min_shift, len(contigs), names, lens, C.byref(h)))
        self._h = h
        self.kind, self.min_shift = kind, min_shift

    def add(self, tid, entries, n_bytes):
        e = np.ascontiguousarray(entries, dtype=BED_ENTRY)
        _check(self._L.bsc_tbx_add(self._h, int(tid), _ptr(e) if len(e) else None, len(e), int(n_bytes)))

    def members(self, sizes):
        a = np.ascontiguousarray(sizes, dtype=np.uint64)
        _check(self._L.bsc_tbx_members(self._h, _ptr(a) if len(a) else None, len(a)))

    def finish(self):
        need = self._L.bsc_tbx_finish(self._h, None, 0)
        if need < 0:
            _check(int(need))
        out = np.empty(need, np.uint8)
        got = self._L.bsc_tbx_finish(self._h, _ptr(out), need)
        if got < 0:
            _check(int(got))
        return out[:got].tobytes()

    def close(self):
        if self._h is not None:
            self._L.bsc_tbx_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SiteCaller:
    def __init__(self, under_conv=0.01, over_conv=0.05, ref_bias=2.0, min_qual=20, device=-1):
        self._L = _lib.load()
        p = _lib.Params(under_conv, over_conv, ref_bias, min_qual, device)
        self.params = {"under_conv": float(under_conv), "over_conv": float(over_conv), "ref_bias": float(ref_bias), "min_qual": int(min_qual)}
        h = C.c_void_p()
        _check(self._L.bsc_create(C.byref(p), C.byref(h)))
        self._h = h
        self._pending = None  # the submitted, not yet fetched block (block_submit / block_submit_to)

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.bsc_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- BGZF on the device ---------------------------------------------------------------------------
    def bgzf(self):
        """A DeviceBgzf writer on this context (close it before the context)."""
        return DeviceBgzf(self)

    def csi_scan_device(self, fmt, d_stream, n_bytes, d_sync, n_sync, min_shift, cap_entries=None, stream=None):
        """bsc_csi_scan_device over a stream in HBM (pointers as integers; d_sync 0 / None: one interval): (entries CSI_ENTRY[], entries
        there are, records, error bits).  cap_entries None: room for every interval and window."""
        import torch

        if cap_entries is None:
            cap_entries = int(n_sync if d_sync else 1) + (int(n_bytes) >> 5) + 2
        ent = torch.zeros(max(1, cap_entries) * 2, dtype=torch.int64, device="cuda")
        tot = torch.zeros(3, dtype=torch.int64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
        _check(self._L.bsc_csi_scan_device(self._h, fmt, C.c_void_p(int(d_stream) if d_stream else None), int(n_bytes),
                                           C.c_void_p(int(d_sync)) if d_sync else None, int(n_sync), int(min_shift), C.c_void_p(ent.data_ptr()),
                                           int(cap_entries), C.c_void_p(tot.data_ptr()), st))
        torch.cuda.synchronize()
        t = [int(v) for v in tot.cpu().numpy().view(np.uint64)]
        n = min(t[0], cap_entries)
        return ent.cpu().numpy().view(CSI_ENTRY)[:n].copy(), t[0], t[1], t[2]

    def block_csi_kept(self, min_shift=14):
        """bsc_block_csi_kept: (entries CSI_ENTRY[], records) of the stream the last *_keep call left on the device."""
        p, n, r = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(self._L.bsc_block_csi_kept(self._h, int(min_shift), C.byref(p), C.byref(n), C.byref(r)))
        if not n.value:
            return np.zeros(0, CSI_ENTRY), int(r.value)
        buf = (C.c_uint8 * (16 * n.value)).from_address(p.value)
        return np.frombuffer(buf, dtype=CSI_ENTRY).copy(), int(r.value)

    def bed_scan_device(self, d_stream, n_bytes, d_sync, n_sync, min_shift, cap_entries=None, stream=None):
        """bsc_bed_scan_device over a methylation table in HBM (pointers as integers; d_sync 0 / None: one interval): (entries BED_ENTRY[],
        entries there are, lines, error bits).  cap_entries None: room for every interval and line."""
        import torch

        if cap_entries is None:
            cap_entries = int(n_sync if d_sync else 1) + int(n_bytes) // 6 + 2
        ent = torch.zeros(max(1, cap_entries) * 3, dtype=torch.int64, device="cuda")
        tot = torch.zeros(3, dtype=torch.int64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
        _check(self._L.bsc_bed_scan_device(self._h, C.c_void_p(int(d_stream) if d_stream else None), int(n_bytes),
                                           C.c_void_p(int(d_sync)) if d_sync else None, int(n_sync), int(min_shift), C.c_void_p(ent.data_ptr()),
                                           int(cap_entries), C.c_void_p(tot.data_ptr()), st))
        torch.cuda.synchronize()
        t = [int(v) for v in tot.cpu().numpy().view(np.uint64)]
        n = min(t[0], cap_entries)
        return ent.cpu().numpy().view(BED_ENTRY)[:n].copy(), t[0], t[1], t[2]

    def block_meth_index_kept(self, min_shift=14):
        """bsc_block_meth_index_kept: (entries BED_ENTRY[], lines) of the table the last bsc_block_meth_kept / _cpg_kept call left on the
        device — block_meth_kept(...) reads the table back without detaching it, so this may follow it."""
        p, n, r = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(self._L.bsc_block_meth_index_kept(self._h, int(min_shift), C.byref(p), C.byref(n), C.byref(r)))
        if not n.value:
            return np.zeros(0, BED_ENTRY), int(r.value)
        buf = (C.c_uint8 * (24 * n.value)).from_address(p.value)
        return np.frombuffer(buf, dtype=BED_ENTRY).copy(), int(r.value)

    def bgzf_compress(self, data, pieces=None):
        """BGZF bytes of `data` (bytes-like), written whole or in the given piece lengths, with the end-of-file marker."""
        z = self.bgzf()
        parts = []
        if pieces is None:
            pieces = [len(data)]
        at = 0
        for k in pieces:
            z.write(data[at : at + k])
            at += k
            parts.append(z.take())
        if at < len(data):
            z.write(data[at:])
        parts.append(z.close())
        return b"".join(parts)

    # -- tables -----------------------------------------------------------------------------------
    def tables(self):
        q = np.zeros((44, 5), dtype=np.float64)
        lf = np.zeros(256, dtype=np.float64)
        _check(self._L.bsc_get_tables(self._h, _ptr(q), _ptr(lf)))
        return q, lf

    # -- host blocks ------------------------------------------------------------------------------
    def call_sites(self, pile, ref, out_stride=200, out=None, skip=None):
        """pile: PILEUP[n], ref: uint8[n] codes 0..4 -> (GT_METH[n] or raw uint8[n, stride], skip uint8[n]).
        `out` / `skip` may be preallocated (e.g. pinned, see pinned_empty) arrays of the right size."""
        pile = np.ascontiguousarray(pile, dtype=PILEUP)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = len(pile)
        if len(ref) != n:
            raise ValueError("pile and ref differ in length")
        if out is None:
            out = np.zeros(n, dtype=GT_METH) if out_stride == 200 else np.zeros((n, out_stride), dtype=np.uint8)
        if skip is None:
            skip = np.zeros(n, dtype=np.uint8)
        _check_dest("out", out, n * out_stride)
        _check_dest("skip", skip, n)
        _check(self._L.bsc_call_sites(self._h, _ptr(pile), _ptr(ref), n, _ptr(out), out_stride, _ptr(skip)))
        return out, skip

    # -- reads -> pile-up (HOT LOOP A) and whole blocks ------------------------------------------------
    def accumulate(self, templates, seq, x, y, out=None):
        """templates: TEMPLATE[nr]; seq: uint8 read bytes; positions x..y inclusive -> PILEUP[y-x+1].
        `out`: optional preallocated PILEUP array (reusing one avoids first-touch page faults in timing loops)."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        n = max(int(y) - int(x) + 1, 0)
        if out is None:
            out = np.zeros(max(n, 1), dtype=PILEUP)
        elif out.dtype != PILEUP or not out.flags["C_CONTIGUOUS"] or len(out) < n:
            raise ValueError("out must be a C-contiguous PILEUP array of at least y - x + 1 = %d records" % n)
        _check(self._L.bsc_accumulate(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(out)))
        return out[: max(int(y) - int(x) + 1, 0)]

    def accumulate_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_cts, stream=None):
        """HOT LOOP A on device-resident reads (raw device pointers); asynchronous — block_status() collects the verdict."""
        _check(self._L.bsc_accumulate_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_cts, stream))

    def block_status(self, stream=None):
        """Wait for `stream` and raise / warn as the block queued last deserves (invalid template, inexact sums)."""
        _check(self._L.bsc_block_status(self._h, stream))

    def last_accumulate_ms(self):
        ms = C.c_float()
        _check(self._L.bsc_last_accumulate_ms(self._h, C.byref(ms)))
        return ms.value

    def call_block(self, templates, seq, x, y, ref, out_stride=200, out=None, skip=None):
        """One call_genotypes_ML block: accumulate + call.  ref: uint8[y-x+1] codes -> (GT_METH[..], skip)."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n:
            raise ValueError("ref must have y - x + 1 entries")
        if out is None:
            out = np.zeros(n, dtype=GT_METH) if out_stride == 200 else np.zeros((n, out_stride), dtype=np.uint8)
        if skip is None:
            skip = np.zeros(n, dtype=np.uint8)
        _check_dest("out", out, n * out_stride)
        _check_dest("skip", skip, n)
        _check(self._L.bsc_call_block(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(ref),
                                      _ptr(out), out_stride, _ptr(skip)))
        return out, skip

    def block_submit(self, templates, seq, x, y, ref, out_stride=200):
        """Queue one block (accumulate + call) and return at once; the inputs may be reused immediately."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        if len(ref) != int(y) - int(x) + 1:
            raise ValueError("ref must have y - x + 1 entries")
        _check(self._L.bsc_block_submit(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(ref), out_stride))
        self._pending = (int(y) - int(x) + 1, out_stride)

    def block_submit_to(self, templates, seq, x, y, ref, out, skip):
        """block_submit with the destination named up front (pinned arrays, see PinnedBuffer): the copy-out is queued
        behind the kernels; block_fetch() then only waits, reports and returns (out, skip)."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n:
            raise ValueError("ref must have y - x + 1 entries")
        stride = out.dtype.itemsize if out.ndim == 1 else out.shape[1]
        _check_dest("out", out, n * stride)
        _check_dest("skip", skip, n)
        _check(self._L.bsc_block_submit_to(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(ref),
                                           _ptr(out), stride, _ptr(skip)))
        self._pending = (out, skip)

    def blocks_submit_to(self, blocks, ref, out_stride=200, inplace=False):
        """bsc_blocks_submit_to: blocks = [(templates, seq, x, y), ...], ref = their y - x + 3 codes each (list of arrays); the
        images of all blocks land in ONE page-locked array (block b from position offset off[b] on, a multiple of 64).  Returns
        (off, out, skip) after the fetch: out = GT_METH[P] (stride 200) or uint8[P, 208].  inplace: bsc_blocks_submit_to_inplace
        from page-locked copies of the joined inputs (no staging copy inside the library)."""
        from .abi import BLOCK_DESC

        tpls, seqs, desc, o = [], [], np.zeros(len(blocks), dtype=BLOCK_DESC), 0
        for i, (t, sq, x, y) in enumerate(blocks):
            t = np.array(t, dtype=TEMPLATE)
            sq = np.ascontiguousarray(sq, dtype=np.uint8)
            t["off"] += np.uint64(o)
            o += sq.size
            tpls.append(t)
            seqs.append(sq)
            desc[i] = (x, y, len(t), 0)
        tpl, seq = np.concatenate(tpls), np.concatenate(seqs)
        refs = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in ref]))
        P = sum(((int(y) - int(x) + 1 + 63) // 64) * 64 for _, _, x, y in blocks)
        self._pin = (PinnedBuffer(P, GT_METH) if out_stride == 200 else PinnedBuffer((P, out_stride), np.uint8), PinnedBuffer(P, np.uint8))
        out, skip = self._pin[0].array, self._pin[1].array
        off = np.zeros(len(blocks), dtype=np.uint64)
        fn = self._L.bsc_blocks_submit_to
        if inplace:
            fn = self._L.bsc_blocks_submit_to_inplace
            pins = (PinnedBuffer(len(tpl), TEMPLATE), PinnedBuffer(max(seq.size, 1), np.uint8), PinnedBuffer(max(refs.size, 1), np.uint8))
            pins[0].array[:] = tpl
            pins[1].array[: seq.size] = seq
            pins[2].array[: refs.size] = refs
            tpl, seq_a, refs = pins[0].array, pins[1].array, pins[2].array
            _check(fn(self._h, _ptr(desc), len(desc), _ptr(tpl), _ptr(seq_a), seq.size, _ptr(refs), _ptr(out), out_stride, _ptr(skip), _ptr(off)))
        else:
            _check(fn(self._h, _ptr(desc), len(desc), _ptr(tpl), _ptr(seq), seq.size, _ptr(refs), _ptr(out), out_stride, _ptr(skip), _ptr(off)))
        self._pending = (out, skip)
        o2, s2 = self.block_fetch()
        if inplace:
            for b in pins:
                b.free()
        return off, o2.copy(), s2.copy()

    def prepare_templates_device(self, raw, seq, misms, left_trim=(0, 0), right_trim=(0, 0), min_qual=20, keep_on_device=False,
                                 profile=None, x=None, ref=None):
        """bsc_prepare_templates_device: the read pre-processing on the GPU.  Host arrays in (uploaded with torch), the prepared
        templates / read bytes / PREP_STATS back — or, keep_on_device, the two device tensors (uint8 views) and the byte count, for
        a caller that goes on with accumulate_device / reads_chain_device."""
        import torch

        from .abi import MISMS, PREP_PARAMS, PREP_STATS, RAW_TEMPLATE

        raw = np.ascontiguousarray(raw, dtype=RAW_TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        misms = np.ascontiguousarray(misms, dtype=MISMS)
        par = np.zeros(1, dtype=PREP_PARAMS)
        par["left_trim"][0], par["right_trim"][0], par["min_qual"][0] = left_trim, right_trim, min_qual
        cap = int(seq.size) + int(np.minimum(misms["size"][misms["type"] == 1].astype(np.uint64), np.uint64(seq.size)).sum()) + 16
        dev = torch.device("cuda", torch.cuda.current_device())

        def up(a):
            b = a.view(np.uint8).reshape(-1)
            return torch.from_numpy(b.copy()).to(dev) if b.size else torch.zeros(64, dtype=torch.uint8, device=dev)

        d_raw, d_seq, d_ms = up(raw), up(seq), up(misms)
        d_tpl = torch.zeros(max(len(raw), 1) * TEMPLATE.itemsize, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
        used = C.c_uint64(0)
        st = np.zeros(1, dtype=PREP_STATS)
        pf = None
        if profile is not None:  # the read profile: the block's codes (x .. y + 2) on the device, the counts on the host
            d_ref = up(np.ascontiguousarray(ref, dtype=np.uint8))
            pf = _lib.ReadProfile(d_ref.data_ptr(), int(x), len(ref), profile.counts.ctypes.data, profile.counts.shape[0], profile.used)
        _check(self._L.bsc_prepare_templates_device(self._h, d_raw.data_ptr(), len(raw), d_seq.data_ptr(), seq.size, d_ms.data_ptr(), len(misms),
                                                    _ptr(par), d_tpl.data_ptr(), d_out.data_ptr(), cap, C.byref(used), _ptr(st),
                                                    None if pf is None else C.byref(pf), None))
        if pf is not None:
            profile.used = int(pf.used)
        if keep_on_device:
            return d_tpl, d_out, int(used.value), st[0]
        tpl = d_tpl.cpu().numpy()[: len(raw) * TEMPLATE.itemsize].view(TEMPLATE).copy()
        return tpl, d_out.cpu().numpy()[: used.value].copy(), st[0]

    def block_fetch(self):
        """Wait for the submitted block and return (GT_METH[n] or uint8[n, stride], skip)."""
        if self._pending is None:
            raise BscError(-1, "block_fetch: no block was submitted")
        pending, self._pending = self._pending, None
        if not isinstance(pending[0], int):  # block_submit_to: the records are already on their way
            out, skip = pending
            _check(self._L.bsc_block_fetch(self._h, None, None))
            return out, skip
        n, stride = pending
        out = np.zeros(n, dtype=GT_METH) if stride == 200 else np.zeros((n, stride), dtype=np.uint8)
        skip = np.zeros(n, dtype=np.uint8)
        _check(self._L.bsc_block_fetch(self._h, _ptr(out), _ptr(skip)))
        return out, skip

    # -- VCF record formation (src/print_vcf.c:32-381) -------------------------------------------------
    def vcf_records(self, gtm, skip, ref, x, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None):
        """gtm: GT_METH[n] (or uint8[n, 208]) for positions x..x+n-1; ref: uint8[n+2] codes of x..x+n+1 -> VCF_CORE[n]."""
        n = len(gtm)
        stride = 200 if gtm.dtype == GT_METH else gtm.shape[1]
        gtm = np.ascontiguousarray(gtm)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        if len(skip) != n or len(ref) != n + 2:
            raise ValueError("skip must have n and ref n + 2 entries")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        out = np.zeros(n, dtype=VCF_CORE)
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        _check(self._L.bsc_vcf_records(self._h, _ptr(gtm), stride, _ptr(skip), _ptr(ref), None if db is None else _ptr(db),
                                       n, x, C.byref(p), _ptr(out)))
        return out

    def vcf_records_device(self, d_gtm, stride, d_skip, d_ref, n, x, d_out, all_positions=False, reg_start=1,
                           reg_stop=0xFFFFFFFF, d_dbsnp=None, stream=None):
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        _check(self._L.bsc_vcf_records_device(self._h, d_gtm, stride, d_skip, d_ref, d_dbsnp, n, x, C.byref(p), d_out, stream))

    # -- the fused chain: pile-ups in, records (+ statistics) out, gt_meth never in HBM -------------------------------
    def chain_device(self, d_cts, d_ref, x, n_block, first, n, d_core, all_positions=False, reg_start=1,
                     reg_stop=0xFFFFFFFF, d_dbsnp=None, with_stats=False, stream=None):
        """One window (block positions first .. first + n - 1) of the block x .. x + n_block - 1.  d_cts points at the
        pile-up of block position first - min(2, first), d_ref at the reference code of first - min(4, first) (see
        include/bscall_amd.h); d_core receives n VCF_CORE records."""
        w = _lib.Window(x, n_block, first, n)
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        _check(self._L.bsc_chain_device(self._h, d_cts, d_ref, d_dbsnp, C.byref(w), C.byref(p), 1 if with_stats else 0,
                                        d_core, stream))

    def reads_chain_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_core, d_aux=None, all_positions=False, reg_start=1,
                           reg_stop=0xFFFFFFFF, d_dbsnp=None, with_stats=False, stream=None):
        """One block, reads in / records out in the chain's single pass (bsc_reads_chain_device): device-resident
        TEMPLATE[nr] + read bytes, d_ref = codes of x .. y + 2 -> d_core (VCF_CORE per position) [+ d_aux, 64 B per position]."""
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        _check(self._L.bsc_reads_chain_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_dbsnp, C.byref(p),
                                              1 if with_stats else 0, d_core, d_aux, stream))

    def reads_chain_len_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_core, d_aux, d_len, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF,
                               d_dbsnp=None, with_stats=False, stream=None):
        """bsc_reads_chain_len_device: reads_chain_device that also leaves every written record's BCF2 length in d_len (a byte per position)."""
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        _check(self._L.bsc_reads_chain_len_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_dbsnp, C.byref(p), 1 if with_stats else 0, d_core,
                                                  d_aux, d_len, stream))

    def bcf_sites_len_device(self, d_core, d_aux, d_len, n, rid, d_out, out_cap, d_totals, names=None, ids=None, stream=None):
        """bsc_bcf_sites_len_device: bcf_sites_device sized from the chain's length bytes (the records are read once)."""
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep = self._bcf_names(names)
        _check(self._L.bsc_bcf_sites_len_device(self._h, d_core, d_aux, d_len, n, rid, C.byref(ids), None if nm is None else C.addressof(nm), d_out,
                                                out_cap, d_totals, stream))
        del keep

    def last_reads_chain_ms(self):
        ms = C.c_float()
        _check(self._L.bsc_last_reads_chain_ms(self._h, C.byref(ms)))
        return ms.value

    def window_size(self, limit: int) -> int:
        """The largest window <= limit positions in which every resident wave runs the same number of tiles (`bsc_chain_window_size`)."""
        return int(self._L.bsc_chain_window_size(self._h, int(limit)))

    def window_quantum(self) -> int:
        """Positions one round of the resident waves covers (`bsc_chain_window_quantum`)."""
        return int(self._L.bsc_chain_window_quantum(self._h))

    def last_chain_ms(self):
        ms = C.c_float()
        _check(self._L.bsc_last_chain_ms(self._h, C.byref(ms)))
        return ms.value

    # -- reads in, written records out (packed: only what the printer would write crosses PCIe) -----------------
    def block_records(self, templates, seq, x, y, ref, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None,
                      with_stats=False, out=None):
        """One block from reads to packed records (VCF_REC[n_written], position order).  ref: uint8[y - x + 3] codes
        of x .. y + 2.  `out`: optional preallocated VCF_REC array (capacity); default capacity = every position."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        if db is not None and len(db) != n:
            raise ValueError("dbsnp must have y - x + 1 entries")
        if out is None:
            out = np.zeros(n, dtype=VCF_REC)
        elif out.dtype != VCF_REC or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("out must be a writable C-contiguous VCF_REC array")
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        cnt = C.c_uint64(0)
        _check(self._L.bsc_block_records(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(ref),
                                         None if db is None else _ptr(db), C.byref(p), 1 if with_stats else 0, _ptr(out),
                                         len(out), C.byref(cnt)))
        return out[: cnt.value]

    def block_records_raw(self, raw, seq, misms, x, y, ref, left_trim=(0, 0), right_trim=(0, 0), min_qual=20, all_positions=False,
                          reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None, with_stats=False, out=None, profile=None):
        """bsc_block_records_raw: one block from what the reader delivers (RAW_TEMPLATE[nr], read bytes, MISMS[]) to packed records;
        the read pre-processing runs on the GPU.  Returns (VCF_REC[n_written], PREP_STATS record)."""
        from .abi import MISMS, PREP_PARAMS, PREP_STATS, RAW_TEMPLATE

        raw = np.ascontiguousarray(raw, dtype=RAW_TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        misms = np.ascontiguousarray(misms, dtype=MISMS)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        if out is None:
            out = np.zeros(n, dtype=VCF_REC)
        par = np.zeros(1, dtype=PREP_PARAMS)
        par["left_trim"][0], par["right_trim"][0], par["min_qual"][0] = left_trim, right_trim, min_qual
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        cnt = C.c_uint64(0)
        st = np.zeros(1, dtype=PREP_STATS)
        pf = None if profile is None else _lib.ReadProfile(None, 0, 0, profile.counts.ctypes.data, profile.counts.shape[0], profile.used)
        _check(self._L.bsc_block_records_raw(self._h, _ptr(raw), len(raw), _ptr(seq), seq.size, _ptr(misms), len(misms), _ptr(par), x, y,
                                             _ptr(ref), None if db is None else _ptr(db), C.byref(p), 1 if with_stats else 0, _ptr(out),
                                             len(out), C.byref(cnt), _ptr(st), None if pf is None else C.byref(pf)))
        if pf is not None:
            profile.used = int(pf.used)
        return out[: cnt.value], st[0]

    # -- reads in, the block's BCF stream out (encoded on the device, csrc/bcfdev.hip) ---------------------------------------
    @staticmethod
    def _bcf_names(names):
        """names: None, or (pos uint32[n] ascending, off uint32[n + 1], bytes) as DbSnpIndex.names gives them -> (struct, keep-alive)."""
        if names is None:
            return None, None
        pos = np.ascontiguousarray(names[0], dtype=np.uint32)
        off = np.ascontiguousarray(names[1], dtype=np.uint32)
        by = np.frombuffer(bytes(names[2]) + b"\0", dtype=np.uint8)
        if len(off) != len(pos) + 1:
            raise ValueError("names: off must have one entry more than pos")
        st = _lib.BcfNames(pos.ctypes.data, off.ctypes.data, by.ctypes.data, len(pos))
        return st, (pos, off, by)

    def block_bcf(self, templates, seq, x, y, ref, rid, names=None, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None,
                  with_stats=False, cap=None, ids=None):
        """bsc_block_bcf: block_records with the BCF encoder behind the packing, on the device.  Returns (bytes, n_records)."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        if db is not None and len(db) != n:
            raise ValueError("dbsnp must have y - x + 1 entries")
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep = self._bcf_names(names)
        cap_given = cap
        cap = 64 + 192 * n if cap is None else int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        nb, nr = C.c_uint64(0), C.c_uint64(0)

        def go(stats):
            return self._L.bsc_block_bcf(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(ref), None if db is None else _ptr(db),
                                         C.byref(p), stats, rid, C.byref(ids), None if nm is None else C.addressof(nm), _ptr(out), cap, C.byref(nb),
                                         C.byref(nr))

        rc = go(1 if with_stats else 0)
        if rc == -1 and nb.value > cap and cap_given is None:  # longer records than the default room: the encoder alone once more
            cap = int(nb.value)
            out = np.empty(cap, dtype=np.uint8)
            rc = self._L.bsc_block_bcf_again(self._h, _ptr(out), cap, C.byref(nb), C.byref(nr))
        _check(rc)
        del keep
        return out[: nb.value].tobytes(), nr.value

    def block_bcf_raw(self, raw, seq, misms, x, y, ref, rid, names=None, left_trim=(0, 0), right_trim=(0, 0), min_qual=20, all_positions=False,
                      reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None, with_stats=False, cap=None, profile=None, ids=None):
        """bsc_block_bcf_raw: what the reader delivers in, the block's BCF bytes out; pre-processing, calling, record formation and the
        encoding all on the device.  Returns (bytes, n_records, PREP_STATS record)."""
        from .abi import MISMS, PREP_PARAMS, PREP_STATS, RAW_TEMPLATE

        raw = np.ascontiguousarray(raw, dtype=RAW_TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        misms = np.ascontiguousarray(misms, dtype=MISMS)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep = self._bcf_names(names)
        cap_given = cap
        cap = 64 + 192 * n if cap is None else int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        par = np.zeros(1, dtype=PREP_PARAMS)
        par["left_trim"][0], par["right_trim"][0], par["min_qual"][0] = left_trim, right_trim, min_qual
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        nb, nr = C.c_uint64(0), C.c_uint64(0)
        st = np.zeros(1, dtype=PREP_STATS)
        pf = None if profile is None else _lib.ReadProfile(None, 0, 0, profile.counts.ctypes.data, profile.counts.shape[0], profile.used)

        def go(stats, st_, pf_):
            return self._L.bsc_block_bcf_raw(self._h, _ptr(raw), len(raw), _ptr(seq), seq.size, _ptr(misms), len(misms), _ptr(par), x, y, _ptr(ref),
                                             None if db is None else _ptr(db), C.byref(p), stats, rid, C.byref(ids),
                                             None if nm is None else C.addressof(nm), _ptr(out), cap, C.byref(nb), C.byref(nr), _ptr(st_),
                                             None if pf_ is None else C.byref(pf_))

        rc = go(1 if with_stats else 0, st, pf)
        if rc == -1 and nb.value > cap and cap_given is None:  # as block_bcf
            cap = int(nb.value)
            out = np.empty(cap, dtype=np.uint8)
            rc = self._L.bsc_block_bcf_again(self._h, _ptr(out), cap, C.byref(nb), C.byref(nr))
        _check(rc)
        del keep
        if pf is not None:
            profile.used = int(pf.used)
        return out[: nb.value].tobytes(), nr.value, st[0]

    def block_bcf_rawdev(self, blk, ref, rid, names=None, left_trim=(0, 0), right_trim=(0, 0), min_qual=20, all_positions=False, reg_start=1,
                         reg_stop=0xFFFFFFFF, dbsnp=None, with_stats=False, cap=None, profile=None, ids=None, keep=False):
        """bsc_block_bcf_rawdev: a block of the DEVICE reader (bamdev.DeviceBamReader.device_blocks(): raw templates, reads and lists in HBM)
        -> the block's BCF bytes; nothing of the reads crosses PCIe a second time.  Returns (bytes, n_records, PREP_STATS record).
        keep: bsc_block_bcf_rawdev_keep + bsc_bcf_stream_read — the same bytes, the stream and the block's arrays left on the device for
        block_csi_kept / block_meth_kept."""
        from .abi import PREP_PARAMS, PREP_STATS

        x, y = int(blk.x), int(blk.y)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = y - x + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep_nm = self._bcf_names(names)
        cap_given = cap
        cap = 64 + 192 * n if cap is None else int(cap)
        out = None if keep else np.empty(max(cap, 1), dtype=np.uint8)
        par = np.zeros(1, dtype=PREP_PARAMS)
        par["left_trim"][0], par["right_trim"][0], par["min_qual"][0] = left_trim, right_trim, min_qual
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        nb, nr = C.c_uint64(0), C.c_uint64(0)
        st = np.zeros(1, dtype=PREP_STATS)
        pf = None if profile is None else _lib.ReadProfile(None, 0, 0, profile.counts.ctypes.data, profile.counts.shape[0], profile.used)

        def go(stats, st_, pf_):
            if keep:
                return self._L.bsc_block_bcf_rawdev_keep(self._h, blk.d_tpl, blk.nr, blk.d_seq, blk.seq_bytes, blk.d_misms, blk.n_misms, blk.ins_pad, _ptr(par),
                                                         x, y, _ptr(ref), None if db is None else _ptr(db), C.byref(p), stats, rid, C.byref(ids),
                                                         None if nm is None else C.addressof(nm), cap, C.byref(nb), C.byref(nr), _ptr(st_),
                                                         None if pf_ is None else C.byref(pf_))
            return self._L.bsc_block_bcf_rawdev(self._h, blk.d_tpl, blk.nr, blk.d_seq, blk.seq_bytes, blk.d_misms, blk.n_misms, blk.ins_pad, _ptr(par), x, y,
                                                _ptr(ref), None if db is None else _ptr(db), C.byref(p), stats, rid, C.byref(ids),
                                                None if nm is None else C.addressof(nm), _ptr(out), cap, C.byref(nb), C.byref(nr), _ptr(st_),
                                                None if pf_ is None else C.byref(pf_))

        rc = go(1 if with_stats else 0, st, pf)
        if rc == -1 and nb.value > cap and cap_given is None:
            cap = int(nb.value)
            out = None if keep else np.empty(cap, dtype=np.uint8)
            rc = self._L.bsc_block_bcf_again(self._h, None if keep else _ptr(out), cap, C.byref(nb), C.byref(nr))
        _check(rc)
        del keep_nm
        if pf is not None:
            profile.used = int(pf.used)
        if keep:
            out = np.empty(max(int(nb.value), 1), dtype=np.uint8)
            if nb.value:
                _check(self._L.bsc_bcf_stream_read(self._h, 0, nb.value, _ptr(out)))
                self.synchronize()
        return out[: nb.value].tobytes(), nr.value, st[0]

    def block_bcf_submit(self, templates, seq, x, y, ref, rid, out, names=None, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None,
                         with_stats=False, ids=None, inplace=False):
        """bsc_block_bcf_submit: queue the block and return (inputs are staged: the arrays may be reused at once); `out`: a writable uint8
        array (a PinnedBuffer's, ideally) that receives the stream; block_bcf_fetch() waits and returns (bytes view, n_records)."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        if db is not None and len(db) != n:
            raise ValueError("dbsnp must have y - x + 1 entries")
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("out must be a writable C-contiguous uint8 array")
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep = self._bcf_names(names)
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        fn = self._L.bsc_block_bcf_submit_inplace if inplace else self._L.bsc_block_bcf_submit
        _check(fn(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(ref), None if db is None else _ptr(db), C.byref(p),
                  1 if with_stats else 0, rid, C.byref(ids), None if nm is None else C.addressof(nm), _ptr(out), out.size))
        del keep
        self._bcf_out = out
        self._bcf_in = (templates, seq, ref, db) if inplace else None  # read where they lie until the fetch

    def block_bcf_fetch(self):
        nb, nr = C.c_uint64(0), C.c_uint64(0)
        out, self._bcf_out = getattr(self, "_bcf_out", None), None
        try:
            _check(self._L.bsc_block_bcf_fetch(self._h, C.byref(nb), C.byref(nr)))
        finally:
            self._bcf_in = None
        return out[: nb.value], nr.value

    def bcf_block_device(self, d_recs, d_n_recs, max_recs, rid, d_out, out_cap, d_totals, names=None, ids=None, stream=None):
        """bsc_bcf_block_device: packed records in HBM -> their BCF stream in HBM (asynchronous on `stream`)."""
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep = self._bcf_names(names)
        _check(self._L.bsc_bcf_block_device(self._h, d_recs, d_n_recs, max_recs, rid, C.byref(ids), None if nm is None else C.addressof(nm), d_out,
                                            out_cap, d_totals, stream))
        del keep

    def bcf_sites_device(self, d_core, d_aux, n, rid, d_out, out_cap, d_totals, names=None, ids=None, stream=None):
        """bsc_bcf_sites_device: the per-position arrays of reads_chain_device (d_core, d_aux) -> the BCF stream, no packing pass."""
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep = self._bcf_names(names)
        _check(self._L.bsc_bcf_sites_device(self._h, d_core, d_aux, n, rid, C.byref(ids), None if nm is None else C.addressof(nm), d_out, out_cap,
                                            d_totals, stream))
        del keep

    # -- VCF text on the device (csrc/vcftextdev.hip) ---------------------------------------------------
    @staticmethod
    def _contig_bytes(contig):
        return contig if isinstance(contig, (bytes, bytearray)) else str(contig).encode()

    def fmt_g_device(self, d_v, n, d_out16, stream=None):
        """bsc_fmt_g_device: n floats in HBM -> 16-byte slots in HBM (the characters of "%g", zero padding, the length in byte 15)."""
        _check(self._L.bsc_fmt_g_device(self._h, d_v, n, d_out16, stream))

    def fmt_g(self, values):
        """bsc_fmt_g: the host checker of fmt_g_device (the C library's snprintf), float32[n] -> uint8[n, 16]."""
        v = np.ascontiguousarray(values, dtype=np.float32)
        out = np.zeros((len(v), 16), dtype=np.uint8)
        _check(self._L.bsc_fmt_g(_ptr(v), len(v), _ptr(out)))
        return out

    def vcf_text_block_device(self, d_recs, d_n_recs, max_recs, contig, d_out, out_cap, d_totals, names=None, stream=None):
        """bsc_vcf_text_block_device: packed records in HBM -> their VCF lines in HBM (asynchronous on `stream`)."""
        nm, keep = self._bcf_names(names)
        _check(self._L.bsc_vcf_text_block_device(self._h, d_recs, d_n_recs, max_recs, self._contig_bytes(contig), None if nm is None else C.addressof(nm),
                                                 d_out, out_cap, d_totals, stream))
        del keep

    def vcf_text_sites_device(self, d_core, d_aux, n, contig, d_out, out_cap, d_totals, names=None, stream=None):
        """bsc_vcf_text_sites_device: the per-position arrays of reads_chain_device (d_core, d_aux) -> the VCF lines, no packing pass."""
        nm, keep = self._bcf_names(names)
        _check(self._L.bsc_vcf_text_sites_device(self._h, d_core, d_aux, n, self._contig_bytes(contig), None if nm is None else C.addressof(nm), d_out,
                                                 out_cap, d_totals, stream))
        del keep

    def block_vcf_rawdev(self, blk, ref, contig, names=None, left_trim=(0, 0), right_trim=(0, 0), min_qual=20, all_positions=False, reg_start=1,
                         reg_stop=0xFFFFFFFF, dbsnp=None, with_stats=False, cap=None, profile=None):
        """bsc_block_vcf_rawdev_keep + bsc_bcf_stream_read: a block of the DEVICE reader -> the block's VCF lines (bytes), encoded on the
        device.  Returns (bytes, n_records, PREP_STATS record).  cap: the room on the device (default: sized from the block; a stream
        that does not fit is encoded once more into the room it needs, bsc_block_bcf_again)."""
        from .abi import PREP_PARAMS, PREP_STATS

        x, y = int(blk.x), int(blk.y)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = y - x + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        nm, keep = self._bcf_names(names)
        cap_given = cap
        cap = 64 + 160 * n if cap is None else int(cap)
        par = np.zeros(1, dtype=PREP_PARAMS)
        par["left_trim"][0], par["right_trim"][0], par["min_qual"][0] = left_trim, right_trim, min_qual
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        nb, nr = C.c_uint64(0), C.c_uint64(0)
        st = np.zeros(1, dtype=PREP_STATS)
        pf = None if profile is None else _lib.ReadProfile(None, 0, 0, profile.counts.ctypes.data, profile.counts.shape[0], profile.used)
        rc = self._L.bsc_block_vcf_rawdev_keep(self._h, blk.d_tpl, blk.nr, blk.d_seq, blk.seq_bytes, blk.d_misms, blk.n_misms, blk.ins_pad, _ptr(par), x, y,
                                               _ptr(ref), None if db is None else _ptr(db), C.byref(p), 1 if with_stats else 0,
                                               self._contig_bytes(contig), None if nm is None else C.addressof(nm), cap, C.byref(nb), C.byref(nr),
                                               _ptr(st), None if pf is None else C.byref(pf))
        if rc == -1 and nb.value > cap and cap_given is None:
            cap = int(nb.value)
            rc = self._L.bsc_block_bcf_again(self._h, None, cap, C.byref(nb), C.byref(nr))
        _check(rc)
        del keep
        if pf is not None:
            profile.used = int(pf.used)
        out = np.empty(max(int(nb.value), 1), dtype=np.uint8)
        if nb.value:
            _check(self._L.bsc_bcf_stream_read(self._h, 0, nb.value, _ptr(out)))
            self.synchronize()
        return out[: nb.value].tobytes(), nr.value, st[0]

    # -- the per-cytosine methylation table on the device (csrc/methdev.hip) -------------------------------
    @staticmethod
    def _meth_params(params):
        if params is None:
            return _lib.MethParams()
        if isinstance(params, _lib.MethParams):
            return params
        return _lib.MethParams(**params)

    def meth_block_device(self, d_recs, d_n_recs, max_recs, contig, d_out, out_cap, d_totals, params=None, stream=None):
        """bsc_meth_block_device: packed records in HBM -> their bedMethyl lines in HBM (asynchronous on `stream`); d_totals: four u64."""
        mp = self._meth_params(params)
        _check(self._L.bsc_meth_block_device(self._h, d_recs, d_n_recs, max_recs, self._contig_bytes(contig), C.byref(mp), d_out, out_cap, d_totals, stream))

    def meth_sites_device(self, d_core, d_aux, n, contig, d_out, out_cap, d_totals, params=None, stream=None):
        """bsc_meth_sites_device: the per-position arrays of reads_chain_device (d_core, d_aux) -> the bedMethyl lines."""
        mp = self._meth_params(params)
        _check(self._L.bsc_meth_sites_device(self._h, d_core, d_aux, n, self._contig_bytes(contig), C.byref(mp), d_out, out_cap, d_totals, stream))

    def meth_cpg_block_device(self, d_recs, d_n_recs, max_recs, contig, d_out, out_cap, d_totals, params=None, stream=None):
        """bsc_meth_cpg_block_device: packed records in HBM -> the combined-strand CpG table (one line per dinucleotide) in HBM
        (asynchronous on `stream`); d_totals: FIVE u64 {length, lines, sum of A, sum of B, pairs written}."""
        mp = self._meth_params(params)
        _check(self._L.bsc_meth_cpg_block_device(self._h, d_recs, d_n_recs, max_recs, self._contig_bytes(contig), C.byref(mp), d_out, out_cap, d_totals, stream))

    def meth_cpg_sites_device(self, d_core, d_aux, n, contig, d_out, out_cap, d_totals, params=None, stream=None):
        """bsc_meth_cpg_sites_device: the per-position arrays of reads_chain_device (d_core, d_aux) -> the combined-strand CpG table."""
        mp = self._meth_params(params)
        _check(self._L.bsc_meth_cpg_sites_device(self._h, d_core, d_aux, n, self._contig_bytes(contig), C.byref(mp), d_out, out_cap, d_totals, stream))

    @staticmethod
    def _regions_array(regions):
        """(start, end) pairs, or a structured array with those fields, as contiguous uint32[n, 2]."""
        r = np.asarray(regions)
        if r.dtype.names:
            r = np.stack([r["start"], r["end"]], axis=1) if len(r) else np.zeros((0, 2), np.uint32)
        r = r.reshape(-1, 2)
        if len(r) and (r.min() < 0 or r.max() > 0xFFFFFFFF):
            raise ValueError("a region's coordinates are 0 .. 2^32 - 1")
        return np.ascontiguousarray(r, dtype=np.uint32)

    def meth_regions_attach(self, regions):
        """bsc_meth_regions_attach: the regions of ONE contig — (start, end) pairs, 0-based and half-open as in BED, sorted by (start, end) —
        uploaded, their accumulators zeroed.  An empty list detaches.  Refused (BscError) when unsorted or start > end: the previous
        attachment then stays.  Returns the count."""
        r = self._regions_array(regions)
        _check(self._L.bsc_meth_regions_attach(self._h, _ptr(r) if len(r) else None, len(r)))
        self._n_meth_regions = len(r)
        return len(r)

    def meth_regions_sites_device(self, d_core, d_aux, n, x0, params=None, stream=None):
        """bsc_meth_regions_sites_device: the per-position arrays of reads_chain_device (entry i = position x0 + i) added into the attached
        regions' accumulators {sites, sum of a, sum of b, sum of pct} (csrc/methregionsdev.hip; asynchronous on `stream`)."""
        mp = self._meth_params(params)
        _check(self._L.bsc_meth_regions_sites_device(self._h, d_core, d_aux, n, x0, C.byref(mp), stream))

    def block_meth_regions_kept(self, params=None):
        """bsc_block_meth_regions_kept: the block the last *_keep call called, added into the attached regions' accumulators from the arrays
        it left on the device.  Returns the block's own (sites, sum of a, sum of b)."""
        mp = self._meth_params(params)
        ns, sums = C.c_uint64(0), (C.c_uint64 * 3)()
        _check(self._L.bsc_block_meth_regions_kept(self._h, C.byref(mp), C.byref(ns), sums))
        return tuple(int(v) for v in sums)

    def meth_regions_read(self):
        """bsc_meth_regions_read: the accumulators as uint64[n, 4] — per attached region {sites, A, B, P} (waits)."""
        n = getattr(self, "_n_meth_regions", 0)
        acc = np.zeros((n, 4), dtype=np.uint64)
        _check(self._L.bsc_meth_regions_read(self._h, _ptr(acc) if n else None, n))
        return acc

    def meth_regions_reset(self):
        """bsc_meth_regions_reset: the accumulators zeroed, the regions stay."""
        _check(self._L.bsc_meth_regions_reset(self._h))

    # -- the methylation bigWig track on the device (csrc/bigwigdev.hip) ------------------------------------
    @staticmethod
    def _bw_params(params):
        if params is None:
            return _lib.BwParams()
        if isinstance(params, _lib.BwParams):
            return params
        return _lib.BwParams(**params)

    def bigwig_sites_device(self, d_core, d_aux, n, x0, chrom_id, d_out, out_cap, d_sections, sec_cap, d_zoom, zoom_cap, d_totals, params=None,
                            bw_params=None, stream=None):
        """bsc_bigwig_sites_device: the per-position arrays of reads_chain_device (entry i = position x0 + i) -> the block's bigWig data stream
        in d_out, the sections' and the level-0 windows' 40-byte summaries, and d_totals: six u64 {bytes, sites, sections, windows, sum of m,
        sum of m * m} (asynchronous on `stream`).  An array whose room is too small is not written; the needs are in d_totals."""
        mp, bp = self._meth_params(params), self._bw_params(bw_params)
        _check(self._L.bsc_bigwig_sites_device(self._h, d_core, d_aux, n, x0, chrom_id, C.byref(mp), C.byref(bp), d_out, out_cap, d_sections, sec_cap,
                                               d_zoom, zoom_cap, d_totals, stream))

    def block_bigwig_kept(self, chrom_id, params=None, bw_params=None, read_stream=True):
        """bsc_block_bigwig_kept + bsc_bigwig_stream_read: the bigWig data of the block the last *_keep call called, from the arrays it left on
        the device.  Returns (stream bytes, sites, sections, zoom0): the two summaries as bigwig.BW_SUM arrays (copies).  read_stream=False:
        the stream stays on the device (block_bigwig_deflate follows) and its length comes back in the bytes' place."""
        from .bigwig import BW_SUM

        mp, bp = self._meth_params(params), self._bw_params(bw_params)
        nb, ns, nsec, nz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        p_sec, p_zoom = C.c_void_p(None), C.c_void_p(None)
        _check(self._L.bsc_block_bigwig_kept(self._h, chrom_id, C.byref(mp), C.byref(bp), C.byref(nb), C.byref(ns), C.byref(p_sec), C.byref(nsec),
                                             C.byref(p_zoom), C.byref(nz)))
        grab = lambda p, k: np.frombuffer(C.string_at(p.value, 40 * k), dtype=BW_SUM).copy() if k else np.zeros(0, dtype=BW_SUM)
        sections, zoom0 = grab(p_sec, nsec.value), grab(p_zoom, nz.value)
        return (self.bigwig_stream_read(0, nb.value) if read_stream else int(nb.value)), int(ns.value), sections, zoom0

    def bigwig_stream_read(self, off, n):
        """bsc_bigwig_stream_read: bytes [off, off + n) of the stream block_bigwig_kept left on the device (waits)."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        if n:
            _check(self._L.bsc_bigwig_stream_read(self._h, off, n, _ptr(out)))
            self.synchronize()
        return out[:n].tobytes()

    # -- zlib streams of fixed-stride pieces, and of a block's bigWig sections (csrc/zlibdev.hip) -----------
    def zlib_pieces_device(self, d_src, n_bytes, piece, d_out, out_cap, d_sizes, sizes_cap, d_totals, stream=None):
        """bsc_zlib_pieces_device: piece k = bytes [k piece, min((k + 1) piece, n_bytes)) of d_src -> one zlib stream each, back to back in
        d_out, their lengths (u32) in d_sizes, and d_totals: two u64 {bytes out, pieces} (asynchronous on `stream`).  An array whose room is
        too small is not written; the needs are in d_totals."""
        _check(self._L.bsc_zlib_pieces_device(self._h, d_src, n_bytes, piece, d_out, out_cap, d_sizes, sizes_cap, d_totals, stream))

    def block_bigwig_deflate(self):
        """bsc_block_bigwig_deflate + bsc_bigwig_zstream_read: the sections of the stream block_bigwig_kept just left on the device, one
        zlib stream each.  Returns (the streams' bytes back to back, their sizes as a uint32 array (a copy))."""
        nb, nsec = C.c_uint64(0), C.c_uint64(0)
        p_sz = C.c_void_p(None)
        _check(self._L.bsc_block_bigwig_deflate(self._h, C.byref(nb), C.byref(p_sz), C.byref(nsec)))
        sizes = np.frombuffer(C.string_at(p_sz.value, 4 * nsec.value), dtype=np.uint32).copy() if nsec.value else np.zeros(0, dtype=np.uint32)
        return self.bigwig_zstream_read(0, nb.value), sizes

    def bigwig_zstream_read(self, off, n):
        """bsc_bigwig_zstream_read: bytes [off, off + n) of the streams block_bigwig_deflate left on the device (waits)."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        if n:
            _check(self._L.bsc_bigwig_zstream_read(self._h, off, n, _ptr(out)))
            self.synchronize()
        return out[:n].tobytes()

    # -- the coverage track, alone or with the level track in one sweep (csrc/bwcovdev.hip) -----------------
    def bigwig_tracks_device(self, d_core, d_aux, n, x0, chrom_id, tracks, level_out, cov_out, d_totals, params=None, bw_params=None, stream=None):
        """bsc_bigwig_tracks_device: bigwig_sites_device for a mask of tracks (1 level, 2 coverage, 3 both) in one sweep.  level_out / cov_out:
        (d_out, out_cap, d_sections, sec_cap, d_zoom, zoom_cap) or a _lib.BwTrackOut per requested track, None for the other; d_totals: six
        u64 {bytes, sites, sections, windows, sum of m, sum of m * m}, the last two 0 without the level track."""
        mp, bp = self._meth_params(params), self._bw_params(bw_params)
        desc = lambda o: None if o is None else C.byref(o if isinstance(o, _lib.BwTrackOut) else _lib.BwTrackOut(*o))
        _check(self._L.bsc_bigwig_tracks_device(self._h, d_core, d_aux, n, x0, chrom_id, C.byref(mp), C.byref(bp), tracks, desc(level_out), desc(cov_out),
                                                d_totals, stream))

    def block_bigwig_tracks_kept(self, chrom_id, tracks, params=None, bw_params=None, read_stream=True):
        """bsc_block_bigwig_tracks_kept (+ the stream reads): the bigWig data of the block the last *_keep call called, for a mask of tracks
        in one sweep.  Returns (sites, level, coverage): per requested track (stream bytes, sections, zoom0) — the summaries as
        bigwig.BW_SUM arrays (copies) —, None for the other.  read_stream=False: the streams stay on the device (block_bigwig_deflate /
        block_bigwig_cov_deflate follow) and their length comes back in the bytes' place."""
        from .bigwig import BW_SUM

        mp, bp = self._meth_params(params), self._bw_params(bw_params)
        nb, ns, nsec, nz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ptr = [C.c_void_p(None) for _ in range(4)]
        _check(self._L.bsc_block_bigwig_tracks_kept(self._h, chrom_id, C.byref(mp), C.byref(bp), tracks, C.byref(nb), C.byref(ns), C.byref(nsec), C.byref(nz),
                                                    *[C.byref(p) for p in ptr]))
        grab = lambda p, k: np.frombuffer(C.string_at(p.value, 40 * k), dtype=BW_SUM).copy() if k else np.zeros(0, dtype=BW_SUM)
        out = []
        for t, read in ((0, self.bigwig_stream_read), (1, self.bigwig_cov_stream_read)):
            if not tracks & (1 << t):
                out.append(None)
                continue
            sections, zoom0 = grab(ptr[2 * t], nsec.value), grab(ptr[2 * t + 1], nz.value)
            out.append((read(0, nb.value) if read_stream else int(nb.value), sections, zoom0))
        return int(ns.value), out[0], out[1]

    def bigwig_cov_stream_read(self, off, n):
        """bsc_bigwig_cov_stream_read: bytes [off, off + n) of the coverage stream block_bigwig_tracks_kept left on the device (waits)."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        if n:
            _check(self._L.bsc_bigwig_cov_stream_read(self._h, off, n, _ptr(out)))
            self.synchronize()
        return out[:n].tobytes()

    def block_bigwig_cov_deflate(self):
        """bsc_block_bigwig_cov_deflate + bsc_bigwig_cov_zstream_read: block_bigwig_deflate for the coverage stream."""
        nb, nsec = C.c_uint64(0), C.c_uint64(0)
        p_sz = C.c_void_p(None)
        _check(self._L.bsc_block_bigwig_cov_deflate(self._h, C.byref(nb), C.byref(p_sz), C.byref(nsec)))
        sizes = np.frombuffer(C.string_at(p_sz.value, 4 * nsec.value), dtype=np.uint32).copy() if nsec.value else np.zeros(0, dtype=np.uint32)
        return self.bigwig_cov_zstream_read(0, nb.value), sizes

    def bigwig_cov_zstream_read(self, off, n):
        """bsc_bigwig_cov_zstream_read: bytes [off, off + n) of the streams block_bigwig_cov_deflate left on the device (waits)."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        if n:
            _check(self._L.bsc_bigwig_cov_zstream_read(self._h, off, n, _ptr(out)))
            self.synchronize()
        return out[:n].tobytes()

    # -- the bedMethyl table as bigBed items (csrc/bigbeddev.hip), zlib streams of ranges (csrc/zlibdev.hip) --
    def bigbed_sites_device(self, d_core, d_aux, n, x0, chrom_id, d_out, out_cap, d_blocks, blk_cap, d_zoom, zoom_cap, d_totals, params=None,
                            bb_params=None, stream=None):
        """bsc_bigbed_sites_device: the per-position arrays of reads_chain_device (entry i = position x0 + i) -> the call's stream of bigBed
        items in d_out (16-byte aligned), the blocks' and the level-0 windows' 24-byte summaries (bigbed.BB_SUM), and d_totals: four u64
        {bytes, sites, blocks, windows} (asynchronous on `stream`).  An array whose room is too small is not written; the needs are in
        d_totals."""
        mp = self._meth_params(params)
        bp = bb_params if isinstance(bb_params, _lib.BbParams) else _lib.BbParams(**(bb_params or {}))
        _check(self._L.bsc_bigbed_sites_device(self._h, d_core, d_aux, n, x0, chrom_id, C.byref(mp), C.byref(bp), d_out, out_cap, d_blocks, blk_cap,
                                               d_zoom, zoom_cap, d_totals, stream))

    def block_bigbed_kept(self, chrom_id, params=None, bb_params=None, read_stream=True):
        """bsc_block_bigbed_kept + bsc_bigbed_stream_read: the bigBed items of the block the last *_keep call called, from the arrays it left
        on the device.  Returns (stream bytes, sites, blocks, zoom0): the two summaries as bigbed.BB_SUM arrays (copies).  read_stream=False:
        the stream stays on the device (block_bigbed_deflate follows) and its length comes back in the bytes' place."""
        from .bigbed import BB_SUM

        mp = self._meth_params(params)
        bp = bb_params if isinstance(bb_params, _lib.BbParams) else _lib.BbParams(**(bb_params or {}))
        nb, ns, nblk, nz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        p_blk, p_zoom = C.c_void_p(None), C.c_void_p(None)
        _check(self._L.bsc_block_bigbed_kept(self._h, chrom_id, C.byref(mp), C.byref(bp), C.byref(nb), C.byref(ns), C.byref(p_blk), C.byref(nblk),
                                             C.byref(p_zoom), C.byref(nz)))
        grab = lambda p, k: np.frombuffer(C.string_at(p.value, 24 * k), dtype=BB_SUM).copy() if k else np.zeros(0, dtype=BB_SUM)
        blocks, zoom0 = grab(p_blk, nblk.value), grab(p_zoom, nz.value)
        return (self.bigbed_stream_read(0, nb.value) if read_stream else int(nb.value)), int(ns.value), blocks, zoom0

    def bigbed_stream_read(self, off, n):
        """bsc_bigbed_stream_read: bytes [off, off + n) of the stream block_bigbed_kept left on the device (waits)."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        if n:
            _check(self._L.bsc_bigbed_stream_read(self._h, off, n, _ptr(out)))
            self.synchronize()
        return out[:n].tobytes()

    def block_bigbed_deflate(self):
        """bsc_block_bigbed_deflate + bsc_bigbed_zstream_read: the blocks of the stream block_bigbed_kept just left on the device, one zlib
        stream each.  Returns (the streams' bytes back to back, their sizes as a uint32 array (a copy))."""
        nb, nblk = C.c_uint64(0), C.c_uint64(0)
        p_sz = C.c_void_p(None)
        _check(self._L.bsc_block_bigbed_deflate(self._h, C.byref(nb), C.byref(p_sz), C.byref(nblk)))
        sizes = np.frombuffer(C.string_at(p_sz.value, 4 * nblk.value), dtype=np.uint32).copy() if nblk.value else np.zeros(0, dtype=np.uint32)
        out = np.empty(max(int(nb.value), 1), dtype=np.uint8)
        if nb.value:
            _check(self._L.bsc_bigbed_zstream_read(self._h, 0, nb.value, _ptr(out)))
            self.synchronize()
        return out[: nb.value].tobytes(), sizes

    def zlib_ranges_device(self, d_src, d_offs, n_pieces, max_piece, d_out, out_cap, d_sizes, sizes_cap, d_totals, stream=None):
        """bsc_zlib_ranges_device: piece k = bytes [offs[k], offs[k + 1]) of d_src (d_offs: n_pieces + 1 ascending device u64, every length
        1 .. max_piece) -> one zlib stream each, back to back in d_out, their lengths (u32) in d_sizes, and d_totals: three u64 {bytes
        out, pieces, bad ranges}.  Waits for the count of bad ranges: a BscError when it is not 0.  An array whose room is too small is not
        written; the needs are in d_totals."""
        _check(self._L.bsc_zlib_ranges_device(self._h, d_src, d_offs, n_pieces, max_piece, d_out, out_cap, d_sizes, sizes_cap, d_totals, stream))

    def block_meth_kept(self, contig, params=None, cap=None, merge=False):
        """bsc_block_meth_kept + bsc_meth_stream_read: the bedMethyl table of the block the last *_keep call called (block_vcf_rawdev,
        block_bcf_rawdev(keep=True)), from the arrays that block left on the device.  params: a _lib.MethParams, a dict of its fields, or
        None (CpG, every covered site).  Returns (bytes, lines, (sum of a, sum of b)).  cap: the room on the device (default: asked for
        and given on a second call).  merge: the combined-strand table, one line per CpG dinucleotide (bsc_block_meth_cpg_kept); the
        sums are then (sum of A, sum of B, pairs written)."""
        mp = self._meth_params(params)
        entry = self._L.bsc_block_meth_cpg_kept if merge else self._L.bsc_block_meth_kept
        nb, nl, sums = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * (3 if merge else 2))()
        room = 1 << 16 if cap is None else int(cap)
        rc = entry(self._h, self._contig_bytes(contig), C.byref(mp), room, C.byref(nb), C.byref(nl), sums)
        if rc == -1 and nb.value > room and cap is None:
            room = int(nb.value)
            rc = entry(self._h, self._contig_bytes(contig), C.byref(mp), room, C.byref(nb), C.byref(nl), sums)
        _check(rc)
        out = np.empty(max(int(nb.value), 1), dtype=np.uint8)
        if nb.value:
            _check(self._L.bsc_meth_stream_read(self._h, 0, nb.value, _ptr(out)))
            self.synchronize()
        return out[: nb.value].tobytes(), int(nl.value), tuple(int(v) for v in sums)

    # -- the variant-only call set (csrc/variantsdev.hip) --------------------------------------------------
    @staticmethod
    def _var_params(params):
        if params is None:
            return _lib.VarParams()
        if isinstance(params, _lib.VarParams):
            return params
        return _lib.VarParams(**params)

    def variants_sites_device(self, d_core, d_aux, d_emit, n, d_recs, max_recs, d_n_recs, d_totals, params=None, stream=None):
        """bsc_variants_sites_device: the per-position arrays of reads_chain_device (d_core, d_aux; d_emit the chain's byte per position or
        None) -> the selected records, packed, in d_recs[<= max_recs], their count (a device u64) in d_n_recs and the ten totals in
        d_totals (asynchronous on `stream`)."""
        vp_ = self._var_params(params)
        _check(self._L.bsc_variants_sites_device(self._h, d_core, d_aux, d_emit, n, C.byref(vp_), d_recs, max_recs, d_n_recs, d_totals, stream))

    def block_variants_kept(self, params=None, cap=None):
        """bsc_block_variants_kept + bsc_variants_stream_read: the variant-only stream of the block the last *_keep call called — the
        selected records as that call's encoder writes them (BCF2 records or VCF lines).  params: a _lib.VarParams, a dict of its fields,
        or None (every variant).  Returns (bytes, records, totals[10]).  cap: the room on the device (default: asked for and given on a
        second call)."""
        vp_ = self._var_params(params)
        nb, nr, tot = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 10)()
        room = 1 << 16 if cap is None else int(cap)
        rc = self._L.bsc_block_variants_kept(self._h, C.byref(vp_), room, C.byref(nb), C.byref(nr), tot)
        if rc == -1 and nb.value > room and cap is None:
            room = int(nb.value)
            rc = self._L.bsc_block_variants_kept(self._h, C.byref(vp_), room, C.byref(nb), C.byref(nr), tot)
        _check(rc)
        return self.variants_stream_read(0, nb.value), int(nr.value), tuple(int(v) for v in tot)

    def variants_stream_read(self, off, n):
        """bsc_variants_stream_read: bytes [off, off + n) of the variant stream the last block_variants_kept left on the device."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        _check(self._L.bsc_variants_stream_read(self._h, int(off), int(n), _ptr(out)))
        if n:
            self.synchronize()
        return out[: int(n)].tobytes()

    def block_variants_csi_kept(self, min_shift=14):
        """bsc_block_variants_csi_kept: (entries CSI_ENTRY[], records) of the variant stream the last block_variants_kept left on the device."""
        p, n, r = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(self._L.bsc_block_variants_csi_kept(self._h, int(min_shift), C.byref(p), C.byref(n), C.byref(r)))
        if not n.value:
            return np.zeros(0, CSI_ENTRY), int(r.value)
        buf = (C.c_uint8 * (16 * n.value)).from_address(p.value)
        return np.frombuffer(buf, dtype=CSI_ENTRY).copy(), int(r.value)

    # -- the read-level CpG concordance table (csrc/cpgreadsdev.hip) ------------------------------------------
    @staticmethod
    def _cr_params(params):
        if params is None:
            return _lib.CpgReadsParams()
        if isinstance(params, _lib.CpgReadsParams):
            return params
        return _lib.CpgReadsParams(**params)

    def cpg_reads_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_sites, sites_cap, d_n_sites, d_totals, params=None, stream=None):
        """bsc_cpg_reads_device: the inputs of reads_chain_device (prepared templates, their read bytes, the block x .. y, d_ref the codes of
        x .. y + 2) -> one bsc_cpg_reads_site per reference CpG in d_sites[<= sites_cap], their count (a device u64) in d_n_sites and the
        eight totals in d_totals (asynchronous on `stream`)."""
        cp = self._cr_params(params)
        _check(self._L.bsc_cpg_reads_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, C.byref(cp), d_sites, sites_cap, d_n_sites, d_totals,
                                            stream))

    def cpg_reads_text_device(self, d_sites, d_n_sites, max_sites, contig, d_out, out_cap, d_totals2, params=None, stream=None):
        """bsc_cpg_reads_text_device: the table's lines of d_sites[min(*d_n_sites, max_sites)] -> d_out[<= out_cap]; d_totals2: {bytes, lines}."""
        cp = self._cr_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        _check(self._L.bsc_cpg_reads_text_device(self._h, d_sites, d_n_sites, max_sites, name, C.byref(cp), d_out, out_cap, d_totals2, stream))

    def block_cpg_reads_kept(self, contig, params=None, cap=None):
        """bsc_block_cpg_reads_kept + bsc_cpg_reads_stream_read: the read-level CpG table of the block the last *_keep call called, from the
        prepared templates, reads and reference codes it left on the device.  params: a _lib.CpgReadsParams, a dict of its fields, or None
        ({4, 1}).  Returns (bytes, lines, totals[8]).  cap: the room on the device (default: asked for and given on a second call)."""
        cp = self._cr_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        nb, nl, tot = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
        room = 1 << 16 if cap is None else int(cap)
        rc = self._L.bsc_block_cpg_reads_kept(self._h, name, C.byref(cp), room, C.byref(nb), C.byref(nl), tot)
        if rc == -1 and nb.value > room and cap is None:
            room = int(nb.value)
            rc = self._L.bsc_block_cpg_reads_kept(self._h, name, C.byref(cp), room, C.byref(nb), C.byref(nl), tot)
        _check(rc)
        return self.cpg_reads_stream_read(0, nb.value), int(nl.value), tuple(int(v) for v in tot)

    def cpg_reads_stream_read(self, off, n):
        """bsc_cpg_reads_stream_read: bytes [off, off + n) of the table the last block_cpg_reads_kept left on the device."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        _check(self._L.bsc_cpg_reads_stream_read(self._h, int(off), int(n), _ptr(out)))
        if n:
            self.synchronize()
        return out[: int(n)].tobytes()

    # -- the allele-specific methylation table (csrc/asmdev.hip) ----------------------------------------------
    @staticmethod
    def _asm_params(params):
        if params is None:
            return _lib.AsmParams()
        if isinstance(params, _lib.AsmParams):
            return params
        return _lib.AsmParams(**params)

    def asm_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_core, d_emit, d_pairs, pairs_cap, d_n_pairs, d_totals, params=None, stream=None):
        """bsc_asm_device: the inputs of cpg_reads_device, the block's dense bsc_vcf_core records d_core and its emit bytes d_emit (or None) ->
        one bsc_asm_pair per (heterozygous SNP, CpG of its window) in d_pairs[<= pairs_cap], their count (a device u64) in d_n_pairs and the
        eight totals in d_totals (queued on `stream`; waits for the two counts)."""
        cp = self._asm_params(params)
        _check(self._L.bsc_asm_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_core, d_emit, C.byref(cp), d_pairs, pairs_cap, d_n_pairs,
                                      d_totals, stream))

    def asm_text_device(self, d_pairs, d_n_pairs, max_pairs, contig, d_out, out_cap, d_totals2, params=None, stream=None):
        """bsc_asm_text_device: the table's lines of d_pairs[min(*d_n_pairs, max_pairs)] -> d_out[<= out_cap]; d_totals2: {bytes, lines}."""
        cp = self._asm_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        _check(self._L.bsc_asm_text_device(self._h, d_pairs, d_n_pairs, max_pairs, name, C.byref(cp), d_out, out_cap, d_totals2, stream))

    def block_asm_kept(self, contig, params=None, cap=None):
        """bsc_block_asm_kept + bsc_asm_stream_read: the allele-specific methylation table of the block the last *_keep call called, from the
        dense records, the prepared templates, reads and reference codes it left on the device.  params: a _lib.AsmParams, a dict of its
        fields, or None ({20, 0, 500, 2}).  Returns (bytes, lines, totals[8]).  cap: the room on the device (default: asked for and given on
        a second call)."""
        cp = self._asm_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        nb, nl, tot = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
        room = 1 << 16 if cap is None else int(cap)
        rc = self._L.bsc_block_asm_kept(self._h, name, C.byref(cp), room, C.byref(nb), C.byref(nl), tot)
        if rc == -1 and nb.value > room and cap is None:
            room = int(nb.value)
            rc = self._L.bsc_block_asm_kept(self._h, name, C.byref(cp), room, C.byref(nb), C.byref(nl), tot)
        _check(rc)
        return self.asm_stream_read(0, nb.value), int(nl.value), tuple(int(v) for v in tot)

    def asm_stream_read(self, off, n):
        """bsc_asm_stream_read: bytes [off, off + n) of the table the last block_asm_kept left on the device."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        _check(self._L.bsc_asm_stream_read(self._h, int(off), int(n), _ptr(out)))
        if n:
            self.synchronize()
        return out[: int(n)].tobytes()

    # -- the M-bias table (csrc/mbiasdev.hip) -------------------------------------------------------------------------------------------
    @staticmethod
    def _mb_params(params):
        if params is None:
            return _lib.MbiasParams()
        if isinstance(params, _lib.MbiasParams):
            return params
        if isinstance(params, dict):
            return _lib.MbiasParams(**params)
        return _lib.MbiasParams(int(params))

    def mbias_device(self, d_raw, nr, d_seq, seq_bytes, d_misms, n_misms, x, y, d_ref, d_counts, d_totals, params=None, stream=None):
        """bsc_mbias_device: the raw templates of a block (d_raw, d_seq, d_misms as the device reader leaves them), the block x .. y and d_ref,
        the codes of x .. y + 2 -> ADDED into d_counts (12 * n_cycles * 2 device u64) and d_totals (eight device u64); asynchronous on
        `stream`.  params: a _lib.MbiasParams, a dict, n_cycles or None ({512})."""
        mp = self._mb_params(params)
        _check(self._L.bsc_mbias_device(self._h, d_raw, nr, d_seq, seq_bytes, d_misms, n_misms, x, y, d_ref, C.byref(mp), d_counts, d_totals, stream))

    def block_mbias_rawdev(self, d_raw, nr, d_seq, seq_bytes, d_misms, n_misms, params=None):
        """bsc_block_mbias_rawdev: the raw block the last *_keep call called (the SAME device pointers) added into the context's M-bias
        accumulator.  Returns the accumulator's totals[8] so far."""
        mp = self._mb_params(params)
        tot = (C.c_uint64 * 8)()
        _check(self._L.bsc_block_mbias_rawdev(self._h, d_raw, nr, d_seq, seq_bytes, d_misms, n_misms, C.byref(mp), tot))
        self._mbias_cycles = int(mp.n_cycles)  # the accumulator's: what mbias_read sizes its array by
        return tuple(int(v) for v in tot)

    def mbias_read(self, params=None):
        """bsc_mbias_read: (counts[2][2][3][n_cycles][2] u64, totals[8]) of the context's accumulator, n_cycles that of the block_mbias_rawdev
        calls that made it.  params (optional): the n_cycles the caller expects — ValueError where the accumulator's differs.  The library
        copies the accumulator's own size whatever the caller believes, so the copy lands in an array of the largest table and is cut."""
        made = getattr(self, "_mbias_cycles", None)
        if params is not None and made is not None and int(self._mb_params(params).n_cycles) != made:
            raise ValueError("the accumulator has %d cycles, not %d" % (made, int(self._mb_params(params).n_cycles)))
        room = np.zeros(12 * 1024 * 2, dtype=np.uint64)  # BSC_MBIAS_N_BINS * BSC_MBIAS_MAX_CYCLES * 2
        tot = (C.c_uint64 * 8)()
        _check(self._L.bsc_mbias_read(self._h, _ptr(room), tot))
        n = made if made is not None else int(self._mb_params(params).n_cycles)
        return room[: 12 * n * 2].reshape(2, 2, 3, n, 2).copy(), tuple(int(v) for v in tot)

    def mbias_reset(self):
        """bsc_mbias_reset: drops the context's M-bias accumulator."""
        _check(self._L.bsc_mbias_reset(self._h))
        self._mbias_cycles = None

    # -- the epiallele table (csrc/epidev.hip) ----------------------------------------------------------------
    @staticmethod
    def _epi_params(params):
        if params is None:
            return _lib.EpiParams()
        if isinstance(params, _lib.EpiParams):
            return params
        return _lib.EpiParams(**params)

    def epi_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_win, win_cap, d_n_win, d_totals, params=None, stream=None):
        """bsc_epi_device: the inputs of cpg_reads_device -> one bsc_epi_window per window of four consecutive reference CpGs in
        d_win[<= win_cap], their count (a device u64) in d_n_win and the eight totals in d_totals (asynchronous on `stream`)."""
        ep = self._epi_params(params)
        _check(self._L.bsc_epi_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, C.byref(ep), d_win, win_cap, d_n_win, d_totals, stream))

    def epi_text_device(self, d_win, d_n_win, max_win, contig, d_out, out_cap, d_totals2, params=None, stream=None):
        """bsc_epi_text_device: the table's lines of d_win[min(*d_n_win, max_win)] -> d_out[<= out_cap]; d_totals2: {bytes, lines}."""
        ep = self._epi_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        _check(self._L.bsc_epi_text_device(self._h, d_win, d_n_win, max_win, name, C.byref(ep), d_out, out_cap, d_totals2, stream))

    def block_epi_kept(self, contig, params=None, cap=None):
        """bsc_block_epi_kept + bsc_epi_stream_read: the epiallele table of the block the last *_keep call called, from the prepared
        templates, reads and reference codes it left on the device.  params: a _lib.EpiParams, a dict of its fields, or None ({10, 0}).
        Returns (bytes, lines, totals[8]).  cap: the room on the device (default: asked for and given on a second call)."""
        ep = self._epi_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        nb, nl, tot = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
        room = 1 << 16 if cap is None else int(cap)
        rc = self._L.bsc_block_epi_kept(self._h, name, C.byref(ep), room, C.byref(nb), C.byref(nl), tot)
        if rc == -1 and nb.value > room and cap is None:
            room = int(nb.value)
            rc = self._L.bsc_block_epi_kept(self._h, name, C.byref(ep), room, C.byref(nb), C.byref(nl), tot)
        _check(rc)
        return self.epi_stream_read(0, nb.value), int(nl.value), tuple(int(v) for v in tot)

    def epi_stream_read(self, off, n):
        """bsc_epi_stream_read: bytes [off, off + n) of the table the last block_epi_kept left on the device."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        _check(self._L.bsc_epi_stream_read(self._h, int(off), int(n), _ptr(out)))
        if n:
            self.synchronize()
        return out[: int(n)].tobytes()

    # -- the per-read CpG pattern table, PAT (csrc/patdev.hip) -----------------------------------------------
    @staticmethod
    def _pat_params(params):
        if params is None:
            return _lib.PatParams()
        if isinstance(params, _lib.PatParams):
            return params
        return _lib.PatParams(**params)

    def pat_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_rec, rec_cap, d_n_rec, d_totals, params=None, stream=None):
        """bsc_pat_device: the inputs of cpg_reads_device -> one bsc_pat_rec per distinct (idx, pattern) of the block in d_rec[<= rec_cap], in
        the table's order, their count (a device u64) in d_n_rec and the eight totals in d_totals (queued on `stream`; waits once, for the
        slot count)."""
        pp = self._pat_params(params)
        _check(self._L.bsc_pat_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, C.byref(pp), d_rec, rec_cap, d_n_rec, d_totals, stream))

    def pat_text_device(self, d_rec, d_n_rec, max_rec, contig, index_base, d_out, out_cap, d_totals2, params=None, stream=None):
        """bsc_pat_text_device: the table's lines of d_rec[min(*d_n_rec, max_rec)] -> d_out[<= out_cap]; d_totals2: {bytes, lines}."""
        pp = self._pat_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        _check(self._L.bsc_pat_text_device(self._h, d_rec, d_n_rec, max_rec, name, int(index_base), C.byref(pp), d_out, out_cap, d_totals2, stream))

    def block_pat_kept(self, contig, params=None, index_base=0, cap=None, guess=None):
        """bsc_block_pat_kept + bsc_pat_stream_read: the PAT table of the block the last *_keep call called, from the prepared templates,
        reads and reference codes it left on the device.  params: a _lib.PatParams, a dict of its fields, or None ({1, 0}).  index_base: the
        sites of the contig in front of the block's first position.  Returns (bytes, lines, totals[8]).  cap: the room on the device
        (default: `guess` bytes, or 64 KiB, and where that is too small the room the first call asks for on a second call, which walks and
        sorts the block again: a caller that knows the last block's need passes a guess above it)."""
        pp = self._pat_params(params)
        name = contig.encode() if isinstance(contig, str) else contig
        nb, nl, tot = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 8)()
        room = (int(guess) if guess else 1 << 16) if cap is None else int(cap)
        rc = self._L.bsc_block_pat_kept(self._h, name, C.byref(pp), int(index_base), room, C.byref(nb), C.byref(nl), tot)
        if rc == -1 and nb.value > room and cap is None:
            room = int(nb.value)
            rc = self._L.bsc_block_pat_kept(self._h, name, C.byref(pp), int(index_base), room, C.byref(nb), C.byref(nl), tot)
        _check(rc)
        return self.pat_stream_read(0, nb.value), int(nl.value), tuple(int(v) for v in tot)

    def pat_stream_read(self, off, n):
        """bsc_pat_stream_read: bytes [off, off + n) of the table the last block_pat_kept left on the device."""
        out = np.empty(max(int(n), 1), dtype=np.uint8)
        _check(self._L.bsc_pat_stream_read(self._h, int(off), int(n), _ptr(out)))
        if n:
            self.synchronize()
        return out[: int(n)].tobytes()

    # -- the per-region fragment methylation summary (csrc/fragdev.hip) ------------------------------------------
    @staticmethod
    def _frag_params(params):
        if params is None:
            return _lib.FragParams()
        if isinstance(params, _lib.FragParams):
            return params
        return _lib.FragParams(**params)

    def frag_attach(self, regions):
        """bsc_frag_attach: the regions of ONE contig — (start, end) pairs, 0-based and half-open as in BED, sorted by (start, end) —
        uploaded, their eight accumulators each zeroed.  An empty list detaches.  Refused (BscError) when unsorted or start > end: the
        previous attachment then stays.  The accumulators are separate from meth_regions_attach's.  Returns the count."""
        r = self._regions_array(regions)
        _check(self._L.bsc_frag_attach(self._h, _ptr(r) if len(r) else None, len(r)))
        self._n_frag_regions = len(r)
        return len(r)

    def frag_device(self, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, d_totals, params=None, stream=None):
        """bsc_frag_device: the inputs of cpg_reads_device added into the attached regions' accumulators {frags, U, X, M, K, Mm, disc,
        short}; the call's eight totals in d_totals (asynchronous on `stream`)."""
        fp = self._frag_params(params)
        _check(self._L.bsc_frag_device(self._h, d_tpl, nr, d_seq, seq_bytes, x, y, d_ref, C.byref(fp), d_totals, stream))

    def block_frag_kept(self, params=None):
        """bsc_block_frag_kept: the block the last *_keep call called, added into the attached regions' accumulators from the prepared
        templates, reads and reference codes it left on the device.  params: a _lib.FragParams, a dict of its fields, or None
        ({3, 25, 75, 0}).  Returns the call's eight totals."""
        fp = self._frag_params(params)
        tot = (C.c_uint64 * 8)()
        _check(self._L.bsc_block_frag_kept(self._h, C.byref(fp), tot))
        return tuple(int(v) for v in tot)

    def frag_read(self):
        """bsc_frag_read: the accumulators as uint64[n, 8] — per attached region {frags, U, X, M, K, Mm, disc, short} (waits)."""
        n = getattr(self, "_n_frag_regions", 0)
        acc = np.zeros((n, 8), dtype=np.uint64)
        _check(self._L.bsc_frag_read(self._h, _ptr(acc) if n else None, n))
        return acc

    def frag_reset(self):
        """bsc_frag_reset: the accumulators zeroed, the regions stay."""
        _check(self._L.bsc_frag_reset(self._h))

    def blocks_records(self, blocks, ref, out=None, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None, with_stats=False,
                       submit_only=False):
        """Several blocks in one launch sequence (bsc_blocks_records): blocks = [(templates, seq, x, y), ...] in genome order;
        ref = their reference codes, a list of uint8[y - x + 3] arrays (or one array, block after block); dbsnp likewise
        (y - x + 1 each) or None.  Returns (VCF_REC[n_written] of all blocks, block after block; records written per block) —
        the records of block_records() called on the blocks one after another.  submit_only: queue and return; then
        blocks_records_fetch()."""
        from .abi import BLOCK_DESC

        tpls, seqs, desc, off = [], [], np.zeros(len(blocks), dtype=BLOCK_DESC), 0
        for i, (t, sq, x, y) in enumerate(blocks):
            t = np.array(t, dtype=TEMPLATE)  # a copy: the read offsets become offsets into the joined read buffer
            sq = np.ascontiguousarray(sq, dtype=np.uint8)
            t["off"] += np.uint64(off)
            off += sq.size
            tpls.append(t)
            seqs.append(sq)
            desc[i] = (x, y, len(t), 0)
        tpl = np.concatenate(tpls) if tpls else np.zeros(0, dtype=TEMPLATE)
        seq = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
        sizes = [int(y) - int(x) + 1 for _, _, x, y in blocks]
        refs = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in ref]) if isinstance(ref, (list, tuple)) else ref, dtype=np.uint8)
        if min(sizes) > 0 and len(refs) != sum(sizes) + 2 * len(sizes):  # (a block with y < x is the library's to refuse)
            raise ValueError("ref must hold y - x + 3 codes per block")
        db = None
        if dbsnp is not None:
            db = np.ascontiguousarray(np.concatenate([np.asarray(d, dtype=np.uint8) for d in dbsnp]) if isinstance(dbsnp, (list, tuple)) else dbsnp, dtype=np.uint8)
            if min(sizes) > 0 and len(db) != sum(sizes):
                raise ValueError("dbsnp must hold y - x + 1 flags per block")
        if out is None:
            out = np.zeros(sum(sizes), dtype=VCF_REC)
        elif out.dtype != VCF_REC or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("out must be a writable C-contiguous VCF_REC array")
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        _check(self._L.bsc_blocks_records_submit(self._h, _ptr(desc), len(desc), _ptr(tpl), _ptr(seq), seq.size, _ptr(refs),
                                                 None if db is None else _ptr(db), C.byref(p), 1 if with_stats else 0, _ptr(out), len(out)))
        self._pending_blocks = (out, len(desc))
        return None if submit_only else self.blocks_records_fetch()

    def blocks_bcf(self, blocks, ref, rid, names=None, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None, with_stats=False, cap=None, ids=None,
                   inplace=False):
        """Several blocks in one launch sequence, their BCF bytes back as ONE stream (bsc_blocks_bcf_submit[_inplace] + _fetch): blocks, ref and
        dbsnp as blocks_records takes them; names = the table of all the blocks' flagged positions.  Returns (bytes, n_records): the streams of
        block_bcf() called on the blocks one after another, concatenated."""
        from .abi import BLOCK_DESC

        tpls, seqs, desc, off = [], [], np.zeros(len(blocks), dtype=BLOCK_DESC), 0
        for i, (t, sq, x, y) in enumerate(blocks):
            t = np.array(t, dtype=TEMPLATE)
            sq = np.ascontiguousarray(sq, dtype=np.uint8)
            t["off"] += np.uint64(off)
            off += sq.size
            tpls.append(t)
            seqs.append(sq)
            desc[i] = (x, y, len(t), 0)
        tpl = np.concatenate(tpls) if tpls else np.zeros(0, dtype=TEMPLATE)
        seq = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
        sizes = [int(y) - int(x) + 1 for _, _, x, y in blocks]
        refs = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in ref]) if isinstance(ref, (list, tuple)) else ref, dtype=np.uint8)
        db = None
        if dbsnp is not None:
            db = np.ascontiguousarray(np.concatenate([np.asarray(d, dtype=np.uint8) for d in dbsnp]) if isinstance(dbsnp, (list, tuple)) else dbsnp, dtype=np.uint8)
        if ids is None:
            ids = _lib.BcfIds()
            self._L.bsc_bcf_default_ids(C.byref(ids))
        nm, keep = self._bcf_names(names)
        cap_given = cap
        cap = 64 + 192 * max(sum(sizes), 1) if cap is None else int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        nb, nr = C.c_uint64(0), C.c_uint64(0)
        fn = self._L.bsc_blocks_bcf_submit_inplace if inplace else self._L.bsc_blocks_bcf_submit
        _check(fn(self._h, _ptr(desc), len(desc), _ptr(tpl), _ptr(seq), seq.size, _ptr(refs), None if db is None else _ptr(db), C.byref(p),
                  1 if with_stats else 0, rid, C.byref(ids), None if nm is None else C.addressof(nm), _ptr(out), cap))
        rc = self._L.bsc_blocks_bcf_fetch(self._h, C.byref(nb), C.byref(nr))
        if rc == -1 and nb.value > cap and cap_given is None:
            cap = int(nb.value)
            out = np.empty(cap, dtype=np.uint8)
            rc = self._L.bsc_block_bcf_again(self._h, _ptr(out), cap, C.byref(nb), C.byref(nr))
        _check(rc)
        del keep, tpl, seq, refs, db, desc
        return out[: nb.value].tobytes(), nr.value

    def blocks_records_joined(self, desc, tpl, seq, ref, out, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None,
                              with_stats=False, inplace=False, submit_only=False):
        """bsc_blocks_records_submit[_inplace] on arrays that are already joined as the C ABI wants them (what a C host that
        flattens its blocks into one set of buffers holds): desc BLOCK_DESC[n_blocks], tpl TEMPLATE[sum nr] with off[] into `seq`,
        ref = the blocks' y - x + 3 codes one block after another.  inplace: no staging copy (the arrays — page-locked ones from
        PinnedBuffer make the upload a DMA — must stay unchanged until the fetch)."""
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        fn = self._L.bsc_blocks_records_submit_inplace if inplace else self._L.bsc_blocks_records_submit
        _check(fn(self._h, _ptr(desc), len(desc), _ptr(tpl), _ptr(seq), seq.size, _ptr(ref), None if dbsnp is None else _ptr(dbsnp),
                  C.byref(p), 1 if with_stats else 0, _ptr(out), len(out)))
        self._pending_blocks = (out, len(desc))
        self._pending_in = (desc, tpl, seq, ref, dbsnp)
        return None if submit_only else self.blocks_records_fetch()

    def blocks_records_fetch(self):
        out, nb = getattr(self, "_pending_blocks", None) or (None, 0)
        if out is None:
            raise BscError(-1, "blocks_records_fetch: no blocks were submitted")
        self._pending_blocks = None
        cnt, per = C.c_uint64(0), np.zeros(nb, dtype=np.uint64)
        _check(self._L.bsc_blocks_records_fetch(self._h, C.byref(cnt), _ptr(per)))
        return out[: cnt.value], per

    def block_records_submit(self, templates, seq, x, y, ref, out, all_positions=False, reg_start=1, reg_stop=0xFFFFFFFF, dbsnp=None,
                             with_stats=False, inplace=False):
        """Queue one block (reads -> packed records into `out`, a VCF_REC array that must stay alive until the fetch) and
        return at once; the inputs may be reused immediately — unless inplace (bsc_block_records_submit_inplace): then they
        are read where they lie, no staging copy, and must stay unchanged until the fetch.  block_records_fetch() completes it."""
        templates = np.ascontiguousarray(templates, dtype=TEMPLATE)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        n = int(y) - int(x) + 1
        if len(ref) != n + 2:
            raise ValueError("ref must have y - x + 3 entries (x .. y + 2)")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        if db is not None and len(db) != n:
            raise ValueError("dbsnp must have y - x + 1 entries")
        if out.dtype != VCF_REC or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("out must be a writable C-contiguous VCF_REC array")
        p = _lib.VcfParams(1 if all_positions else 0, reg_start, reg_stop)
        fn = self._L.bsc_block_records_submit_inplace if inplace else self._L.bsc_block_records_submit
        _check(fn(self._h, _ptr(templates), len(templates), _ptr(seq), seq.size, x, y, _ptr(ref), None if db is None else _ptr(db),
                  C.byref(p), 1 if with_stats else 0, _ptr(out), len(out)))
        self._pending_rec = out
        self._pending_in = (templates, seq, ref, db) if inplace else None  # kept alive until the fetch

    def block_records_fetch(self):
        """Wait for the submitted block: VCF_REC[n_written] (a view of the array named at submit)."""
        out = getattr(self, "_pending_rec", None)
        if out is None:
            raise BscError(-1, "block_records_fetch: no block was submitted")
        self._pending_rec = None
        cnt = C.c_uint64(0)
        try:
            _check(self._L.bsc_block_records_fetch(self._h, C.byref(cnt)))
        finally:
            self._pending_in = None
        return out[: cnt.value]

    def vcf_compact_device(self, d_core, d_gtm, stride, n, d_out, out_cap, d_count, d_dbsnp=None, stream=None):
        _check(self._L.bsc_vcf_compact_device(self._h, d_core, d_gtm, stride, d_dbsnp, n, d_out, out_cap, d_count, stream))

    # -- site statistics (the sums of the reference's bs_stats; the payload of a sharded run's all-reduce) -----
    def vcf_stats(self, core, gtm, dbsnp=None):
        """Add the statistics of one block (VCF_CORE[n] from vcf_records + the GT_METH[n] behind them) to the context."""
        core = np.ascontiguousarray(core, dtype=VCF_CORE)
        gtm = np.ascontiguousarray(gtm)
        stride = gtm.dtype.itemsize if gtm.ndim == 1 else gtm.shape[1]
        if len(gtm) != len(core):
            raise ValueError("core and gtm differ in length")
        db = None if dbsnp is None else np.ascontiguousarray(dbsnp, dtype=np.uint8)
        _check(self._L.bsc_vcf_stats(self._h, _ptr(core), _ptr(gtm), stride, None if db is None else _ptr(db), len(core)))

    def vcf_stats_device(self, d_core, d_gtm, stride, n, d_dbsnp=None, stream=None):
        _check(self._L.bsc_vcf_stats_device(self._h, d_core, d_gtm, stride, d_dbsnp, n, stream))

    # -- a contig of the dbSNP index kept in HBM (csrc/dbsnpdev.hip) --------------------------------------
    def dbsnp_attach(self, db):
        """bsc_dbsnp_attach: snapshot the contig loaded in `db` (a dbsnp.DbSnpIndex) into the context; while it is attached the
        block_*_rawdev entries take dbsnp=None / names=None as "from the attachment".  Returns the number of entries."""
        n = C.c_uint64(0)
        _check(self._L.bsc_dbsnp_attach(self._h, db._h, C.byref(n)))
        return n.value

    def dbsnp_detach(self):
        _check(self._L.bsc_dbsnp_detach(self._h))

    def dbsnp_count(self, x0, n):
        """bsc_dbsnp_count: (names, name bytes) of positions x0 .. x0 + n - 1 of the attached contig — host arithmetic."""
        k, nb = C.c_uint32(0), C.c_uint64(0)
        _check(self._L.bsc_dbsnp_count(self._h, x0, n, C.byref(k), C.byref(nb)))
        return k.value, nb.value

    def dbsnp_flags_device(self, x0, n, d_out, stream=None):
        """bsc_dbsnp_flags_device: d_out[n] (device pointer, any alignment) = DbSnpIndex.flags(x0, n); asynchronous on `stream`."""
        _check(self._L.bsc_dbsnp_flags_device(self._h, x0, n, d_out, stream))

    def dbsnp_names_device(self, x0, n, d_pos, d_off, d_bytes, cap_names, cap_bytes, stream=None):
        """bsc_dbsnp_names_device: the three arrays of DbSnpIndex.names(x0, n) into device memory sized by dbsnp_count()."""
        _check(self._L.bsc_dbsnp_names_device(self._h, x0, n, d_pos, d_off, d_bytes, cap_names, cap_bytes, stream))

    def site_stats(self):
        """The accumulated bsc_site_stats as a numpy record (SITE_STATS)."""
        out = np.zeros(1, dtype=SITE_STATS)
        _check(self._L.bsc_get_site_stats(self._h, _ptr(out)))
        return out[0]

    def set_gc_bins(self, d_gc, n_bins, start_pos):
        """GC bins of the contig being walked (device pointer, see `gc_bins`); None switches the GC table off."""
        _check(self._L.bsc_set_gc_bins(self._h, d_gc, n_bins, start_pos))

    def set_gc_bins_host(self, bins, start_pos):
        """The same from a host array (the context keeps its own device copy); None / empty switches the table off."""
        if bins is None or len(bins) == 0:
            _check(self._L.bsc_set_gc_bins_host(self._h, None, 0, 0))
            return
        b = np.ascontiguousarray(bins, dtype=np.uint8)
        _check(self._L.bsc_set_gc_bins_host(self._h, _ptr(b), b.size, start_pos))

    def gc_stats(self):
        """Positions by [total depth][G+C count of their 100-base bin]: the report's "GC" object, (4096, 101) uint64."""
        out = np.zeros((4096, 101), dtype=np.uint64)
        _check(self._L.bsc_get_gc_stats(self._h, _ptr(out)))
        return out

    def site_totals(self):
        """snps, indels, multi, dbSNP_sites, dbSNP_var, CpG_ref, CpG_nonref as a (7, 2) array [all, passed]: the
        reference's per-contig copy (gt_ctg_stats) is the difference of two reads."""
        out = np.zeros(14, dtype=np.uint64)
        _check(self._L.bsc_get_site_totals(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out.reshape(7, 2)

    def reset_site_stats(self):
        _check(self._L.bsc_reset_site_stats(self._h))

    # -- device-resident blocks (raw device pointers, e.g. torch tensor .data_ptr()) ---------------
    def call_sites_device(self, d_cts, d_ref, n, d_out, d_skip, out_stride=200, stream=None):
        _check(self._L.bsc_call_sites_device(self._h, d_cts, d_ref, n, d_out, out_stride, d_skip, stream))

    def synth_device(self, seed, first_site, n, coverage, d_cts, d_ref, flags=0, stream=None):
        _check(self._L.bsc_synth_pileup_device(self._h, seed, first_site, n, coverage, flags, d_cts, d_ref, stream))

    def stream_probe_ms(self, d_cts, d_ref, n, d_out, d_skip, reps=5, stream=None):
        """Best-of-reps time of the no-arithmetic copy kernel with call_sites_device's traffic (OVERWRITES d_out / d_skip)."""
        ms = C.c_float(0)
        _check(self._L.bsc_stream_probe_ms(self._h, d_cts, d_ref, n, d_out, d_skip, reps, stream, C.byref(ms)))
        return ms.value

    def set_reads_fused(self, fused=True):
        """reads -> records in ONE kernel (True) or through a pile-up in HBM (False, the default: faster)."""
        _check(self._L.bsc_set_reads_fused(self._h, 1 if fused else 0))

    def debug_fail_summary_alloc(self, on=True):
        """test hook: the two-kernel form's summaries cannot be allocated (bsc_debug_fail_summary_alloc)"""
        _check(self._L.bsc_debug_fail_summary_alloc(self._h, 1 if on else 0))

    def set_profiling(self, enable=True):
        _check(self._L.bsc_set_profiling(self._h, 1 if enable else 0))

    def last_kernel_ms(self):
        """(calling kernel ms, Fisher kernel ms) of the most recent launch, from HIP events on its stream."""
        a, b = C.c_float(), C.c_float()
        _check(self._L.bsc_last_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_ms_history(self, n):
        """[(calling kernel ms, Fisher kernel ms)] of the last n launches, oldest first (the library keeps the last 32):
        read after a timed loop, so that the loop itself never waits on an event."""
        out = []
        for age in range(min(int(n), 32) - 1, -1, -1):
            a, b = C.c_float(), C.c_float()
            _check(self._L.bsc_kernel_ms_history(self._h, age, C.byref(a), C.byref(b)))
            out.append((a.value, b.value))
        return out

    def synchronize(self):
        _check(self._L.bsc_synchronize(self._h))

    # -- counters ---------------------------------------------------------------------------------
    def stats(self):
        s = _lib.Stats()
        _check(self._L.bsc_get_stats(self._h, C.byref(s)))
        return {
            "sites": int(s.sites),
            "covered": int(s.covered),
            "gt_hist": [int(x) for x in s.gt_hist],
            "het_calls": int(s.het_calls),
        }

    def stats_vector(self):
        """The counters as a flat int64 vector (the block ranks all-reduce at the end of a sharded run)."""
        s = self.stats()
        return np.array([s["sites"], s["covered"]] + s["gt_hist"] + [s["het_calls"]], dtype=np.int64)

    def reset_stats(self):
        _check(self._L.bsc_reset_stats(self._h))


def synth_pileup_host(seed, first_site, n, coverage, flags=0):
    """Host twin of the device generator (bsc_synth_pileup_host): identical bits, no GPU needed."""
    L = _lib.load()
    pile = np.zeros(n, dtype=PILEUP)
    ref = np.zeros(n, dtype=np.uint8)
    _check(L.bsc_synth_pileup_host(seed, first_site, n, coverage, flags, _ptr(pile), _ptr(ref)))
    return pile, ref


def synth_reads_host(seed, x, n_sites, coverage, flags=0):
    """Synthetic read pairs over positions x .. x+n_sites-1 (bsc_synth_reads_host) -> (TEMPLATE[nt], seq uint8[])."""
    L = _lib.load()
    max_t = int(n_sites) * int(coverage) // 150 + 64
    cap = max_t * 200 + 1024
    tpl = np.zeros(max_t, dtype=TEMPLATE)
    seq = np.zeros(cap, dtype=np.uint8)
    used = C.c_uint64(0)
    nt = L.bsc_synth_reads_host(seed, x, n_sites, coverage, flags, _ptr(tpl), max_t, _ptr(seq), cap, C.byref(used))
    if nt < 0:
        raise BscError(-3, "bsc_synth_reads_host: buffer too small")
    return tpl[:nt].copy(), seq[: used.value].copy()


def synth_ref_host(seed, first_site, n, flags=0):
    """Reference codes of the synthetic genome (the ref[] of synth_pileup_host without the pile-ups)."""
    _, ref = synth_pileup_host(seed, first_site, n, 0, flags)
    return ref


class PinnedBuffer:
    """A page-locked host allocation (bsc_alloc_host) viewed as a numpy array; freed with the object."""

    def __init__(self, shape, dtype):
        self._L = _lib.load()
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) if not isinstance(shape, int) else int(shape)
        self.nbytes = max(n * dt.itemsize, 1)
        self._p = self._L.bsc_alloc_host(self.nbytes)
        if not self._p:
            raise BscError(-3, self._L.bsc_last_error().decode("utf-8", "replace"))
        raw = (C.c_uint8 * self.nbytes).from_address(self._p)
        self.array = np.frombuffer(raw, dtype=np.uint8, count=n * dt.itemsize).view(dt).reshape(shape)

    def free(self):
        if getattr(self, "_p", None):
            self.array = None
            self._L.bsc_free_host(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def gc_bins(codes):
    """ctg_stats->gc of a contig (src/read_reference.c:44-131) from its reference codes 0..4 (position 1 first):
    (start_pos, uint8 bins)."""
    L = _lib.load()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.zeros(codes.size // 100 + 1, dtype=np.uint8)
    start, nb = C.c_uint32(0), C.c_uint64(0)
    _check(L.bsc_gc_bins(_ptr(codes), codes.size, C.byref(start), _ptr(out), out.size, C.byref(nb)))
    return int(start.value), out[: nb.value].copy()


class ReadProfile:
    """bs_stats.meth_profile: the non-CpG read profile accumulated over blocks by `prepare_templates(..., profile=...)`
    (src/meth_profile.c).  `counts[i + 1]` = the four counts of read position i; `used` = the reference vector's length."""

    def __init__(self, cap=4096):
        self.counts = np.zeros((cap, 4), dtype=np.uint64)
        self.used = 0

    def reported(self):
        """What the report lists: elements 0 .. used - 1 (the report skips element 0 itself)."""
        return self.counts[: self.used]


def prepare_templates(raw, seq, misms, left_trim=(0, 0), right_trim=(0, 0), min_qual=20, profile=None, x=None, ref=None):
    """Read pre-processing on the host (bsc_prepare_templates; src/process_template.c:36-111): RAW_TEMPLATE[nr] + read
    bytes + MISMS[] -> (TEMPLATE[nr], prepared read bytes, PREP_STATS record).  No GPU involved.  With `profile` (a
    ReadProfile), the block start `x` and the block's reference codes `ref` (x .. y + 2) the templates also feed the
    non-CpG read profile."""
    from .abi import MISMS, PREP_PARAMS, PREP_STATS, RAW_TEMPLATE

    L = _lib.load()
    raw = np.ascontiguousarray(raw, dtype=RAW_TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    misms = np.ascontiguousarray(misms, dtype=MISMS)
    par = np.zeros(1, dtype=PREP_PARAMS)
    par["left_trim"][0], par["right_trim"][0], par["min_qual"][0] = left_trim, right_trim, min_qual
    # room for the prepared bytes: the reads plus what their listed insertions can add; a size field larger than the block's
    # bytes is damage (the entry refuses it), not a reason to reserve gigabytes
    cap = int(seq.size) + int(np.minimum(misms["size"][misms["type"] == 1].astype(np.uint64), np.uint64(seq.size)).sum()) + 16
    out_tpl = np.zeros(len(raw), dtype=TEMPLATE)
    out_seq = np.zeros(cap, dtype=np.uint8)
    used = C.c_uint64(0)
    st = np.zeros(1, dtype=PREP_STATS)
    if profile is None:
        _check(L.bsc_prepare_templates(_ptr(raw), len(raw), _ptr(seq), seq.size, _ptr(misms), len(misms), _ptr(par), _ptr(out_tpl),
                                       _ptr(out_seq), cap, C.byref(used), _ptr(st)))
    else:
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        pf = _lib.ReadProfile(ref.ctypes.data, int(x), ref.size, profile.counts.ctypes.data, profile.counts.shape[0], profile.used)
        _check(L.bsc_prepare_templates_profile(_ptr(raw), len(raw), _ptr(seq), seq.size, _ptr(misms), len(misms), _ptr(par),
                                               _ptr(out_tpl), _ptr(out_seq), cap, C.byref(used), _ptr(st), C.byref(pf)))
        profile.used = int(pf.used)
    return out_tpl, out_seq[: used.value].copy(), st[0]


def cpg_reads_sites_host(tpl, seq, x, y, ref, min_qual=20, params=None, cap=None):
    """The host form of the read-level CpG table (bsc_cpg_reads_sites_host; csrc/cpgreads.c): prepared TEMPLATE[nr] + their read bytes, the
    block x .. y and its reference codes (x .. y + 2) -> (SITE records[min(count, cap)], count, totals[8]).  No GPU involved.  cap: the
    room (default: every site)."""
    from .cpgreads import SITE

    L = _lib.load()
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    if ref.size < int(y) - int(x) + 2:
        raise ValueError("ref must hold the codes of x .. y + 1 at least")
    cp = SiteCaller._cr_params(params)
    room = int(y) - int(x) + 1 if cap is None else int(cap)
    out = np.zeros(max(room, 1), dtype=SITE)
    n, tot = C.c_uint64(0), (C.c_uint64 * 8)()
    _check(L.bsc_cpg_reads_sites_host(_ptr(tpl), len(tpl), _ptr(seq), seq.size, int(x), int(y), _ptr(ref), int(min_qual), C.byref(cp), _ptr(out), room,
                                      C.byref(n), tot))
    return out[: min(int(n.value), room)].copy(), int(n.value), tuple(int(v) for v in tot)


def cpg_reads_format_host(contig, recs, params=None, cap=None):
    """bsc_cpg_reads_format: the table's lines of SITE records -> (bytes, lines).  cap: the room (default: asked for first); a room too
    small gives (None, the length needed)."""
    from .cpgreads import SITE

    L = _lib.load()
    recs = np.ascontiguousarray(recs, dtype=SITE)
    cp = SiteCaller._cr_params(params)
    name = contig.encode() if isinstance(contig, str) else contig
    t2 = (C.c_uint64 * 2)()
    if cap is None:
        need = L.bsc_cpg_reads_format(name, _ptr(recs), len(recs), C.byref(cp), None, 0, t2)
        if need < 0:
            _check(int(need))
        cap = int(need)
    buf = np.full(max(int(cap), 1) + 8, 0xA5, dtype=np.uint8)
    got = L.bsc_cpg_reads_format(name, _ptr(recs), len(recs), C.byref(cp), _ptr(buf), int(cap), t2)
    if got < 0:
        _check(int(got))
    assert (buf[int(cap) :] == 0xA5).all() and int(t2[0]) == got
    if got > int(cap):
        assert (buf == 0xA5).all()
        return None, int(got)
    return buf[:got].tobytes(), int(t2[1])


def asm_pairs_host(tpl, seq, x, y, ref, core, emit=None, lfact=None, min_qual=20, params=None, cap=None):
    """The host form of the allele-specific methylation table (bsc_asm_pairs_host; csrc/asm.c): prepared TEMPLATE[nr] + their read bytes, the
    block x .. y, its reference codes (x .. y + 2), its VCF_CORE records and (optionally) its emit bytes -> (PAIR records[min(count, cap)],
    count, totals[8]).  lfact: ln k! for k < 256 (default: asm.lfact_table(), which bsc_get_tables equals).  No GPU involved.  cap: the room
    (default: asked for first)."""
    from .asm import PAIR, lfact_table

    L = _lib.load()
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    core = np.ascontiguousarray(core, dtype=VCF_CORE)
    n_pos = int(y) - int(x) + 1
    if ref.size < n_pos + 1 or len(core) != n_pos:
        raise ValueError("ref must hold the codes of x .. y + 1 at least, core one record per position")
    if emit is not None:
        emit = np.ascontiguousarray(emit, dtype=np.uint8)
        if emit.size != n_pos:
            raise ValueError("emit must hold one byte per position")
    lf = np.ascontiguousarray(lfact_table() if lfact is None else lfact, dtype=np.float64)
    assert lf.size == 256
    cp = SiteCaller._asm_params(params)
    n, tot = C.c_uint64(0), (C.c_uint64 * 8)()
    args = (_ptr(tpl), len(tpl), _ptr(seq), seq.size, int(x), int(y), _ptr(ref), int(min_qual), _ptr(core), None if emit is None else _ptr(emit), _ptr(lf),
            C.byref(cp))
    if cap is None:
        _check(L.bsc_asm_pairs_host(*args, None, 0, C.byref(n), tot))
        cap = int(n.value)
    room = int(cap)
    out = np.zeros(max(room, 1), dtype=PAIR)
    _check(L.bsc_asm_pairs_host(*args, _ptr(out), room, C.byref(n), tot))
    return out[: min(int(n.value), room)].copy(), int(n.value), tuple(int(v) for v in tot)


def asm_format_host(contig, recs, params=None, cap=None):
    """bsc_asm_format: the table's lines of PAIR records -> (bytes, lines).  cap: the room (default: asked for first); a room too small gives
    (None, the length needed)."""
    from .asm import PAIR

    L = _lib.load()
    recs = np.ascontiguousarray(recs, dtype=PAIR)
    cp = SiteCaller._asm_params(params)
    name = contig.encode() if isinstance(contig, str) else contig
    t2 = (C.c_uint64 * 2)()
    if cap is None:
        need = L.bsc_asm_format(name, _ptr(recs), len(recs), C.byref(cp), None, 0, t2)
        if need < 0:
            _check(int(need))
        cap = int(need)
    buf = np.full(max(int(cap), 1) + 8, 0xA5, dtype=np.uint8)
    got = L.bsc_asm_format(name, _ptr(recs), len(recs), C.byref(cp), _ptr(buf), int(cap), t2)
    if got < 0:
        _check(int(got))
    assert (buf[int(cap) :] == 0xA5).all() and int(t2[0]) == got
    if got > int(cap):
        assert (buf == 0xA5).all()
        return None, int(got)
    return buf[:got].tobytes(), int(t2[1])


def asm_fisher_p_host(tables, lfact=None):
    """bsc_asm_fisher_p over the rows of an n x 4 integer array (each >= 0, a row's sum <= 46340) -> float64[n]: the z of the rule's AQ."""
    from .asm import lfact_table

    L = _lib.load()
    c = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 4)
    if len(c) and (c.min() < 0 or c.sum(axis=1).max() > 46340):
        raise ValueError("counts must be >= 0 and a table's sum <= 46340")
    lf = np.ascontiguousarray(lfact_table() if lfact is None else lfact, dtype=np.float64)
    return np.array([L.bsc_asm_fisher_p(_ptr(row), _ptr(lf)) for row in c], dtype=np.float64)


def mbias_host(raw, seq, misms, x, y, ref, min_qual=20, params=None, counts=None, totals=None):
    """The host form of the M-bias table (bsc_mbias_host; csrc/mbias.c): RAW_TEMPLATE[nr], their read bytes and MISMS lists, the block x .. y
    and its reference codes (x .. y + 2) ADDED into counts[2][2][3][n_cycles][2] / totals[8] (made of zeros when None).  No GPU involved.
    Returns (counts, totals)."""
    from .abi import MISMS, RAW_TEMPLATE

    L = _lib.load()
    raw = np.ascontiguousarray(raw, dtype=RAW_TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    misms = np.ascontiguousarray(misms, dtype=MISMS)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    if int(y) >= int(x) and ref.size < int(y) - int(x) + 3:
        raise ValueError("ref must hold the codes of x .. y + 2")
    mp = SiteCaller._mb_params(params)
    if counts is None:
        counts = np.zeros((2, 2, 3, int(mp.n_cycles) if 1 <= int(mp.n_cycles) <= 1024 else 1, 2), dtype=np.uint64)  # (a refused n_cycles: any table)
    if totals is None:
        totals = np.zeros(8, dtype=np.uint64)
    assert counts.dtype == np.uint64 and counts.flags.c_contiguous and totals.dtype == np.uint64
    _check(L.bsc_mbias_host(_ptr(raw), len(raw), _ptr(seq), seq.size, _ptr(misms), len(misms), int(x), int(y), _ptr(ref), int(min_qual), C.byref(mp),
                            _ptr(counts), totals.ctypes.data_as(C.POINTER(C.c_uint64))))
    return counts, totals


def mbias_format_host(counts, cap=None):
    """bsc_mbias_format: the table's text of counts[2][2][3][n_cycles][2] -> (bytes, length).  cap: the room (default: asked for first); a room
    too small gives (None, the length needed), with nothing written."""
    L = _lib.load()
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    mp = _lib.MbiasParams(counts.shape[3])
    if cap is None:
        need = L.bsc_mbias_format(_ptr(counts), C.byref(mp), None, 0)
        if need < 0:
            _check(int(need))
        cap = int(need)
    buf = np.full(max(int(cap), 1) + 8, 0xA5, dtype=np.uint8)
    got = L.bsc_mbias_format(_ptr(counts), C.byref(mp), _ptr(buf), int(cap))
    if got < 0:
        _check(int(got))
    assert (buf[int(cap) :] == 0xA5).all()
    if got > int(cap):
        assert (buf == 0xA5).all()
        return None, int(got)
    return buf[:got].tobytes(), int(got)


def epi_windows_host(tpl, seq, x, y, ref, min_qual=20, params=None, cap=None):
    """The host form of the epiallele table (bsc_epi_windows_host; csrc/epi.c): prepared TEMPLATE[nr] + their read bytes, the block x .. y and
    its reference codes (x .. y + 2) -> (WINDOW records[min(count, cap)], count, totals[8]).  No GPU involved.  cap: the room (default:
    every window)."""
    from .epialleles import WINDOW

    L = _lib.load()
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    if ref.size < int(y) - int(x) + 2:
        raise ValueError("ref must hold the codes of x .. y + 1 at least")
    ep = SiteCaller._epi_params(params)
    room = int(y) - int(x) + 1 if cap is None else int(cap)
    out = np.zeros(max(room, 1), dtype=WINDOW)
    n, tot = C.c_uint64(0), (C.c_uint64 * 8)()
    _check(L.bsc_epi_windows_host(_ptr(tpl), len(tpl), _ptr(seq), seq.size, int(x), int(y), _ptr(ref), int(min_qual), C.byref(ep), _ptr(out), room,
                                  C.byref(n), tot))
    return out[: min(int(n.value), room)].copy(), int(n.value), tuple(int(v) for v in tot)


def epi_format_host(contig, recs, params=None, cap=None):
    """bsc_epi_format: the table's lines of WINDOW records -> (bytes, lines).  cap: the room (default: asked for first); a room too small
    gives (None, the length needed)."""
    from .epialleles import WINDOW

    L = _lib.load()
    recs = np.ascontiguousarray(recs, dtype=WINDOW)
    ep = SiteCaller._epi_params(params)
    name = contig.encode() if isinstance(contig, str) else contig
    t2 = (C.c_uint64 * 2)()
    if cap is None:
        need = L.bsc_epi_format(name, _ptr(recs), len(recs), C.byref(ep), None, 0, t2)
        if need < 0:
            _check(int(need))
        cap = int(need)
    buf = np.full(max(int(cap), 1) + 8, 0xA5, dtype=np.uint8)
    got = L.bsc_epi_format(name, _ptr(recs), len(recs), C.byref(ep), _ptr(buf), int(cap), t2)
    if got < 0:
        _check(int(got))
    assert (buf[int(cap) :] == 0xA5).all() and int(t2[0]) == got
    if got > int(cap):
        assert (buf == 0xA5).all()
        return None, int(got)
    return buf[:got].tobytes(), int(t2[1])


def pat_recs_host(tpl, seq, x, y, ref, min_qual=20, params=None, cap=None):
    """The host form of the per-read CpG pattern table (bsc_pat_recs_host; csrc/pat.c): prepared TEMPLATE[nr] + their read bytes, the block
    x .. y and its reference codes (x .. y + 2) -> (REC records[min(count, cap)], count, totals[8]).  No GPU involved.  cap: the room
    (default: asked for with a room of 0 first)."""
    from .pat import REC

    L = _lib.load()
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    if ref.size < int(y) - int(x) + 2:
        raise ValueError("ref must hold the codes of x .. y + 1 at least")
    pp = SiteCaller._pat_params(params)
    n, tot = C.c_uint64(0), (C.c_uint64 * 8)()
    if cap is None:
        _check(L.bsc_pat_recs_host(_ptr(tpl), len(tpl), _ptr(seq), seq.size, int(x), int(y), _ptr(ref), int(min_qual), C.byref(pp), None, 0, C.byref(n),
                                   tot))
        cap = int(n.value)
    room = int(cap)
    out = np.zeros(max(room, 1), dtype=REC)
    _check(L.bsc_pat_recs_host(_ptr(tpl), len(tpl), _ptr(seq), seq.size, int(x), int(y), _ptr(ref), int(min_qual), C.byref(pp), _ptr(out), room,
                               C.byref(n), tot))
    return out[: min(int(n.value), room)].copy(), int(n.value), tuple(int(v) for v in tot)


def pat_format_host(contig, index_base, recs, params=None, cap=None):
    """bsc_pat_format: the table's lines of REC records -> (bytes, lines).  cap: the room (default: asked for first); a room too small gives
    (None, the length needed)."""
    from .pat import REC

    L = _lib.load()
    recs = np.ascontiguousarray(recs, dtype=REC)
    pp = SiteCaller._pat_params(params)
    name = contig.encode() if isinstance(contig, str) else contig
    t2 = (C.c_uint64 * 2)()
    if cap is None:
        need = L.bsc_pat_format(name, int(index_base), _ptr(recs), len(recs), C.byref(pp), None, 0, t2)
        if need < 0:
            _check(int(need))
        cap = int(need)
    buf = np.full(max(int(cap), 1) + 8, 0xA5, dtype=np.uint8)
    got = L.bsc_pat_format(name, int(index_base), _ptr(recs), len(recs), C.byref(pp), _ptr(buf), int(cap), t2)
    if got < 0:
        _check(int(got))
    assert (buf[int(cap) :] == 0xA5).all() and int(t2[0]) == got
    if got > int(cap):
        assert (buf == 0xA5).all()
        return None, int(got)
    return buf[:got].tobytes(), int(t2[1])


def frag_regions_host(tpl, seq, x, y, ref, regions, min_qual=20, params=None, acc=None, with_totals=True):
    """The host form of the per-region fragment summary (bsc_frag_regions_host; csrc/frag.c): prepared TEMPLATE[nr] + their read bytes, the
    block x .. y, its reference codes (x .. y + 2) and (start, end) regions in any order -> (uint64[n, 8] accumulators, totals[8]).  acc:
    accumulators to add into (default: zeros).  No GPU involved."""
    from .methbed import _regions

    L = _lib.load()
    tpl = np.ascontiguousarray(tpl, dtype=TEMPLATE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    if ref.size < int(y) - int(x) + 2:
        raise ValueError("ref must hold the codes of x .. y + 1 at least")
    regs = _regions(regions)
    fp = SiteCaller._frag_params(params)
    out = np.zeros((len(regs), 8), dtype=np.uint64) if acc is None else np.ascontiguousarray(acc, dtype=np.uint64).reshape(len(regs), 8).copy()
    tot = (C.c_uint64 * 8)()
    _check(L.bsc_frag_regions_host(_ptr(tpl), len(tpl), _ptr(seq), seq.size, int(x), int(y), _ptr(ref), int(min_qual), C.byref(fp),
                                   _ptr(regs) if len(regs) else None, len(regs), _ptr(out) if len(regs) else None, tot if with_totals else None))
    return out, tuple(int(v) for v in tot)


def frag_format_host(contig, regions, names, acc, cap=None):
    """bsc_frag_format: the table's lines of one contig's regions and their accumulators -> bytes.  cap: the room (default: asked for
    first); a room too small gives (None, the length needed); a bad argument raises ValueError."""
    from .methbed import _regions

    L = _lib.load()
    regs = _regions(regions)
    acc = np.ascontiguousarray(acc, dtype=np.uint64).reshape(-1, 8)
    if len(acc) != len(regs) or (names is not None and len(names) != len(regs)):
        raise ValueError("as many accumulators and names as regions")
    name = contig if isinstance(contig, (bytes, bytearray)) else str(contig).encode()
    nm = None
    if names is not None:
        nm = (C.c_char_p * max(len(regs), 1))(*[(None if s is None else s if isinstance(s, (bytes, bytearray)) else str(s).encode()) for s in names])
    rp, ap = (regs.ctypes.data, acc.ctypes.data) if len(regs) else (None, None)
    if cap is None:
        need = L.bsc_frag_format(name, rp, nm, ap, len(regs), None, 0)
        if need < 0:
            raise ValueError("bsc_frag_format: bad argument")
        cap = int(need)
    buf = np.full(max(int(cap), 1) + 8, 0xA5, dtype=np.uint8)
    got = L.bsc_frag_format(name, rp, nm, ap, len(regs), _ptr(buf) if cap else None, int(cap))
    if got < 0:
        raise ValueError("bsc_frag_format: bad argument")
    assert (buf[int(cap) :] == 0xA5).all()
    if got > int(cap):
        assert (buf == 0xA5).all()
        return None, int(got)
    return buf[:got].tobytes()


def pat_count_sites(codes, start, stop):
    """bsc_pat_count_sites: the sites p with start <= p < stop (positions, 1 first) over a contig's codes as bsc_fasta_contig gives them."""
    L = _lib.load()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n = C.c_uint64(0)
    _check(L.bsc_pat_count_sites(_ptr(codes), codes.size, int(start), int(stop), C.byref(n)))
    return int(n.value)
