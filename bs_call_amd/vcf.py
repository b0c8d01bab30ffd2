"""Host-side text rendering of bsc_vcf_core records (+ their gt_meth) as VCF data lines — through the library's ONE host
formatter, bsc_vcf_format / bsc_vcf_format_rec (host C, csrc/vcf_format.c).  The device writes the same lines at speed
(csrc/vcftextdev.hip: SiteCaller.vcf_text_*_device, block_vcf_rawdev); the host formatter is that encoder's CHECKER, and the
contract between them is bytes: whatever bsc_vcf_format_rec writes for a record, the device writes.

The reference hands each record to htslib (bcf_write, src/print_vcf.c:160-380); htslib is not part of this
repository, so the lines are the layout htslib's VCF text writer gives those fields.  Integer fields are exact by
construction; the float text format of GL (htslib prints floats with %g-style 6 significant digits) is NOT pinned
against htslib here.  No computation happens in this module: every number comes from the device records."""
from .abi import GENOTYPES

FLT_NAMES = ("q20", "qd2", "fs60", "mq40")  # src/init_param.c:15
CS_STR = tuple(("+" if "C" in g else "") + ("-" if "G" in g else "") or "NA" for g in GENOTYPES)  # src/print_vcf.c:61-62
HEADER = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s"


def format_block(cores, gtms, contig):
    """VCF data lines of one block, in position order (records with emit == 0 produce nothing): bsc_vcf_format."""
    import ctypes as C

    import numpy as np

    from . import _lib
    from .abi import GT_METH, VCF_CORE

    L = _lib.load()
    cores = np.ascontiguousarray(cores, dtype=VCF_CORE)
    gtms = np.ascontiguousarray(gtms, dtype=GT_METH)
    buf = C.create_string_buffer(1024)
    out = []
    cb, gb = cores.ctypes.data, gtms.ctypes.data
    for i in range(len(cores)):
        n = L.bsc_vcf_format(cb + 64 * i, gb + 200 * i, contig.encode(), None, buf, 1024)
        if n < 0:
            raise RuntimeError("bsc_vcf_format: buffer too small")
        if n:
            out.append(buf.raw[:n].decode())
    return out


def format_records_c(recs, contig):
    """VCF lines of packed records (VCF_REC[], what SiteCaller.block_records returns) through bsc_vcf_format_rec."""
    import ctypes as C

    import numpy as np

    from . import _lib
    from .abi import VCF_REC

    L = _lib.load()
    recs = np.ascontiguousarray(recs, dtype=VCF_REC)
    buf = C.create_string_buffer(1024)
    out = []
    rb = recs.ctypes.data
    for i in range(len(recs)):
        n = L.bsc_vcf_format_rec(rb + 128 * i, contig.encode(), None, buf, 1024)
        if n < 0:
            raise RuntimeError("bsc_vcf_format_rec: buffer too small")
        if n:
            out.append(buf.raw[:n].decode())
    return out


format_block_c = format_block  # round-1 name


# ---- BCF output: what the reference's output file holds (src/print_vcf.c:621-731 the header, :160-380 the records) -----------
INFO_FILTER_FORMAT_LINES = (  # src/print_vcf.c:712-731, verbatim texts (the FS line's missing '>' included)
    '##INFO=<ID=CX,Number=1,Type=String,Description="5 base sequence context (from position -2 to +2 on the positive strand) determined from the reference">',
    '##FILTER=<ID=fail,Description="No sample passed filters">',
    '##FILTER=<ID=q20,Description="Genotype Quality below 20">',
    '##FILTER=<ID=qd2,Description="Quality By Depth below 2">',
    '##FILTER=<ID=fs60,Description="Fisher Strand above 60">',
    '##FILTER=<ID=mq40,Description="RMS Mapping Quality below 40">',
    '##FILTER=<ID=mac1,Description="Minor allele count <= 1">',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
    '##FORMAT=<ID=FT,Number=1,Type=String,Description="Sample Genotype Filter">',
    '##FORMAT=<ID=GL,Number=G,Type=Float,Description="Genotype Likelihood">',
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Phred scaled conditional genotype quality">',
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read Depth (non converted reads only)">',
    '##FORMAT=<ID=MQ,Number=1,Type=Integer,Description="RMS Mapping Quality">',
    '##FORMAT=<ID=QD,Number=1,Type=Integer,Description="Quality By Depth (Variant quality / read depth (non-converted reads only))">',
    '##FORMAT=<ID=MC8,Number=8,Type=Integer,Description="Base counts: non-informative for methylation (ACGT) followed by informative for methylation (ACGT)">',
    '##FORMAT=<ID=AMQ,Number=.,Type=Integer,Description="Average base quailty for where MC8 base count non-zero">',
    '##FORMAT=<ID=CS,Number=1,Type=String,Description="Strand of Cytosine relative to reference sequence (+/-/+-/NA)">',
    '##FORMAT=<ID=CG,Number=1,Type=String,Description="CpG Status (from genotype calls: Y/N/H/?)">',
    '##FORMAT=<ID=CX,Number=1,Type=String,Description="5 base sequence context (from position -2 to +2 on the positive strand) determined from genotype call">',
    '##FORMAT=<ID=FS,Number=1,Type=Integer,Description="Phred scaled log p-value from Fishers exact test of strand bias">',
)


def header_text(contigs, sample, under_conv=0.01, over_conv=0.05, mapq_thresh=20, min_qual=20, date=None, dbsnp_header=None,
                benchmark_mode=False, version="2.1", fileformat="VCFv4.2"):
    """The VCF header print_vcf_header assembles (src/print_vcf.c:621-731): fileformat, htslib's PASS filter, the date /
    source / dbsnp lines (not in benchmark mode), one ##contig per (name, length[, assembly, md5, species]), the INFO /
    FILTER / FORMAT definitions, the column line.  The last FORMAT line is closed here (the reference's text lacks its '>';
    htslib's header parser decides what becomes of it — unpinned).  `fileformat` is htslib's bcf_hdr_get_version()."""
    import time

    lines = ["##fileformat=%s" % fileformat, '##FILTER=<ID=PASS,Description="All filters passed">']
    if not benchmark_mode:
        d = date or (lambda t: (t.tm_mday, t.tm_mon, t.tm_year))(time.localtime())
        lines.append("##fileDate(dd/mm/yyyy)=%02d/%02d/%04d" % tuple(d))
        lines.append("##source=bs_call_v%s,under_conversion=%g,over_conversion=%g,mapq_thresh=%d,bq_thresh=%d"
                     % (version, under_conv, over_conv, mapq_thresh, min_qual))
        if dbsnp_header:
            lines.append("##dbsnp=<%s>" % dbsnp_header)
    for c in contigs:
        extra = "".join(",%s=%s" % (k, v) for k, v in zip(("assembly", "md5", "sp"), c[2:]) if v)
        lines.append("##contig=<ID=%s,length=%d%s>" % (c[0], c[1], extra))
    lines += INFO_FILTER_FORMAT_LINES
    lines.append(HEADER % sample)
    return "\n".join(lines) + "\n"


def bcf_block(recs, rid, dbsnp=None):
    """The BCF2 records of a block's packed records (VCF_REC[]), concatenated (bsc_bcf_block); dbsnp: a DbSnpIndex with the
    block's contig loaded, to name the records whose rs_found flag is set."""
    import ctypes as C

    import numpy as np

    from . import _lib
    from .abi import VCF_REC

    L = _lib.load()
    recs = np.ascontiguousarray(recs, dtype=VCF_REC)
    ids = _lib.BcfIds()
    L.bsc_bcf_default_ids(C.byref(ids))
    cap = 64 + 256 * max(1, len(recs))
    buf = np.empty(cap, dtype=np.uint8)
    done = C.c_uint64(0)
    n = L.bsc_bcf_block(recs.ctypes.data, len(recs), rid, C.byref(ids), None if dbsnp is None else dbsnp._h, buf.ctypes.data, cap,
                        C.byref(done))
    if n < 0 or done.value != len(recs):
        raise RuntimeError("bsc_bcf_block failed (%d, %d of %d records)" % (n, done.value, len(recs)))
    return buf[:n].tobytes()


def _bgzf_block(data: bytes) -> bytes:
    """One BGZF block (SAM specification section 4.1): a gzip member with the 'BC' extra field holding the block size."""
    import struct
    import zlib

    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    total = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + body
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def write_bcf(path, header: str, record_blocks, compressed=True):
    """A BCF file: magic, header text, the records (an iterable of bsc_bcf_block outputs), BGZF-compressed like the
    reference's default output ("wb") or plain ("wbu")."""
    import struct

    text = header.encode() + b"\0"
    head = b"BCF\x02\x02" + struct.pack("<I", len(text)) + text
    with open(path, "wb") as f:
        if not compressed:
            f.write(head)
            for b in record_blocks:
                f.write(b)
            return
        pend = bytearray(head)
        for b in record_blocks:
            pend += b
            while len(pend) >= 0xFF00:
                f.write(_bgzf_block(bytes(pend[:0xFF00])))
                del pend[:0xFF00]
        if pend:
            f.write(_bgzf_block(bytes(pend)))
        f.write(BGZF_EOF)


def write_vcf(path, header: str, line_blocks, bgzip=False):
    """A VCF text file: the header, then the data lines (an iterable of lists of lines, e.g. format_records_c outputs);
    bgzip=True writes BGZF blocks (the reference's "wz" mode).  The GL floats are printed with %g (see the module text)."""
    def chunks():
        yield header.encode()
        for lines in line_blocks:
            if lines:
                yield ("\n".join(lines) + "\n").encode()

    with open(path, "wb") as f:
        if not bgzip:
            for c in chunks():
                f.write(c)
            return
        pend = bytearray()
        for c in chunks():
            pend += c
            while len(pend) >= 0xFF00:
                f.write(_bgzf_block(bytes(pend[:0xFF00])))
                del pend[:0xFF00]
        if pend:
            f.write(_bgzf_block(bytes(pend)))
        f.write(BGZF_EOF)


def write_vcf_blobs(path, header: str, blobs, compressed=False):
    """write_vcf for blocks that are already bytes (the device text encoder's streams: SiteCaller.block_vcf_rawdev): the header,
    then the blobs; compressed=True writes BGZF members cut every 0xFF00 bytes of the stream, as write_bcf does."""
    with open(path, "wb") as f:
        if not compressed:
            f.write(header.encode())
            for b in blobs:
                f.write(b)
            return
        pend = bytearray(header.encode())
        for b in blobs:
            pend += b
            while len(pend) >= 0xFF00:
                f.write(_bgzf_block(bytes(pend[:0xFF00])))
                del pend[:0xFF00]
        if pend:
            f.write(_bgzf_block(bytes(pend)))
        f.write(BGZF_EOF)


# ---- region queries through a CSI index (CSIv1): what bam2bcf --index / bsc_csi_* write beside a compressed file --------------------
def read_csi(path):
    """A .csi file parsed: {"min_shift", "depth", "aux" (bytes), "names" (the tabix block's, [] for BCF), "refs": [{bin: (loffset,
    [(beg, end), ...])}, ...], "n_no_coor"}.  Virtual offsets are integers (file offset of the member << 16 | offset inside it)."""
    import gzip
    import struct

    with gzip.open(path, "rb") as f:
        b = f.read()
    if b[:4] != b"CSI\x01":
        raise ValueError("%s: not a CSI index" % path)
    min_shift, depth, l_aux = struct.unpack_from("<iii", b, 4)
    aux = b[16 : 16 + l_aux]
    at = 16 + l_aux
    names = []
    if l_aux >= 28:
        l_nm = struct.unpack_from("<i", aux, 24)[0]
        names = [n.decode() for n in aux[28 : 28 + l_nm].split(b"\0")[:-1]]
    (n_ref,) = struct.unpack_from("<i", b, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", b, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            bin_, loff, n_chunk = struct.unpack_from("<IQi", b, at)
            at += 16
            bins[bin_] = (loff, [struct.unpack_from("<QQ", b, at + 16 * k) for k in range(n_chunk)])
            at += 16 * n_chunk
        refs.append(bins)
    n_no_coor = struct.unpack_from("<Q", b, at)[0] if at + 8 <= len(b) else 0
    return {"min_shift": min_shift, "depth": depth, "aux": aux, "names": names, "refs": refs, "n_no_coor": n_no_coor}


def csi_reg2bins(beg, end, min_shift, depth):
    """The bins of every level that overlap [beg, end) (0-based, half open): the CSI specification's reg2bins."""
    bins = []
    if beg >= end:
        return bins
    end -= 1
    s, t = min_shift + 3 * depth, 0
    for level in range(depth + 1):
        bins.extend(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
        t += 1 << (3 * level)
    return bins


def csi_chunks(index, tid, beg, end):
    """The chunks [(vbeg, vend), ...] of the file that may hold records of contig tid in [beg, end): the bins of reg2bins over all levels,
    without the chunks that end at or before the loffset of the first existing bin — found as htslib finds it: the leaf of beg, then its
    previous siblings, then the parents —, sorted, adjacent ones merged."""
    if tid < 0 or tid >= len(index["refs"]) or beg >= end:
        return []
    bins = index["refs"][tid]
    min_shift, depth = index["min_shift"], index["depth"]
    pseudo = ((1 << (3 * (depth + 1))) - 1) // 7 + 1
    b = ((1 << (3 * depth)) - 1) // 7 + (beg >> min_shift)
    min_off = 0
    while True:
        if b in bins and b != pseudo:
            min_off = bins[b][0]
            break
        if b == 0:
            break
        parent = (b - 1) >> 3
        b = b - 1 if b > (parent << 3) + 1 else parent
    got = []
    for k in csi_reg2bins(beg, end, min_shift, depth):
        if k in bins and k != pseudo:
            got += [c for c in bins[k][1] if c[1] > min_off]
    got.sort()
    out = []
    for c in got:
        if out and c[0] <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], c[1]))
        else:
            out.append((c[0], c[1]))
    return out


class _BgzfReader:
    """Members of a BGZF file read at their file offsets; a position is a virtual offset, kept normalised: the end of a member is the
    beginning of the next."""

    def __init__(self, f):
        self.f = f
        self.coff, self.data, self.bsize, self.uoff = -1, b"", 0, 0

    def _load(self, coff):
        import struct
        import zlib

        self.f.seek(coff)
        h = self.f.read(18)
        if len(h) < 18:
            self.coff, self.data, self.bsize = coff, b"", 0
            return
        if h[:4] != b"\x1f\x8b\x08\x04" or h[12:14] != b"BC":
            raise ValueError("not a BGZF member at %d" % coff)
        bsize = struct.unpack("<H", h[16:18])[0] + 1
        body = self.f.read(bsize - 18)
        self.coff, self.data, self.bsize = coff, zlib.decompress(body[:-8], -15), bsize

    def seek(self, voff):
        if voff >> 16 != self.coff:
            self._load(voff >> 16)
        self.uoff = voff & 0xFFFF
        self._norm()

    def _norm(self):
        while self.bsize and self.uoff >= len(self.data):
            self._load(self.coff + self.bsize)
            self.uoff = 0

    def tell(self):
        return self.coff << 16 | self.uoff

    def read(self, n):
        out = bytearray()
        while n and self.bsize:
            k = self.data[self.uoff : self.uoff + n]
            out += k
            n -= len(k)
            self.uoff += len(k)
            self._norm()
        return bytes(out)

    def readline(self):
        out = bytearray()
        while self.bsize:
            e = self.data.find(b"\n", self.uoff)
            if e >= 0:
                out += self.data[self.uoff : e + 1]
                self.uoff = e + 1
                self._norm()
                break
            out += self.data[self.uoff :]
            self.uoff = len(self.data)
            self._norm()
        return bytes(out)


def fetch(path, contig, beg, end, index=None):
    """The records of `contig` (a name, or the header's 0-based contig number) whose 0-based position lies in [beg, end), from the
    BGZF-compressed BCF or VCF file `path` through its CSI index (`index`: a read_csi result; default path + ".csi"): raw BCF2 records
    (l_shared and l_indiv included) or text lines with their newline, in file order.  Only the index's chunks are read."""
    import re
    import struct

    ix = index if index is not None else read_csi(path + ".csi")
    out = []
    with open(path, "rb") as f:
        r = _BgzfReader(f)
        r.seek(0)
        is_bcf = r.data[:5] == b"BCF\x02\x02"
        if isinstance(contig, str):
            if is_bcf:
                r.read(5)
                (l_text,) = struct.unpack("<I", r.read(4))
                names = re.findall(r"^##contig=<ID=([^,>]+)", r.read(l_text).decode("utf-8", "replace"), flags=re.M)
            else:
                names = ix["names"]
            if contig not in names:
                return out
            tid = names.index(contig)
        else:
            tid = int(contig)
        name = None
        if not is_bcf and tid < len(ix["names"]):
            name = ix["names"][tid].encode()
        for vbeg, vend in csi_chunks(ix, tid, beg, end):
            r.seek(vbeg)
            while r.bsize and r.tell() < vend:
                if is_bcf:
                    h = r.read(8)
                    if len(h) < 8:
                        break
                    l_shared, l_indiv = struct.unpack("<II", h)
                    body = r.read(l_shared + l_indiv)
                    rid, pos = struct.unpack_from("<ii", body, 0)
                    if rid == tid and beg <= pos < end:
                        out.append(h + body)
                else:
                    line = r.readline()
                    if not line or line[:1] == b"#":
                        continue
                    cols = line.split(b"\t", 2)
                    if (name is None or cols[0] == name) and beg <= int(cols[1]) - 1 < end:
                        out.append(line)
    return out
