"""BAM -> BCF through the library, block by block — the reference's four threads in a line (reader: bsc_bam_next_block;
process: the block's reference; process + calc + print: bsc_block_bcf_raw on the GPU — pre-processing, calling, record formation and
the BCF encoding; output: the writer) —
and the run's JSON report.  An example of the pieces put together for tests and for INTEGRATION.md, not a command-line
replacement of bs_call: the reference's argument parsing, region / contig selection and FASTA reader are out of scope
(SURVEY.md section 8)."""
from typing import Dict, Optional

import numpy as np

from . import _lib, report, vcf
from .bam import BamReader, block_reference
from .caller import ReadProfile, SiteCaller, gc_bins, pat_count_sites, prepare_templates


def run(bam_path: str, reference: Dict[str, np.ndarray], bcf_path: str, sample: str = "SAMPLE", report_path: Optional[str] = None,
        caller: Optional[SiteCaller] = None, dbsnp=None, compressed: bool = True, date=None, left_trim=(0, 0), right_trim=(0, 0),
        min_qual: Optional[int] = None, benchmark_mode: bool = False, under_conv: Optional[float] = None, over_conv: Optional[float] = None,
        host_prep: bool = False, host_bcf: bool = False, device_reader: bool = False, shard_rank: Optional[int] = None, shard_world: int = 1,
        reduce_device=None, text: bool = False, dbsnp_device: bool = False, meth_path: Optional[str] = None, meth_params=None, meth_merge: bool = False,
        meth_regions=None, meth_regions_path: Optional[str] = None, meth_window: Optional[int] = None, bigwig_path: Optional[str] = None,
        cov_bigwig_path: Optional[str] = None,
        bigwig_section: int = 1024, bigwig_zoom: int = 1024, bigwig_compress: bool = False, bigbed_path: Optional[str] = None, bigbed_items: int = 512,
        bigbed_zoom: int = 1024, bigbed_compress: bool = False, meth_index: Optional[str] = None, variants_path: Optional[str] = None,
        variants_params=None, cpg_reads_path: Optional[str] = None, cpg_reads_params=None, asm_path: Optional[str] = None, asm_params=None,
        mbias_path: Optional[str] = None, mbias_params=None, epi_path: Optional[str] = None, epi_params=None,
        pat_path: Optional[str] = None, pat_params=None, frag_path: Optional[str] = None, frag_params=None, **reader_kw) -> dict:
    """reference: contig name -> uint8 reference codes (0 = N, 1..4 = ACGT; position 1 first).  Returns a summary dict.
    under_conv / over_conv / min_qual (defaults 0.01 / 0.05 / 20, src/init_param.c:26-31) are the MODEL's parameters: without
    `caller` the run builds its SiteCaller from them; with one, they are taken from it and a differing explicit value is an error
    (the header must name the thresholds the genotypes were computed with, src/print_vcf.c:647-692).  host_prep: the read
    pre-processing on the host (bsc_prepare_templates_profile) instead of the device (round 5's default) — same bytes.  host_bcf:
    the packed records come back and the host encodes them (bsc_bcf_block) instead of the device's encoder (bsc_block_bcf_raw,
    round 5's default) — same bytes.  device_reader: the blocks are formed on the device from the inflated BAM bytes (round 6:
    bamdev.DeviceBamReader — the host only inflates) and go on to bsc_block_bcf_rawdev where they lie — same bytes.
    shard_rank / shard_world: ONE RANK of a sharded run over one file (SURVEY.md 8e on real input; the reference's unit of parallelism is a
    process per contig over an indexed file, src/process.c:125, src/get_template_vector.c:69-99): the header's contigs are dealt to the ranks by
    shard.assign_contigs (longest first), every rank reads the stretches of the file that hold ITS contigs (the device reader's contig
    selection: no index file), writes each contig's records to a shard beside bcf_path, and at the end the ranks all-reduce what the report
    sums (torch.distributed's default group: RCCL between GPUs, gloo in the rehearsal; reduce_device = the tensors' device) and rank 0
    concatenates the shards in contig order behind the header — the bytes of the single run.
    text: the output file is VCF TEXT (the reference's -O v; with `compressed`, BGZF members cut every 0xFF00 bytes: its -O z) — the header
    text, then every block's lines as the device's text encoder writes them (SiteCaller.block_vcf_rawdev: bsc_block_vcf_rawdev_keep).  Needs
    device_reader; a sharded text run is refused.
    dbsnp_device: with a `dbsnp` and the device reader, each contig of the index is kept in HBM (SiteCaller.dbsnp_attach at the contig
    change) and the blocks' flags and names are made there (csrc/dbsnpdev.hip) instead of on this thread — same bytes, same report.
    meth_path: the per-cytosine methylation table (bedMethyl; include/bscall_amd.h has the line) of the same run, written beside the output:
    every block's lines from the arrays the block left on the device (SiteCaller.block_meth_kept, csrc/methdev.hip); with `compressed`,
    BGZF like the main file.  meth_params: a _lib.MethParams or a dict of its fields (default: CpG cytosines, every covered site).  Needs
    device_reader and is refused where text=True is; the main file and the report are those of the run without it.  meth_merge: the table
    is the combined-strand one, a line per CpG dinucleotide with both strands' counts added (bsc_block_meth_cpg_kept); needs meth_path and
    CpG-only meth_params.
    meth_index: "tbi" or "csi" — the index of the compressed table, written to meth_path + ".tbi" / ".csi" (include/bscall_amd.h has the
    rule): every block's table is scanned on the device where it lies (SiteCaller.block_meth_index_kept, csrc/beddev.hip), the entries
    go to a detached TabixIndex, and the sizes of the members this process compressed on the host close it.  Needs meth_path and
    compressed=True.
    meth_regions / meth_window with meth_regions_path: the per-region methylation summary of the same run (include/bscall_amd.h has the rule
    and the ten columns), summed on the device: a contig's regions are attached at the contig change, every block adds its cytosines
    (SiteCaller.block_meth_regions_kept, csrc/methregionsdev.hip), the sums are read at the next contig change and at the end.
    meth_regions: the path of a BED file, or a list of (contig, start, end[, name]) — 0-based, half-open; sorted here as the BED reader
    sorts, stably by (start, end) —, or what methbed.parse_regions returns.  meth_window=n in its place: fixed tiles of n bases over every
    contig.  meth_params apply; meth_path is not needed.  The file is plain text, contigs in the order their blocks come; a contig without
    a block gives no line.  The same conditions as meth_path.
    bigwig_path: the methylation bigWig track of the same run (include/bscall_amd.h has the rule and the file's layout): every block's data
    sections and summaries from the arrays it left on the device (SiteCaller.block_bigwig_kept, csrc/bigwigdev.hip), the file by
    bigwig.Writer.  bigwig_section: sites a section (1 .. 65535); bigwig_zoom: the width of a level-0 zoom window.  meth_params apply; the
    track is per cytosine whatever meth_merge says; meth_path is not needed.  The same conditions as meth_path.  bigwig_compress: every
    section leaves the device as a zlib stream (SiteCaller.block_bigwig_deflate, csrc/zlibdev.hip) and the writer deflates the zoom blocks:
    the file readers meet in practice, about half the bytes; needs bigwig_path or cov_bigwig_path and bigwig_section <= 8157.
    cov_bigwig_path: the coverage track of the same sites (the depth a + b; the coverage rule of include/bscall_amd.h), alone or beside
    bigwig_path — then ONE SiteCaller.block_bigwig_tracks_kept call (csrc/bwcovdev.hip, mask 3) reduces the block for both files.  It
    honours bigwig_section, bigwig_zoom and bigwig_compress; the same conditions as bigwig_path.

    bigbed_path: the per-cytosine table of the same run as a bigBed file (include/bscall_amd.h has the rule and the file's layout): every
    block's items and summaries from the arrays it left on the device (SiteCaller.block_bigbed_kept, csrc/bigbeddev.hip), the file by
    bigbed.Writer.  bigbed_items: sites a block (1 .. 65535); bigbed_zoom: the width of a level-0 zoom window.  meth_params apply; the same
    conditions as bigwig_path.  bigbed_compress: every block leaves the device as a zlib stream (SiteCaller.block_bigbed_deflate); needs
    bigbed_path and bigbed_items <= bigbed.Z_ITEMS_MAX.

    variants_path: the variant-only call set of the same run (include/bscall_amd.h has the rule): every block's records with an ALT
    allele, selected on the device from the arrays the block left there and encoded by the block's own encoder
    (SiteCaller.block_variants_kept, csrc/variantsdev.hip) — a file of the run's format and compression with the main file's header.
    variants_params: a _lib.VarParams or a dict of min_phred / pass_only / known_only.  The summary gets "variant_records" and
    "variant_totals" (the ten totals of the rule).  The same conditions as meth_path.
    cpg_reads_path: the read-level CpG concordance table of the same run (include/bscall_amd.h has the rule): behind every block the walk over
    the prepared templates, reads and reference codes the block left on the device (SiteCaller.block_cpg_reads_kept, csrc/cpgreadsdev.hip)
    — a line per reference CpG a template reads, plain text or BGZF as `compressed` says.  cpg_reads_params: a _lib.CpgReadsParams or a dict
    of min_sites / min_cov.  The summary gets "cpg_reads_lines" and "cpg_reads_totals" (the eight totals of the rule).  The same conditions as
    meth_path.
    asm_path: the allele-specific methylation table of the same run (include/bscall_amd.h has the rule): behind every block, for each
    heterozygous SNP the block's call wrote and each reference CpG within max_dist of it, the templates of allele 1 / allele 2 that read the
    CpG methylated / unmethylated and the phred of Fisher's p of that table (SiteCaller.block_asm_kept, csrc/asmdev.hip) — lines ordered by
    SNP, plain text or BGZF as `compressed` says.  asm_params: a _lib.AsmParams or a dict of min_phred / pass_only / max_dist / min_cov.  The
    summary gets "asm_lines" and "asm_totals" (the eight totals of the rule).  The same conditions as meth_path.
    mbias_path: the M-bias table of the same run (include/bscall_amd.h has the rule): methylated / unmethylated calls per sequencing cycle by
    read end, bisulfite strand and CpG / CHG / CHH, from the raw templates as sequenced — behind every block the walk over the raw arrays the
    device reader left in HBM (SiteCaller.block_mbias_rawdev, csrc/mbiasdev.hip) into the context's accumulator, which the run resets before
    and after; ONE table per run, plain text whatever `compressed` says.  mbias_params: a _lib.MbiasParams, a dict of n_cycles, or n_cycles
    (default 512, 1 .. 1024).  The summary gets "mbias_totals" (the eight totals of the rule).  The same conditions as meth_path.
    epi_path: the epiallele table of the same run (include/bscall_amd.h has the rule): behind every block, per window of four consecutive
    reference CpGs, the templates that show each of the 16 methylation patterns, from the prepared templates, reads and reference codes the
    block left on the device (SiteCaller.block_epi_kept, csrc/epidev.hip) — plain text, or BGZF where `compressed` says so or the name ends
    in .gz.  epi_params: a _lib.EpiParams or a dict of min_cov.  The summary gets "epi_lines" and "epi_totals" (the eight totals of the
    rule).  The same conditions as meth_path.
    pat_path: the per-read CpG pattern table (PAT) of the same run (include/bscall_amd.h has the rule): behind every block the templates'
    methylation strings over the reference CpGs they cover, collapsed, counted and sorted on the device (SiteCaller.block_pat_kept,
    csrc/patdev.hip) — `chrom index pattern count`, wgbstools-unpinned bytes, the index the CpG's 1-based ordinal within its contig, 64 CpGs a
    line at the most; plain text, or BGZF where `compressed` says so or the name ends in .gz.  pat_params: a _lib.PatParams or a dict of
    min_sites.  The summary gets "pat_lines" and "pat_totals" (the eight totals of the rule).  Refused where epi_path is.
    frag_path: the per-region fragment methylation summary of the same run (include/bscall_amd.h has the rule) over the meth_regions /
    meth_window intervals: per interval the templates that are mostly unmethylated, mixed and mostly methylated within it, twelve columns
    whose first four join the meth_regions_path lines — attached, summed behind every block (SiteCaller.block_frag_kept, csrc/fragdev.hip)
    and read where the region summary is.  With frag_path, meth_regions_path may be left out.  frag_params: a _lib.FragParams or a dict of
    min_sites / u_max_pct / m_min_pct.  The summary gets "frag_lines" and "frag_totals".  The same conditions as meth_regions."""
    if pat_params is not None and pat_path is None:
        raise ValueError("pat_params are thresholds of the table pat_path names: they need pat_path")
    if pat_path is not None and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("pat_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if epi_params is not None and epi_path is None:
        raise ValueError("epi_params are thresholds of the table epi_path names: they need epi_path")
    if epi_path is not None and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("epi_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if mbias_params is not None and mbias_path is None:
        raise ValueError("mbias_params size the table mbias_path names: they need mbias_path")
    if mbias_path is not None and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("mbias_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if mbias_path is not None:
        from . import mbias as _mbias

        mbias_cycles = _mbias.n_cycles_of(mbias_params)
    if asm_params is not None and asm_path is None:
        raise ValueError("asm_params are thresholds of the table asm_path names: they need asm_path")
    if asm_path is not None and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("asm_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if cpg_reads_params is not None and cpg_reads_path is None:
        raise ValueError("cpg_reads_params are thresholds of the table cpg_reads_path names: they need cpg_reads_path")
    if cpg_reads_path is not None and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("cpg_reads_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if variants_params is not None and variants_path is None:
        raise ValueError("variants_params select among the records variants_path names: they need variants_path")
    if variants_path is not None and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("variants_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    want_bb = bigbed_path is not None
    if bigbed_compress and not want_bb:
        raise ValueError("bigbed_compress needs bigbed_path")
    if bigbed_compress and int(bigbed_items) > 0xFF00 // 100:
        raise ValueError("bigbed_compress: a block of more than %d sites may be more than 0xFF00 bytes" % (0xFF00 // 100))
    if want_bb and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("bigbed_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if want_bb and not (1 <= int(bigbed_items) <= 65535 and 1 <= int(bigbed_zoom) <= 0xFFFFFFFF):
        raise ValueError("bigbed_items is 1 .. 65535 sites, bigbed_zoom 1 or more bases")
    want_bw, want_cov = bigwig_path is not None, cov_bigwig_path is not None
    if bigwig_compress and not (want_bw or want_cov):
        raise ValueError("bigwig_compress needs bigwig_path")
    if bigwig_compress and int(bigwig_section) > 8157:
        raise ValueError("bigwig_compress: a section of more than 8157 sites is more than 0xFF00 bytes")
    if want_bw and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("bigwig_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if want_cov and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("cov_bigwig_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if (want_bw or want_cov) and not (1 <= int(bigwig_section) <= 65535 and 1 <= int(bigwig_zoom) <= 0xFFFFFFFF):
        raise ValueError("bigwig_section is 1 .. 65535 sites, bigwig_zoom 1 or more bases")
    want_regions = meth_regions is not None or meth_window is not None
    if meth_regions is not None and meth_window is not None:
        raise ValueError("meth_regions and meth_window exclude each other: the regions are the given ones or the fixed tiles")
    if (want_regions != (meth_regions_path is not None)) and not (want_regions and frag_path is not None):
        raise ValueError("meth_regions / meth_window and meth_regions_path go together: the regions to sum and the summary to write")
    if frag_params is not None and frag_path is None:
        raise ValueError("frag_params are thresholds of the summary frag_path names: they need frag_path")
    if frag_path is not None and not want_regions:
        raise ValueError("frag_path sums over the intervals of meth_regions or meth_window: it needs one of them")
    if frag_path is not None:
        from . import frag as _frag

        _frag._params(frag_params)  # (refused before the run starts)
    if meth_window is not None and int(meth_window) < 1:
        raise ValueError("meth_window is a count of bases, 1 or more")
    if want_regions and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("meth_regions is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    region_sets = None
    if meth_regions is not None:
        from . import methbed

        if isinstance(meth_regions, (str, bytes)) or hasattr(meth_regions, "__fspath__"):
            region_sets = methbed.read_regions(meth_regions)
        elif isinstance(meth_regions, dict):
            region_sets = meth_regions
        else:
            region_sets = {}
            for row in meth_regions:
                region_sets.setdefault(str(row[0]), []).append((int(row[1]), int(row[2]), str(row[3]) if len(row) > 3 else "."))
            for k, rows in region_sets.items():
                rows.sort(key=lambda r: (r[0], r[1]))  # (stable)
                regs = np.zeros(len(rows), dtype=methbed.REGION)
                regs["start"], regs["end"] = [r[0] for r in rows], [r[1] for r in rows]
                region_sets[k] = (regs, [r[2] for r in rows])
    if meth_merge and meth_path is None:
        raise ValueError("meth_merge=True combines the strands of the table meth_path names: it needs meth_path")
    if meth_merge and meth_params is not None and (meth_params.contexts if hasattr(meth_params, "contexts") else meth_params.get("contexts", 0)) != 0:
        raise ValueError("meth_merge=True is the CpG table: only a CpG has a partner strand (meth_params.contexts must be BSC_METH_CPG)")
    if meth_index is not None and meth_index not in ("tbi", "csi"):
        raise ValueError("meth_index is 'tbi' or 'csi', not %r" % (meth_index,))
    if meth_index is not None and (meth_path is None or not compressed):
        raise ValueError("meth_index indexes the compressed table meth_path names: it needs meth_path and compressed=True")
    if meth_path is not None and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("meth_path is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    if dbsnp_device and not device_reader:
        raise ValueError("dbsnp_device=True needs the device reader (device_reader=True)")
    if dbsnp_device and shard_rank is not None:
        raise ValueError("dbsnp_device=True is a single run (no shard_rank)")
    on_device = dbsnp_device and dbsnp is not None
    if text and (shard_rank is not None or not device_reader or host_prep or host_bcf):
        raise ValueError("text=True is a single run on the device reader (device_reader=True, no shard_rank, no host_prep / host_bcf)")
    bw_writer = cov_writer = bb_writer = None
    bb_sites = 0
    own = caller is None
    if own:
        under_conv = 0.01 if under_conv is None else under_conv
        over_conv = 0.05 if over_conv is None else over_conv
        min_qual = 20 if min_qual is None else min_qual
        c = SiteCaller(under_conv=under_conv, over_conv=over_conv, min_qual=min_qual)
    else:
        c = caller
        for name, given in (("under_conv", under_conv), ("over_conv", over_conv), ("min_qual", min_qual)):
            if given is not None and given != c.params[name]:
                raise ValueError("%s=%r disagrees with the supplied caller's %r" % (name, given, c.params[name]))
        under_conv, over_conv, min_qual = c.params["under_conv"], c.params["over_conv"], c.params["min_qual"]
    try:
        prof = ReadProfile()
        base_filter = np.zeros(5, dtype=np.uint64)
        passed = np.zeros(2, dtype=np.uint64)
        per_contig = []
        n_blocks = n_records = 0
        meth_blobs, meth_lines = [], 0
        var_blobs, var_totals = [], np.zeros(10, dtype=np.uint64)
        reads_blobs, reads_lines, reads_totals = [], 0, np.zeros(8, dtype=np.uint64)
        asm_blobs, asm_lines, asm_totals = [], 0, np.zeros(8, dtype=np.uint64)
        epi_blobs, epi_lines, epi_totals = [], 0, np.zeros(8, dtype=np.uint64)
        pat_blobs, pat_lines, pat_totals = [], 0, np.zeros(8, dtype=np.uint64)
        mbias_any = False
        if mbias_path is not None:
            c.mbias_reset()
        meth_entries = []  # meth_index: (contig number, BED_ENTRY[], bytes of the block's table)
        bw_sites = cov_sites = 0
        region_out, region_cur = [], None  # the summary's lines, contig by contig; (name, regions, names) of the contig attached
        frag_out, frag_totals = [], np.zeros(8, dtype=np.uint64)  # frag_path: the fragment summary's lines over the same regions
        c.reset_site_stats()
        sharded = shard_rank is not None
        if sharded:
            from . import shard as S
            from .bamdev import BamStream

            device_reader = True
            with BamStream(bam_path, threads=1, contigs=[]) as hs:  # the header alone
                all_refs = hs.refs
            parts = S.assign_contigs([l for _, l in all_refs], shard_world)
            mine = sorted(parts[shard_rank])
            if all_refs and len(all_refs) - 1 in parts[shard_rank]:
                mine = mine + [-1]  # the unplaced reads at the file's end go with the last contig's rank
            reader_kw = dict(reader_kw, contigs=mine)
            shard_files = {}
        if device_reader:
            if host_prep or host_bcf:
                raise ValueError("device_reader goes with the device pre-processing and encoder")
            from .bamdev import DeviceBamReader

            reader = DeviceBamReader(c, bam_path, **reader_kw)
        else:
            reader = BamReader(bam_path, **reader_kw)
        with reader as rd:
            refs = rd.refs
            # the header names the run's own thresholds (print_vcf_header, src/print_vcf.c:647-692)
            header = vcf.header_text([(n, l) for n, l in refs], sample, under_conv=under_conv, over_conv=over_conv,
                                     mapq_thresh=reader_kw.get("mapq_thresh", 20), min_qual=min_qual, date=date,
                                     dbsnp_header=None if dbsnp is None else dbsnp.header, benchmark_mode=benchmark_mode)

            if want_bw or want_cov:
                from . import bigwig

                bw_par = {"items_per_section": int(bigwig_section), "reduction": int(bigwig_zoom)}
                if want_bw:
                    bw_writer = bigwig.Writer(bigwig_path, refs, int(bigwig_section), int(bigwig_zoom), compress=bool(bigwig_compress))
                if want_cov:
                    cov_writer = bigwig.Writer(cov_bigwig_path, refs, int(bigwig_section), int(bigwig_zoom), compress=bool(bigwig_compress), track="coverage")

            if want_bb:
                from . import bigbed

                bb_writer = bigbed.Writer(bigbed_path, refs, int(bigbed_items), int(bigbed_zoom), compress=bool(bigbed_compress))
                bb_par = {"items_per_block": int(bigbed_items), "reduction": int(bigbed_zoom)}

            def regions_flush():
                nonlocal region_cur
                if region_cur is not None:
                    from . import methbed

                    if meth_regions_path is not None:
                        region_out.append(methbed.format_regions(region_cur[0], region_cur[1], region_cur[2], c.meth_regions_read()))
                    if frag_path is not None:
                        frag_out.append(_frag.format_regions(region_cur[0], region_cur[1], region_cur[2], c.frag_read()))
                region_cur = None

            def block_blobs():
                nonlocal n_blocks, n_records, base_filter, passed, meth_lines, region_cur, bw_sites, cov_sites, bb_sites, var_totals, reads_lines, reads_totals, asm_lines, asm_totals, mbias_any, epi_lines, epi_totals, pat_lines, pat_totals, frag_totals
                before, cur_tid = c.site_totals(), -1
                pat_base, pat_from = 0, 1  # the contig's CpGs in front of position pat_from
                pat_room = 8.0  # the table's room in bytes a position: a quarter above the last block's need, so that a block is walked once
                for item in (rd.device_blocks() if device_reader else rd.blocks()):
                    if device_reader:
                        dblk = item
                        tid, y = int(dblk.tid), int(dblk.y)
                    else:
                        tid, y, raw, seq, ms = item
                    name, _ = refs[tid]
                    if tid != cur_tid:
                        if cur_tid >= 0:
                            after = c.site_totals()
                            per_contig.append((refs[cur_tid][0], after - before))
                            before = after
                        cur_tid = tid
                        pat_base, pat_from = 0, 1
                        if want_regions:
                            regions_flush()
                            if meth_window is not None:
                                from . import methbed

                                region_cur = (name, methbed.window_regions(refs[tid][1], int(meth_window)), None)
                            else:
                                region_cur = (name, *region_sets[name]) if name in region_sets else None
                            n_att = 0
                            if meth_regions_path is not None:
                                n_att = c.meth_regions_attach(region_cur[1] if region_cur else [])
                            if frag_path is not None:
                                n_att = c.frag_attach(region_cur[1] if region_cur else [])
                            if n_att == 0:
                                region_cur = None
                        if dbsnp is not None:
                            dbsnp.load_contig(name)
                            if on_device:
                                c.dbsnp_attach(dbsnp)
                        # the contig's GC bins (load_sequence computes them when a report is asked for), resident on the device
                        gc_start, bins = gc_bins(reference[name])
                        c.set_gc_bins_host(bins, gc_start)
                    codes = reference[name]
                    if device_reader:
                        x = int(dblk.x)
                    else:
                        x = int(raw["pos"][0][0]) or int(raw["pos"][0][1])
                        x = x - 2 if x > 2 else 1  # process_template_vector, src/process_template.c:22-28
                    ref = block_reference(codes, x, y)
                    flags = None if dbsnp is None or on_device else dbsnp.flags(x, y - x + 1)
                    if device_reader:  # the block is in HBM already: pre-processing, calling, encoding behind it
                        names = None if dbsnp is None or on_device else dbsnp.names(x, y - x + 1)
                        if text:
                            blob, n_rec, st = c.block_vcf_rawdev(dblk, ref, name, names=names, left_trim=left_trim, right_trim=right_trim, min_qual=min_qual,
                                                                 reg_stop=len(codes), dbsnp=flags, with_stats=True, profile=prof)
                        else:
                            blob, n_rec, st = c.block_bcf_rawdev(dblk, ref, tid, names=names, left_trim=left_trim, right_trim=right_trim, min_qual=min_qual,
                                                                 reg_stop=len(codes), dbsnp=flags, with_stats=True, profile=prof,
                                                                 keep=meth_path is not None or want_regions or want_bw or want_cov or want_bb or variants_path is not None
                                                                 or cpg_reads_path is not None or asm_path is not None or mbias_path is not None or epi_path is not None
                                                                 or pat_path is not None)
                        if mbias_path is not None:  # the block's raw templates, still in the reader's buffers, into the run's accumulator
                            c.block_mbias_rawdev(dblk.d_tpl, dblk.nr, dblk.d_seq, dblk.seq_bytes, dblk.d_misms, dblk.n_misms, mbias_cycles)
                            mbias_any = True
                        if region_cur is not None and meth_regions_path is not None:  # the block's cytosines into the attached regions' sums
                            c.block_meth_regions_kept(meth_params)
                        if region_cur is not None and frag_path is not None and len(blob):  # ... and its templates into their fragment sums
                            frag_totals += np.array(c.block_frag_kept(frag_params), dtype=np.uint64)
                        if want_cov:  # the coverage track, and the level track with it, from ONE sweep over the block's arrays
                            ns, lv, cv = c.block_bigwig_tracks_kept(tid, (_lib.BW_LEVEL if want_bw else 0) | _lib.BW_COVERAGE, meth_params, bw_par,
                                                                    read_stream=not bigwig_compress)
                            for w, got, deflate in ((bw_writer, lv, c.block_bigwig_deflate), (cov_writer, cv, c.block_bigwig_cov_deflate)):
                                if got is None:
                                    continue
                                if bigwig_compress:
                                    zdata, zsizes = deflate()
                                    w.add_z(tid, zdata, zsizes, got[1], got[2])
                                else:
                                    w.add(tid, *got)
                            cov_sites += ns
                            bw_sites += ns if want_bw else 0
                        elif want_bw:  # the block's bigWig sections and summaries, appended to the track's file
                            data, ns, secs, zoom0 = c.block_bigwig_kept(tid, meth_params, bw_par, read_stream=not bigwig_compress)
                            if bigwig_compress:  # ... as zlib streams: the plain stream stays on the device
                                zdata, zsizes = c.block_bigwig_deflate()
                                bw_writer.add_z(tid, zdata, zsizes, secs, zoom0)
                            else:
                                bw_writer.add(tid, data, secs, zoom0)
                            bw_sites += ns
                        if want_bb:  # the block's bigBed items and summaries, appended to the bigBed's file
                            data, ns, blks, zoom0 = c.block_bigbed_kept(tid, meth_params, bb_par, read_stream=not bigbed_compress)
                            if bigbed_compress:  # ... as zlib streams: the plain stream stays on the device
                                zdata, zsizes = c.block_bigbed_deflate()
                                bb_writer.add_z(tid, zdata, zsizes, data, blks, zoom0)
                            else:
                                bb_writer.add(tid, data, blks, zoom0)
                            bb_sites += ns
                        if meth_path is not None:  # the same block's table, from what it left on the device
                            mb, ml, _ = c.block_meth_kept(name, meth_params, merge=meth_merge)
                            meth_blobs.append(mb)
                            meth_lines += ml
                            if meth_index is not None and mb:  # while the table is still the context's: the scan by the encoder's tile offsets
                                meth_entries.append((tid, c.block_meth_index_kept(14)[0], len(mb)))
                        if variants_path is not None:  # the same block's variant-only stream, by the block's own encoder
                            vb, _, vt = c.block_variants_kept(variants_params)
                            var_blobs.append(vb)
                            var_totals += np.array(vt, dtype=np.uint64)
                        if cpg_reads_path is not None:  # the same block's read-level CpG table, from its prepared reads still on the device
                            rb, rl, rt = c.block_cpg_reads_kept(name, cpg_reads_params)
                            reads_blobs.append(rb)
                            reads_lines += rl
                            reads_totals += np.array(rt, dtype=np.uint64)
                        if asm_path is not None:  # the same block's allele-specific table, from its dense records and its prepared reads
                            ab, al, at = c.block_asm_kept(name, asm_params)
                            asm_blobs.append(ab)
                            asm_lines += al
                            asm_totals += np.array(at, dtype=np.uint64)
                        if epi_path is not None:  # the same block's epiallele table, from its prepared reads still on the device
                            eb, el, et = c.block_epi_kept(name, epi_params)
                            epi_blobs.append(eb)
                            epi_lines += el
                            epi_totals += np.array(et, dtype=np.uint64)
                        if pat_path is not None:  # the same block's pattern table; its index counts the contig's CpGs
                            pat_base += pat_count_sites(codes, pat_from, x)
                            pat_from = x
                            pb, pl, pt = c.block_pat_kept(name, pat_params, index_base=pat_base, guess=int((y - x + 1) * pat_room) + 4096)
                            pat_room = 1.25 * len(pb) / (y - x + 1) + 1.0
                            pat_blobs.append(pb)
                            pat_lines += pl
                            pat_totals += np.array(pt, dtype=np.uint64)
                        recs = None
                    elif host_prep:  # round 4's split: the process thread's per-template work here, then the block
                        tpl, pseq, st = prepare_templates(raw, seq, ms, left_trim, right_trim, min_qual, profile=prof, x=x, ref=ref)
                        recs = c.block_records(tpl, pseq, x, y, ref, reg_stop=len(codes), dbsnp=flags, with_stats=True)
                    elif host_bcf:  # raw templates up, pre-processing and the read profile on the device (bsc_block_records_raw)
                        recs, st = c.block_records_raw(raw, seq, ms, x, y, ref, left_trim, right_trim, min_qual, reg_stop=len(codes), dbsnp=flags,
                                                       with_stats=True, profile=prof)
                    else:  # ... and the BCF encoding too: the block's stream comes back (bsc_block_bcf_raw)
                        names = None if dbsnp is None else dbsnp.names(x, y - x + 1)
                        blob, n_rec, st = c.block_bcf_raw(raw, seq, ms, x, y, ref, tid, names=names, left_trim=left_trim, right_trim=right_trim,
                                                          min_qual=min_qual, reg_stop=len(codes), dbsnp=flags, with_stats=True, profile=prof)
                        recs = None
                    base_filter += np.array([st["base_none"], st["base_trim"], st["base_clip"], st["base_overlap"], st["base_lowqual"]], dtype=np.uint64)
                    passed += np.array([st["reads"], st["read_bases"]], dtype=np.uint64)
                    if recs is not None:
                        blob, n_rec = vcf.bcf_block(recs, tid, dbsnp), len(recs)
                    if sharded:  # this contig's shard, written as its blocks are formed
                        if tid not in shard_files:
                            shard_files[tid] = open("%s.shard%05d" % (bcf_path, tid), "wb")
                        shard_files[tid].write(blob)
                    else:
                        yield blob
                    n_blocks += 1
                    n_records += n_rec
                if cur_tid >= 0:
                    per_contig.append((refs[cur_tid][0], c.site_totals() - before))

            if sharded:
                for _ in block_blobs():
                    pass
                for f_ in shard_files.values():
                    f_.close()
            elif text:
                vcf.write_vcf_blobs(bcf_path, header, block_blobs(), compressed)
            else:
                vcf.write_bcf(bcf_path, header, block_blobs(), compressed)  # blocks go to the writer as they are formed
            if meth_path is not None:
                vcf.write_vcf_blobs(meth_path, "", meth_blobs, compressed)
                if meth_index is not None:
                    from .caller import TBX_CSI, TBX_TBI, TabixIndex

                    with open(meth_path, "rb") as f:
                        zb = f.read()
                    sizes, at = [], 0
                    while at < len(zb):  # the members' sizes, from their own BSIZE fields; the last one is the end-of-file marker
                        sizes.append(int.from_bytes(zb[at + 16 : at + 18], "little") + 1)
                        at += sizes[-1]
                    with TabixIndex(None, TBX_TBI if meth_index == "tbi" else TBX_CSI, refs, 14, 0) as ix:
                        for tid_, ent, nb in meth_entries:
                            ix.add(tid_, ent, nb)
                        ix.members(sizes[:-1])
                        with open(meth_path + "." + meth_index, "wb") as f:
                            f.write(ix.finish())
            if variants_path is not None:
                if text:
                    vcf.write_vcf_blobs(variants_path, header, var_blobs, compressed)
                else:
                    vcf.write_bcf(variants_path, header, var_blobs, compressed)
            if cpg_reads_path is not None:
                vcf.write_vcf_blobs(cpg_reads_path, "", reads_blobs, compressed)
            if asm_path is not None:
                vcf.write_vcf_blobs(asm_path, "", asm_blobs, compressed)
            if epi_path is not None:
                vcf.write_vcf_blobs(epi_path, "", epi_blobs, compressed or str(epi_path).endswith(".gz"))
            if pat_path is not None:
                vcf.write_vcf_blobs(pat_path, "", pat_blobs, compressed or str(pat_path).endswith(".gz"))
            if mbias_path is not None:  # a run without a block has no accumulator: the header alone
                mbias_counts, mbias_totals = c.mbias_read(mbias_cycles) if mbias_any else (_mbias.empty(mbias_cycles)[0], (0,) * 8)
                c.mbias_reset()
                with open(mbias_path, "wb") as f:
                    f.write(_mbias.format_table(mbias_counts))
            if want_bw:
                bw_writer.finish()
            if want_cov:
                cov_writer.finish()
            if want_bb:
                bb_writer.finish()
            if want_regions:
                regions_flush()
                if meth_regions_path is not None:
                    with open(meth_regions_path, "wb") as f:
                        f.write(b"".join(region_out))
                if frag_path is not None:
                    with open(frag_path, "wb") as f:
                        f.write(b"".join(frag_out))
            cts, bases = rd.filter_counts()
        cts[0] += int(passed[0])
        bases[0] += int(passed[1])
        c.set_gc_bins_host(None, 0)
        site_stats, gc = c.site_stats(), c.gc_stats()
        prof_rows = prof.reported()
        if sharded:  # everything the report holds is a sum over positions / reads / templates: the ranks' shares add
            import torch.distributed as dist

            site_stats = S.allreduce_site_stats(site_stats, reduce_device)
            gc = S.allreduce_counts(gc, reduce_device)
            small = np.zeros(15 + 15 + 5 + 2 + 1, dtype=np.uint64)
            small[:15], small[15:30], small[30:35] = cts, bases, base_filter
            small[35], small[36], small[37] = n_blocks, n_records, 0
            small = S.allreduce_counts(small, reduce_device)
            cts, bases, base_filter = [int(v) for v in small[:15]], [int(v) for v in small[15:30]], small[30:35]
            n_blocks, n_records = int(small[35]), int(small[36])
            # the read profile: the vectors add; its length is the longest any rank saw
            used = np.array([prof.used], dtype=np.uint64)
            rows = S.allreduce_counts(prof.counts, reduce_device)
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                import torch

                t = torch.from_numpy(used.view(np.int64).copy())
                if reduce_device is not None:
                    t = t.to(reduce_device)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                used = t.cpu().numpy().view(np.uint64)
            prof_rows = rows[: int(used[0])]
            # per contig: each is one rank's; a sum of the zero-padded table is a gather
            tab = np.zeros((len(refs), 14), dtype=np.uint64)
            names = [n for n, _ in refs]
            for n_, v in per_contig:
                tab[names.index(n_)] += np.asarray(v, dtype=np.uint64).reshape(-1)
            tab = S.allreduce_counts(tab, reduce_device)
            seen = np.zeros(len(refs), dtype=np.uint64)
            for n_, _v in per_contig:
                seen[names.index(n_)] = 1
            seen = S.allreduce_counts(seen, reduce_device)
            per_contig = [(names[i], tab[i].reshape(7, 2)) for i in range(len(refs)) if seen[i]]
            if dist.is_available() and dist.is_initialized():
                dist.barrier()  # every shard is on disk
        report_text = report.render_json(site_stats, gc=gc, min_qual=min_qual, date=date, have_dbsnp=dbsnp is not None, filter_cts=cts, filter_bases=bases,
                                  base_filter=np.asarray(base_filter).tolist(), read_profile=prof_rows, contigs=per_contig)
        if sharded and shard_rank == 0:  # the header, then the contigs' shards in the header's order
            import os

            def shards():
                for tid in range(len(refs)):
                    p_ = "%s.shard%05d" % (bcf_path, tid)
                    if os.path.exists(p_):
                        with open(p_, "rb") as f_:
                            while True:
                                b_ = f_.read(1 << 24)
                                if not b_:
                                    break
                                yield b_
                        os.remove(p_)

            vcf.write_bcf(bcf_path, header, shards(), compressed)
        if report_path and (not sharded or shard_rank == 0):
            with open(report_path, "w") as f:
                f.write(report_text)
        summary = {"blocks": n_blocks, "records": n_records, "report": report_text, "filter_cts": cts, "contigs": [n for n, _ in per_contig]}
        if meth_path is not None:
            summary["meth_lines"] = meth_lines
        if variants_path is not None:
            summary["variant_records"] = int(var_totals[0])
            summary["variant_totals"] = tuple(int(v) for v in var_totals)
        if cpg_reads_path is not None:
            summary["cpg_reads_lines"] = reads_lines
            summary["cpg_reads_totals"] = tuple(int(v) for v in reads_totals)
        if asm_path is not None:
            summary["asm_lines"] = asm_lines
            summary["asm_totals"] = tuple(int(v) for v in asm_totals)
        if epi_path is not None:
            summary["epi_lines"] = epi_lines
            summary["epi_totals"] = tuple(int(v) for v in epi_totals)
        if pat_path is not None:
            summary["pat_lines"] = pat_lines
            summary["pat_totals"] = tuple(int(v) for v in pat_totals)
        if mbias_path is not None:
            summary["mbias_totals"] = tuple(int(v) for v in mbias_totals)
        if want_bw:
            summary["bigwig_sites"] = bw_sites
        if want_cov:
            summary["cov_bigwig_sites"] = cov_sites
        if want_bb:
            summary["bigbed_items"] = bb_sites
        if meth_regions_path is not None:
            summary["meth_region_lines"] = sum(b.count(b"\n") for b in region_out)
        if frag_path is not None:
            summary["frag_lines"] = sum(b.count(b"\n") for b in frag_out)
            summary["frag_totals"] = tuple(int(v) for v in frag_totals)
        return summary
    finally:
        if bw_writer is not None:
            bw_writer.close()
        if cov_writer is not None:
            cov_writer.close()
        if bb_writer is not None:
            bb_writer.close()
        if own:
            c.close()
        else:  # a supplied caller goes back as it came
            if on_device:
                c.dbsnp_detach()
            if want_regions and meth_regions_path is not None:
                c.meth_regions_attach([])
            if frag_path is not None:
                c.frag_attach([])
