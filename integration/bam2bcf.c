/*
 * bam2bcf.c — plain-C host program against libbscall_amd.so (gcc only): the reference's data path from a coordinate-sorted
 * BAM file and a FASTA reference to an uncompressed BCF stream and the JSON report, block by block, with nothing but the
 * C ABI of include/bscall_amd.h — what bs_call's four threads do between sam_read1() and bcf_write():
 *
 *   reader thread     bsc_bamdev_next_block         read_input / get_next_align_details ON THE DEVICE (round 6): the host inflates the BGZF
 *                                                   blocks (BAM2BCF_THREADS helpers, default: one per core), the records become blocks of
 *                                                   raw templates in HBM (csrc/bamdev.hip).  BAM2BCF_HOST_READER: bsc_bam_next_block, the
 *                                                   host reader of rounds 2-5 (csrc/bamio.c) — same bytes
 *   process thread    bsc_block_reference           get_sequence_string
 *   process + calc    bsc_block_bcf_raw             process_template_vector + meth_profile (on the device since round 5:
 *     + print                                       bsc_prepare_templates_device), call_genotypes_ML, _print_vcf_entry WITH the
 *                                                   encoding (the bcf_enc_* calls and bcf_write's fixed fields, csrc/bcfdev.hip), the
 *                                                   statistics: the block's BCF bytes come back
 *                                                   (BAM2BCF_HOST_BCF: bsc_block_records_raw, then bsc_bcf_block on this thread;
 *                                                   BAM2BCF_HOST_PREP: also the pre-processing on this thread,
 *                                                   bsc_prepare_templates_profile + bsc_block_records, as in round 4)
 *   output            fwrite                        bcf_write's write (-O u)
 *     + BGZF          bsc_bgzf_write[_device]       -O b: hts_open(..., "wb")'s BGZF layer, ON THE DEVICE (csrc/bgzfdev.hip): the header and
 *                     bsc_bgzf_take / _close        every block's kept stream go in, the completed members come out to the output thread
 *     + index         bsc_block_csi_kept            --index: bcf_index_build / tbx_index_build's product, made beside the file: a block's
 *                     bsc_csi_add / _finish         kept stream is scanned on the device (csrc/csidev.hip) before it goes to the compressor
 *   at the end        bsc_report_json               output_stats
 *
 * Not a replacement of the bs_call executable (no option parsing beyond -O / -D, regions, contig lists, compressed VCF): a worked
 * example of the calls in order, and the C twin of bs_call_amd/pipeline.py — tests/test_gpu_pipeline.py checks that both
 * write the same bytes.
 *
 *   make bam2bcf && bs_call_amd/lib/bam2bcf [-O u|b] [--format bcf|vcf] [--index] [-D dbsnp.idx] in.bam ref.fa out.bcf report.json [sample]
 *
 * A sharded run over ONE file (SURVEY.md 8e on real input; the reference's unit of parallelism is a process per contig set, README.md): rank r of n
 *   bam2bcf --rank r --world n in.bam ref.fa out.bcf report.json [sample]
 * takes its share of the contigs (whole contigs, longest first to the least loaded rank: bs_call_amd/shard.py's assignment), reads the
 * stretches of the file that hold them (bsc_bamdev_open_contigs: no index file), writes every contig's records to out.bcf.shardNNNNN and what
 * the report sums over to out.bcf.rankNNNNN.sums; no rank talks to another.  When all have finished,
 *   bam2bcf --merge n in.bam ref.fa out.bcf report.json [sample]
 * writes the header, the shards behind it in the header's contig order, and the report from the ranks' sums — the bytes of the single run
 * (tests/test_gpu_shard_bam.py).  tools/bam2bcf_sharded.sh starts the ranks, one per GPU, and merges.
 * The header's date lines are left out (the reference's --benchmark-mode) so that the output is reproducible.
 *
 * Output type (the reference's -O): -O u (the default) writes uncompressed BCF; -O b writes compressed BCF, BGZF on the device
 * (bsc_bgzf_*, csrc/bgzfdev.hip): the header goes in through bsc_bgzf_write, every block's kept stream through bsc_bgzf_write_device, and
 * the members bsc_bgzf_take hands over go to the output thread, which writes them at the running compressed offset; bsc_bgzf_close gives
 * the last member and the end-of-file marker.  Decompressed, the file is byte for byte the -O u file.
 * Format: --format bcf (the default) writes BCF2 records; --format vcf writes VCF TEXT — the same header text without the BCF magic, length
 * and terminator, then every block's lines, encoded on the device too (bsc_block_vcf_rawdev_keep, csrc/vcftextdev.hip): with -O u the
 * reference's -O v, with -O b (the same BGZF path) its -O z.  A single run on the device reader only (no --rank / --merge, no BAM2BCF_HOST_*).  -O b needs the device reader and
 * encoder and a single run (a shard compressed on its own would cut its members elsewhere than the single run does).
 * Index: --index (with -O b, either format) writes out.bcf.csi, a CSI index (min_shift 14) of the compressed file, while the file is written: the
 * block's kept stream is scanned where it lies, right behind the encoder on the context's stream (bsc_block_csi_kept: the runs of records per
 * 16 384-position window and their offsets), the entries are noted at the writer's logical length (bsc_csi_add) before the stream goes into
 * the compressor, and bsc_csi_finish turns the offsets into virtual offsets from the members' compressed sizes once the file is closed.  The
 * data file's bytes are those of the run without --index.  Without -O b, or with --rank / --merge / BAM2BCF_HOST_*: refused.
 * dbSNP (the reference's -D): -D index names the records, forces out the homozygous-reference records of the index's fq_mask sites and fills
 * the report's dbSNP counters.  Each contig of the index is loaded by the thread that loads its reference, kept in HBM (bsc_dbsnp_attach at
 * the contig change) and the blocks' flags and names are made there (csrc/dbsnpdev.hip): the block calls pass NULL for both.  The header is
 * the --benchmark-mode header, which has no ##dbsnp line.  With either -O and either --format; a single run on the device reader only.
 * Methylation table: --meth out.bed writes, beside the BCF / VCF of the same run, the bedMethyl line of every cytosine the rule of
 * include/bscall_amd.h admits (CpG cytosines called CC / GG; --meth-all: CHG / CHH too; --meth-min-cov N, --meth-min-gq N, --meth-pass: the
 * thresholds), encoded on the device from the arrays the block call left there (bsc_block_meth_kept, csrc/methdev.hip) — nothing is read
 * back out of the records' stream.  The table changes hands like the block's stream (bsc_meth_stream_detach) and goes through the same
 * output thread, as one more job of its own file; with -O b through a second BGZF writer.  With either --format, with -D and --index; the
 * BCF / VCF, the .csi and the report are those of the run without it.  A single run on the device reader only.  --meth-merge: the table
 * is the combined-strand one — a line per CpG dinucleotide, both strands' counts added (bsc_block_meth_cpg_kept); not with --meth-all.
 *
 * --meth-bgzf: the table leaves the device as BGZF whatever -O says (with -O b it does anyway).  --meth-index tbi|csi: out.bed.gz.tbi /
 * out.bed.gz.csi beside the compressed table, made while the table is written — the block's table is scanned where it lies, by the
 * encoder's own tile offsets (bsc_block_meth_index_kept, csrc/beddev.hip: the runs of lines per 16 384-base window, a line across a border
 * apart), noted at the table writer's logical length (bsc_tbx_add) and turned into virtual offsets once the table is closed
 * (bsc_tbx_finish).  The table's bytes are those of the run without it.  Needs --meth and -O b or --meth-bgzf; a single run on the device reader.
 * --meth-bigwig out.bw: the methylation level per cytosine as a bigWig track (include/bscall_amd.h has the rule and the file's layout): every
 * block's data sections and summaries on the device (bsc_block_bigwig_kept, csrc/bigwigdev.hip), read into a host buffer and handed to the
 * output thread as one more job, which bsc_bigwig_add places in the track's own file; bsc_bigwig_finish writes the indexes, the zoom levels and
 * the header at the end.  --meth-bigwig-section n: sites a section (default 1024); --meth-bigwig-zoom n: the level-0 zoom window (default
 * 1024).  The --meth-* thresholds and --meth-all apply; the track is per cytosine even with --meth-merge; --meth is not needed.
 * --meth-bigbed out.bb: the per-cytosine table as a bigBed file (include/bscall_amd.h has the rule and the file's layout): every block's items,
 * block and window summaries on the device (bsc_block_bigbed_kept, csrc/bigbeddev.hip), handed to the output thread as one more job for
 * bsc_bigbed_add; bsc_bigbed_finish writes the indexes, the zoom levels and the header at the end.  --meth-bigbed-items n: sites a block
 * (default 512); --meth-bigbed-zoom n: the level-0 zoom window (default 1024); the --meth-all / --meth-min-cov / --meth-min-gq / --meth-pass
 * thresholds apply.  --meth-bigbed-compress: every block leaves the device as a zlib stream (bsc_block_bigbed_deflate) for bsc_bigbed_add_z;
 * needs --meth-bigbed and at most BSC_BB_Z_ITEMS_MAX sites a block.  Refused like --meth-bigwig in a sharded run and on the BAM2BCF_HOST_* paths.
 * --meth-bigwig-compress: the file readers meet in practice — every section leaves the device as a zlib stream (bsc_block_bigwig_deflate,
 * csrc/zlibdev.hip), the job carries the streams and their sizes for bsc_bigwig_add_z, and bsc_bigwig_finish deflates the zoom blocks.  Needs
 * --meth-bigwig or --cov-bigwig; sections of at most 8157 sites.
 * --cov-bigwig cov.bw: the depth a + b of the same sites as a second bigWig track (the coverage rule of include/bscall_amd.h), alone or beside
 * --meth-bigwig.  With both, ONE bsc_block_bigwig_tracks_kept call (csrc/bwcovdev.hip, mask 3) reduces the block for the two files: the
 * per-position arrays are read once.  --meth-bigwig-section, --meth-bigwig-zoom and --meth-bigwig-compress apply to both files (the
 * coverage sections through bsc_block_bigwig_cov_deflate); each file is a job of its own for the output thread.  Refused where --meth-bigwig is.
 * Without --cov-bigwig the program makes the calls it made before the switch existed.
 *
 * --meth-regions regions.bed --meth-regions-out out.tsv: the per-region methylation summary — per interval of the BED file the cytosines
 * inside it added up on the device (bsc_meth_regions_attach at the contig change, where -D attaches; bsc_block_meth_regions_kept behind
 * every block; bsc_meth_regions_read at the next contig change and at the end), ten columns a region: chrom start end name sites A+B A B
 * level mean.  --meth-window n in the BED's place: fixed tiles of n bases over every contig.  The --meth-* thresholds and --meth-all
 * apply; --meth is not needed.  Contigs come out in the order their blocks do (the BAM header's); a contig without a block gives no line.
 *
 * --meth-reads out.tsv: the read-level CpG concordance table (include/bscall_amd.h has the rule) — a line per reference CpG that a template
 * reads: chrom start end m u e d dist mm mu um uu, start / end those of the --meth-merge line of the same CpG.  Behind every block
 * bsc_block_cpg_reads_kept walks the prepared templates, reads and reference codes the block call left in HBM; the table is detached
 * (bsc_cpg_reads_stream_detach) and goes to the output thread as one more job for its own file, through a BGZF writer of its own under -O b
 * or --meth-bgzf.  --meth-reads-min-sites n (default 4): a template is judged concordant / discordant from n CpGs with a state on;
 * --meth-reads-min-cov n (default 1): m + u a line needs.  Not gated by the called genotype (a C>T SNP at a reference CpG reads as
 * unmethylated): the join with the --meth-merge table is the filter.  Refused where --meth is: sharded runs, the BAM2BCF_HOST_* paths.
 * Without the switch the program makes the calls it made before the switch existed.
 *
 * --meth-asm out.tsv: the allele-specific methylation table (include/bscall_amd.h has the rule) — a line per (heterozygous SNP the block's call
 * wrote, reference CpG within --meth-asm-window bases of it) that templates of both alleles read: chrom start end snp_pos gt m1 u1 m2 u2 aq dist,
 * start / end those of the --meth-merge and --meth-reads lines of the same CpG, aq the phred of Fisher's two-sided p of {m1, u1, m2, u2}.  The
 * lines are ordered by SNP, then by CpG — NOT by start: the windows of neighbouring SNPs overlap — and the file has no index.  Behind every
 * block bsc_block_asm_kept reads the dense records, the prepared templates, reads and reference codes the block call left in HBM; the table is
 * detached (bsc_asm_stream_detach) and goes to the output thread as one more job for its own file, through a BGZF writer of its own when the
 * name ends in .gz, under -O b or --meth-bgzf.  --meth-asm-window n (default 500, 1 .. 65535), --meth-asm-min-qual n (default 20: the QUAL a SNP
 * needs), --meth-asm-min-cov n (default 2: m1 + u1 and m2 + u2 a line needs), --meth-asm-pass (PASS SNPs only).  Refused where --meth-reads is.
 * Without the switch the program makes the calls it made before the switch existed.
 *
 * --meth-epialleles out.tsv: the epiallele table (include/bscall_amd.h has the rule) — a line per window of four consecutive reference CpGs
 * that templates read whole: chrom start end n k c0 .. c15, c<code> the templates with that methylation pattern (bit 0 the leftmost CpG, 15 = all
 * methylated), n their sum, k the patterns seen; start is that of the --meth-merge and --meth-reads lines of the window's first CpG.  No float
 * is written: epipolymorphism and entropy are the reader's (bs_call_amd/epialleles.py has both).  Behind every block bsc_block_epi_kept walks
 * the prepared templates, reads and reference codes the block call left in HBM; the table is detached (bsc_epi_stream_detach) and goes to the
 * output thread as one more job for its own file, through a BGZF writer of its own when the name ends in .gz, under -O b or --meth-bgzf.
 * --meth-epialleles-min-cov n (default 10): the n a line needs.  Refused where --meth-reads is.  Without the switch the program makes the calls
 * it made before the switch existed.
 *
 * --meth-pat out.pat: the per-read CpG pattern table, PAT (include/bscall_amd.h has the rule) — a line per distinct methylation string of the
 * block's templates: chrom index pattern count, the pattern in C (methylated) / T (unmethylated) / . (no call) over consecutive reference CpGs
 * from the index on, identical strings collapsed, lines sorted by index, then pattern: the interchange format of the read-level methylation
 * tools.  The bytes are wgbstools-unpinned (no copy of that tool is at hand: the format is written from its description), and the index is the
 * CpG's 1-based ordinal within its CONTIG, not genome-wide (bs_call_amd/pat.py has contig_offsets and shift to convert); a line holds 64 CpGs at
 * the most, a longer molecule's string is cut.  Behind every block bsc_block_pat_kept walks the prepared templates, reads and reference codes
 * the block call left in HBM, sorts and collapses on the device; index_base is kept per contig: bsc_pat_count_sites advances it over the stretch
 * between the previous block's start and this block's, and it is reset at the contig change.  Blocks of a contig do not overlap, so a key never
 * occurs in two blocks and the concatenated tables are sorted within the contig.  The table is detached (bsc_pat_stream_detach) and goes to
 * the output thread as one more job for its own file, through a BGZF writer of its own when the name ends in .gz, under -O b or --meth-bgzf.
 * --meth-pat-min-sites n (default 1): the states a template needs.  Refused where --meth-epialleles is.  Without the switch the program makes
 * the calls it made before the switch existed.
 *
 * --meth-frags out.tsv: the per-region fragment methylation summary (include/bscall_amd.h has the rule) over the intervals of --meth-regions
 * or --meth-window — per interval the templates that are mostly unmethylated, mixed and mostly methylated within it, twelve columns: chrom
 * start end name frags U X M K Mm disc short, whose first four join the --meth-regions-out lines.  bsc_frag_attach at the contig change, where
 * the region summary attaches; bsc_block_frag_kept behind every block; bsc_frag_read and bsc_frag_format at the next contig change and at the
 * end.  --meth-frags-min-sites n (default 3), --meth-frags-u-max pct (25), --meth-frags-m-min pct (75).  With --meth-frags,
 * --meth-regions-out may be left out.  Refused where --meth-regions is.  Without the switch the program makes the calls it made before the
 * switch existed.
 *
 * --mbias out.tsv: the M-bias table (include/bscall_amd.h has the rule) — methylated and unmethylated calls per sequencing cycle, by read 1 /
 * read 2, bisulfite strand and CpG / CHG / CHH, from the RAW templates as sequenced (no trim, clip or overlap edit): what -L / -R and the
 * under-conversion rate are chosen from.  Behind every block bsc_block_mbias_rawdev walks the block's raw arrays, still in the reader's
 * buffers, into one accumulator of the context's; ONE table per run, over every block of every contig, is read (bsc_mbias_read), formatted
 * (bsc_mbias_format) and written at the end, and one more line with its totals goes to stdout.  --mbias-cycles n (default 512, 1 .. 1024):
 * the cycles the table holds; calls beyond them are counted in the line on stdout.  Plain text whatever -O says.  Refused where
 * --meth-regions is: sharded runs, the BAM2BCF_HOST_* paths.  Without the switch the program makes the calls it made before the switch
 * existed.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <bscall_amd.h>

#define CHECK(call)                                                          \
  do {                                                                       \
    long rc_ = (long)(call);                                                 \
    if (rc_ < 0) {                                                           \
      fprintf(stderr, "%s failed (%ld): %s\n", #call, rc_, bsc_last_error()); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static double now(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static void *xrealloc(void *p, size_t n) {
  void *q = realloc(p, n ? n : 1);
  if (!q) {
    fprintf(stderr, "out of memory\n");
    exit(1);
  }
  return q;
}

static void *pinned(size_t n) { /* page-locked: the copy-out is a true DMA, queued behind the kernels */
  void *p = bsc_alloc_host(n);
  if (!p) {
    fprintf(stderr, "out of page-locked memory (%zu bytes)\n", n);
    exit(1);
  }
  return p;
}

/* The output thread (bcf_write's write).  A block's stream stays on the device (bsc_block_bcf_rawdev_keep) and is HANDED to this thread
 * (bsc_bcf_stream_detach): it reads it out in pieces of 32 MB — two page-locked buffers, the next piece's copy in flight on a stream of
 * its own while the last is written — and writes each at its offset of its file, then gives the buffer back (bsc_detached_free: the next
 * blocks take theirs from what came back).  The main thread meanwhile pulls the next block out of the reader and calls it: on a file of
 * several contigs the inflate (the reader's bound) and the write (this thread's: ~10 GB/s into the page cache) overlap instead of taking
 * turns — round 6's first form read the pieces on the main thread, which therefore waited for this one with the reader's slabs full.
 * ONE writer: three of them writing pieces of one file in parallel were 2.5 x slower (0.70 s against 0.28 for the 2.9 GB of a contig-sized
 * block: writes to one inode take turns anyway).  Page-locking a host buffer for a whole stream would cost more than the calling. */
#define PIECE ((size_t)32 << 20)
#define N_JOB 4 /* (a block is two jobs with --meth, three with --variants beside it, four with --meth-reads, five with --meth-asm, six with --meth-epialleles, seven with --meth-pat: a push waits for a
                 * free slot) */
typedef struct {
  void *d;        /* the stream on the device; NULL: only close_fd */
  uint64_t n, at; /* its length, where it goes in the file */
  int fd, close_fd;
  /* --meth-bigwig: a block's data in a host buffer of the job's own with copies of its summaries, for bsc_bigwig_add (which places them in the
   * track's file itself); freed here */
  bsc_bigwig *bw;
  uint32_t bw_tid;
  void *bw_data;
  bsc_bw_sum *bw_sec, *bw_zoom;
  uint64_t bw_n_sec, bw_n_zoom;
  uint32_t *bw_zsizes; /* --meth-bigwig-compress: bw_data holds the sections' zlib streams, these are their sizes */
  /* --meth-bigbed: the same for bsc_bigbed_add / _add_z — the block's items (or their zlib streams: bb_zsizes, bb_raw the plain length) */
  bsc_bigbed *bb;
  void *bb_data;
  bsc_bb_sum *bb_blk, *bb_zoom;
  uint64_t bb_n_blk, bb_n_zoom, bb_raw;
  uint32_t *bb_zsizes;
} out_job;
typedef struct {
  bsc_context *ctx;
  uint8_t *buf[2];
  out_job job[N_JOB];
  int head, count, quit, failed, started;
  double t_wait, t_write, t_idle; /* the output thread's own account (BAM2BCF_TIMING) */
  pthread_mutex_t mu;
  pthread_cond_t cv;
  pthread_t th;
} out_writer;
static double now(void);
static void *writer_main(void *a) {
  out_writer *w = a;
  for (;;) {
    double t0 = now(), t1;
    pthread_mutex_lock(&w->mu);
    while (!w->count && !w->quit) pthread_cond_wait(&w->cv, &w->mu);
    w->t_idle += (t1 = now()) - t0;
    if (!w->count) {
      pthread_mutex_unlock(&w->mu);
      return NULL;
    }
    const out_job j = w->job[w->head];
    pthread_mutex_unlock(&w->mu);
    int bad = 0;
    if (j.d) {
      uint64_t off = 0;
      int k = 0;
      size_t take = j.n < PIECE ? (size_t)j.n : PIECE;
      if (take && bsc_detached_read(w->ctx, j.d, 0, take, w->buf[0]) < 0) bad = 1;
      while (off < j.n && !bad) {
        t0 = now();
        if (bsc_detached_wait(w->ctx) < 0) bad = 1; /* piece k is here */
        w->t_wait += (t1 = now()) - t0;
        const uint64_t next = off + take;
        const size_t take2 = j.n - next < PIECE ? (size_t)(j.n - next) : PIECE;
        if (!bad && take2 && bsc_detached_read(w->ctx, j.d, next, take2, w->buf[k ^ 1]) < 0) bad = 1; /* the next one: while this one is written */
        size_t done = 0;
        while (done < take && !bad) {
          const ssize_t r = pwrite(j.fd, w->buf[k] + done, take - done, (off_t)(j.at + off + done));
          if (r <= 0) bad = 1;
          else done += (size_t)r;
        }
        w->t_write += now() - t1;
        off = next;
        take = take2;
        k ^= 1;
      }
      if (bsc_detached_free(w->ctx, j.d) < 0) bad = 1;
    }
    if (j.bw) {
      const int rc = j.bw_zsizes ? bsc_bigwig_add_z(j.bw, j.bw_tid, j.bw_data, j.n, j.bw_zsizes, j.bw_sec, j.bw_n_sec, j.bw_zoom, j.bw_n_zoom)
                                 : bsc_bigwig_add(j.bw, j.bw_tid, j.bw_data, j.n, j.bw_sec, j.bw_n_sec, j.bw_zoom, j.bw_n_zoom);
      if (rc < 0) {
        fprintf(stderr, "bam2bcf: %s\n", bsc_last_error());
        bad = 1;
      }
      free(j.bw_zsizes);
      free(j.bw_data);
      free(j.bw_sec);
      free(j.bw_zoom);
    }
    if (j.bb) {
      const int rc = j.bb_zsizes ? bsc_bigbed_add_z(j.bb, j.bw_tid, j.bb_data, j.n, j.bb_zsizes, j.bb_raw, j.bb_blk, j.bb_n_blk, j.bb_zoom, j.bb_n_zoom)
                                 : bsc_bigbed_add(j.bb, j.bw_tid, j.bb_data, j.n, j.bb_blk, j.bb_n_blk, j.bb_zoom, j.bb_n_zoom);
      if (rc < 0) {
        fprintf(stderr, "bam2bcf: %s\n", bsc_last_error());
        bad = 1;
      }
      free(j.bb_zsizes);
      free(j.bb_data);
      free(j.bb_blk);
      free(j.bb_zoom);
    }
    if (j.close_fd && j.fd >= 0) close(j.fd);
    pthread_mutex_lock(&w->mu);
    if (bad) w->failed = 1;
    w->head = (w->head + 1) % N_JOB;
    w->count--;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
  }
}
static void writer_push(out_writer *w, out_job j) {
  pthread_mutex_lock(&w->mu);
  while (w->count == N_JOB) pthread_cond_wait(&w->cv, &w->mu);
  w->job[(w->head + w->count) % N_JOB] = j;
  w->count++;
  pthread_cond_broadcast(&w->cv);
  pthread_mutex_unlock(&w->mu);
}

/* The next contig's reference in the background (load_sequence + the GC bins): a thread of its own reads the FASTA while the reader's helpers
 * inflate.  One request in flight. */
typedef struct {
  const char *fasta, *name;
  uint64_t want;
  uint8_t *codes, *gc;
  uint64_t codes_len, n_bins;
  uint32_t gc_start;
  int rc, tid;
  char err[256];
  pthread_t th;
  int running;
} ref_job;
static bsc_dbsnp *g_dbsnp; /* -D: the contig's entries are loaded behind its reference; the main thread attaches them (a snapshot) before the next job starts */
static void *ref_main(void *a) {
  ref_job *j = a;
  j->codes = malloc(j->want ? j->want : 1);
  j->gc = NULL;
  j->rc = j->codes ? bsc_fasta_contig(j->fasta, j->name, j->codes, j->want, &j->codes_len) : -1;
  if (j->rc >= 0) {
    j->gc = malloc((size_t)(j->codes_len / 100 + 1));
    j->rc = j->gc ? bsc_gc_bins(j->codes, j->codes_len, &j->gc_start, j->gc, j->codes_len / 100 + 1, &j->n_bins) : -1;
  }
  if (j->rc >= 0 && g_dbsnp) j->rc = bsc_dbsnp_load_contig(g_dbsnp, j->name, NULL);
  if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", bsc_last_error());
  return NULL;
}
static void ref_start(ref_job *j, const char *fasta, const char *name, uint64_t len, int tid) {
  memset(j, 0, sizeof *j);
  j->fasta = fasta;
  j->name = name;
  j->want = len;
  j->tid = tid;
  j->running = pthread_create(&j->th, NULL, ref_main, j) == 0;
  if (!j->running) ref_main(j);
}

/* the header print_vcf_header assembles in --benchmark-mode (src/print_vcf.c:621-745) */
static void write_header(FILE *f, int n_refs, const char *const *names, const uint32_t *lens, const char *sample, int text) {
  static const char *const defs[] = {
      "##INFO=<ID=CX,Number=1,Type=String,Description=\"5 base sequence context (from position -2 to +2 on the positive strand) determined from the reference\">",
      "##FILTER=<ID=fail,Description=\"No sample passed filters\">",
      "##FILTER=<ID=q20,Description=\"Genotype Quality below 20\">",
      "##FILTER=<ID=qd2,Description=\"Quality By Depth below 2\">",
      "##FILTER=<ID=fs60,Description=\"Fisher Strand above 60\">",
      "##FILTER=<ID=mq40,Description=\"RMS Mapping Quality below 40\">",
      "##FILTER=<ID=mac1,Description=\"Minor allele count <= 1\">",
      "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
      "##FORMAT=<ID=FT,Number=1,Type=String,Description=\"Sample Genotype Filter\">",
      "##FORMAT=<ID=GL,Number=G,Type=Float,Description=\"Genotype Likelihood\">",
      "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Phred scaled conditional genotype quality\">",
      "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Read Depth (non converted reads only)\">",
      "##FORMAT=<ID=MQ,Number=1,Type=Integer,Description=\"RMS Mapping Quality\">",
      "##FORMAT=<ID=QD,Number=1,Type=Integer,Description=\"Quality By Depth (Variant quality / read depth (non-converted reads only))\">",
      "##FORMAT=<ID=MC8,Number=8,Type=Integer,Description=\"Base counts: non-informative for methylation (ACGT) followed by informative for methylation (ACGT)\">",
      "##FORMAT=<ID=AMQ,Number=.,Type=Integer,Description=\"Average base quailty for where MC8 base count non-zero\">",
      "##FORMAT=<ID=CS,Number=1,Type=String,Description=\"Strand of Cytosine relative to reference sequence (+/-/+-/NA)\">",
      "##FORMAT=<ID=CG,Number=1,Type=String,Description=\"CpG Status (from genotype calls: Y/N/H/?)\">",
      "##FORMAT=<ID=CX,Number=1,Type=String,Description=\"5 base sequence context (from position -2 to +2 on the positive strand) determined from genotype call\">",
      "##FORMAT=<ID=FS,Number=1,Type=Integer,Description=\"Phred scaled log p-value from Fishers exact test of strand bias\">"};
  size_t cap = 1 << 16, len = 0;
  char *t = xrealloc(NULL, cap);
#define ADD(...)                                                  \
  do {                                                            \
    for (;;) {                                                    \
      const int w_ = snprintf(t + len, cap - len, __VA_ARGS__);   \
      if ((size_t)w_ < cap - len) {                               \
        len += (size_t)w_;                                        \
        break;                                                    \
      }                                                           \
      cap *= 2;                                                   \
      t = xrealloc(t, cap);                                       \
    }                                                             \
  } while (0)
  ADD("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n");
  for (int i = 0; i < n_refs; i++) ADD("##contig=<ID=%s,length=%u>\n", names[i], lens[i]);
  for (size_t i = 0; i < sizeof defs / sizeof defs[0]; i++) ADD("%s\n", defs[i]);
  ADD("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", sample);
#undef ADD
  if (text) { /* --format vcf: the header text as it is — no magic, no length, no terminator */
    fwrite(t, 1, len, f);
    free(t);
    return;
  }
  const uint32_t l_text = (uint32_t)len + 1; /* the terminator is part of the BCF header text */
  fwrite("BCF\2\2", 1, 5, f);
  fwrite(&l_text, 4, 1, f); /* little-endian hosts only, like the rest of this example */
  fwrite(t, 1, len + 1, f);
  free(t);
}

/* ---- the sharded run ------------------------------------------------------------------------------------------------------------- */
#define PROF_CAP 4096
typedef struct { /* what a rank hands the merge: everything the report adds up */
  uint64_t magic, n_ref, n_blocks, n_records, malformed;
  uint64_t filter_cts[15], filter_bases[15], base_filter[5];
  uint64_t prof_used, prof[PROF_CAP][4];
  bsc_site_stats total;
  /* followed by: gc[BSC_COV_CAP * 101], then per contig {seen, totals[14]} x n_ref */
} rank_sums;
#define SUMS_MAGIC 0x3173635f6d756273ull

/* whole contigs to ranks, longest first, each to the least loaded rank (ties: the lower index) — bs_call_amd/shard.py assign_contigs */
static int *assign_contigs(const uint32_t *len, int n_ref, int world) {
  int *owner = calloc((size_t)n_ref + 1, sizeof *owner), *order = calloc((size_t)n_ref + 1, sizeof *order);
  uint64_t *load = calloc((size_t)world, sizeof *load);
  for (int i = 0; i < n_ref; i++) order[i] = i;
  for (int i = 1; i < n_ref; i++) { /* by (-length, index): an insertion sort keeps equal lengths in index order */
    const int v = order[i];
    int j = i;
    while (j > 0 && len[order[j - 1]] < len[v]) {
      order[j] = order[j - 1];
      j--;
    }
    order[j] = v;
  }
  for (int k = 0; k < n_ref; k++) {
    int best = 0;
    for (int r = 1; r < world; r++)
      if (load[r] < load[best]) best = r;
    owner[order[k]] = best;
    load[best] += len[order[k]];
  }
  free(order);
  free(load);
  return owner;
}

static void header_of(const char *bam_path, int *n_ref, const char ***names, uint32_t **lens, bsc_bamstream **keep) {
  bsc_bamstream *h = NULL;
  CHECK(bsc_bamstream_open_contigs(bam_path, 1, 0, 0, NULL, 0, &h)); /* no contig at all: the header alone */
  *n_ref = bsc_bamstream_n_refs(h);
  *names = calloc((size_t)*n_ref + 1, sizeof **names);
  *lens = calloc((size_t)*n_ref + 1, sizeof **lens);
  for (int i = 0; i < *n_ref; i++) {
    (*names)[i] = bsc_bamstream_ref_name(h, i);
    (*lens)[i] = bsc_bamstream_ref_len(h, i);
  }
  *keep = h; /* (the names live in it) */
}

static void write_header(FILE *f, int n_refs, const char *const *names, const uint32_t *lens, const char *sample, int text);

static int merge_main(int world, char **argv, const char *sample) {
  int n_ref;
  const char **names;
  uint32_t *lens;
  bsc_bamstream *hs;
  header_of(argv[1], &n_ref, &names, &lens, &hs);
  FILE *out = fopen(argv[3], "wb");
  if (!out) {
    perror(argv[3]);
    return 1;
  }
  write_header(out, n_ref, names, lens, sample, 0);
  char *path = malloc(strlen(argv[3]) + 64), *buf = malloc(1 << 24);
  for (int t = 0; t < n_ref; t++) { /* the contigs' shards in the header's order */
    sprintf(path, "%s.shard%05d", argv[3], t);
    FILE *f = fopen(path, "rb");
    if (!f) continue;
    size_t n;
    while ((n = fread(buf, 1, 1 << 24, f)) > 0) fwrite(buf, 1, n, out);
    fclose(f);
    remove(path);
  }
  fclose(out);
  /* the report: every number in it is a sum over positions / reads / templates, the read profile's length the longest any rank saw */
  rank_sums *acc = calloc(1, sizeof *acc), *one = malloc(sizeof *one);
  uint64_t *gc = calloc((size_t)BSC_COV_CAP * 101, 8), *gc1 = malloc((size_t)BSC_COV_CAP * 101 * 8);
  uint64_t *ct = calloc((size_t)n_ref * 15 + 1, 8), *ct1 = malloc(((size_t)n_ref * 15 + 1) * 8);
  for (int r = 0; r < world; r++) {
    sprintf(path, "%s.rank%05d.sums", argv[3], r);
    FILE *f = fopen(path, "rb");
    if (!f || fread(one, sizeof *one, 1, f) != 1 || one->magic != SUMS_MAGIC || one->n_ref != (uint64_t)n_ref ||
        fread(gc1, 8, (size_t)BSC_COV_CAP * 101, f) != (size_t)BSC_COV_CAP * 101 || fread(ct1, 8, (size_t)n_ref * 15, f) != (size_t)n_ref * 15) {
      fprintf(stderr, "bam2bcf --merge: %s is missing or not a rank's sums of this input\n", path);
      return 1;
    }
    fclose(f);
    remove(path);
    acc->n_blocks += one->n_blocks;
    acc->n_records += one->n_records;
    acc->malformed += one->malformed;
    for (int i = 0; i < 15; i++) acc->filter_cts[i] += one->filter_cts[i], acc->filter_bases[i] += one->filter_bases[i];
    for (int i = 0; i < 5; i++) acc->base_filter[i] += one->base_filter[i];
    if (one->prof_used > acc->prof_used) acc->prof_used = one->prof_used;
    for (int i = 0; i < PROF_CAP * 4; i++) (&acc->prof[0][0])[i] += (&one->prof[0][0])[i];
    { /* bsc_site_stats: the leading words are counters, the last 4 x 101 doubles (include/bscall_amd.h) */
      const size_t n_int = (sizeof(bsc_site_stats) - 404 * sizeof(double)) / 8;
      uint64_t *a = (uint64_t *)&acc->total;
      const uint64_t *b = (const uint64_t *)&one->total;
      for (size_t i = 0; i < n_int; i++) a[i] += b[i];
      double *ad = (double *)(a + n_int);
      const double *bd = (const double *)(b + n_int);
      for (int i = 0; i < 404; i++) ad[i] += bd[i];
    }
    for (size_t i = 0; i < (size_t)BSC_COV_CAP * 101; i++) gc[i] += gc1[i];
    for (size_t i = 0; i < (size_t)n_ref * 15; i++) ct[i] += ct1[i];
  }
  if (acc->malformed)
    fprintf(stderr, "bam2bcf: warning: %llu BAM records dropped, their CIGAR does not cover the sequence (damaged input?)\n", (unsigned long long)acc->malformed);
  bsc_report rep;
  memset(&rep, 0, sizeof rep);
  rep.under_conv = 0.01;
  rep.over_conv = 0.05;
  rep.mapq_thresh = 20;
  rep.min_qual = 20;
  rep.day = 1, rep.month = 1, rep.year = 2000;
  memcpy(rep.filter_cts, acc->filter_cts, sizeof rep.filter_cts);
  memcpy(rep.filter_bases, acc->filter_bases, sizeof rep.filter_bases);
  memcpy(rep.base_filter, acc->base_filter, sizeof rep.base_filter);
  rep.total = &acc->total;
  rep.gc = gc;
  rep.read_profile = &acc->prof[0][0];
  rep.n_read_profile = (uint32_t)acc->prof_used;
  bsc_contig_totals *listed = calloc((size_t)n_ref + 1, sizeof *listed);
  uint32_t nl = 0;
  for (int i = 0; i < n_ref; i++)
    if (ct[(size_t)i * 15]) {
      listed[nl].name = names[i];
      memcpy(listed[nl].snps, ct + (size_t)i * 15 + 1, 14 * 8);
      nl++;
    }
  rep.contigs = listed;
  rep.n_contigs = nl;
  const long need = bsc_report_json(&rep, NULL, 0);
  CHECK(need);
  char *text = xrealloc(NULL, (size_t)need + 1);
  bsc_report_json(&rep, text, (size_t)need + 1);
  FILE *fr = fopen(argv[4], "w");
  if (!fr) {
    perror(argv[4]);
    return 1;
  }
  fwrite(text, 1, (size_t)need, fr);
  fclose(fr);
  printf("%llu blocks, %llu records written\n", (unsigned long long)acc->n_blocks, (unsigned long long)acc->n_records);
  bsc_bamstream_close(hs);
  return 0;
}

/* --meth-regions: the attached contig's accumulators read and its lines appended */
static uint64_t regions_flush(bsc_context *ctx, FILE *f, const char *contig, const bsc_meth_region *regs, const char *const *names, uint64_t n) {
  if (!n) return 0;
  uint64_t *acc = xrealloc(NULL, (size_t)n * 4 * sizeof *acc);
  CHECK(bsc_meth_regions_read(ctx, acc, n));
  const long need = bsc_meth_regions_format(contig, regs, names, acc, (size_t)n, NULL, 0);
  CHECK(need);
  char *buf = xrealloc(NULL, (size_t)need);
  CHECK(bsc_meth_regions_format(contig, regs, names, acc, (size_t)n, buf, (size_t)need));
  if (fwrite(buf, 1, (size_t)need, f) != (size_t)need) {
    perror("--meth-regions-out");
    exit(1);
  }
  free(buf);
  free(acc);
  return n;
}

/* --meth-frags: the attached contig's fragment accumulators read and its lines appended */
static uint64_t frags_flush(bsc_context *ctx, FILE *f, const char *contig, const bsc_meth_region *regs, const char *const *names, uint64_t n) {
  if (!n) return 0;
  uint64_t *acc = xrealloc(NULL, (size_t)n * BSC_FRAG_N_SUMS * sizeof *acc);
  CHECK(bsc_frag_read(ctx, acc, n));
  const long need = bsc_frag_format(contig, regs, names, acc, (size_t)n, NULL, 0);
  CHECK(need);
  char *buf = xrealloc(NULL, (size_t)(need ? need : 1));
  CHECK(bsc_frag_format(contig, regs, names, acc, (size_t)n, buf, (size_t)need));
  if (fwrite(buf, 1, (size_t)need, f) != (size_t)need) {
    perror("--meth-frags");
    exit(1);
  }
  free(buf);
  free(acc);
  return n;
}

int main(int argc, char **argv) {
  int rank = -1, world = 1, merge = 0, bgzf = 0, text = 0, index = 0, meth_merge = 0;
  const char *dbsnp_path = NULL, *meth_path = NULL, *regions_path = NULL, *regions_out_path = NULL, *bigwig_path = NULL, *cov_path = NULL;
  uint32_t meth_window = 0;
  bsc_bw_params bwpar;
  bsc_bw_params_default(&bwpar);
  int bigwig_z = 0;
  const char *bigbed_path = NULL;
  bsc_bb_params bbpar;
  bsc_bb_params_default(&bbpar);
  int bigbed_z = 0;
  int meth_bgzf = 0;
  const char *meth_index = NULL; /* --meth-index tbi | csi */
  bsc_meth_params mpar;
  bsc_meth_params_default(&mpar);
  const char *variants_path = NULL; /* --variants out: the records with an ALT allele, in the run's format */
  bsc_var_params vpar;
  bsc_var_params_default(&vpar);
  int variants_opts = 0;
  const char *reads_path = NULL; /* --meth-reads out.tsv: the read-level CpG concordance table */
  bsc_cpg_reads_params crpar;
  bsc_cpg_reads_params_default(&crpar);
  int reads_opts = 0;
  const char *asm_path = NULL; /* --meth-asm out.tsv: the allele-specific methylation table */
  bsc_asm_params aspar;
  bsc_asm_params_default(&aspar);
  int asm_opts = 0;
  const char *epi_path = NULL; /* --meth-epialleles out.tsv: the epiallele table */
  bsc_epi_params eppar;
  bsc_epi_params_default(&eppar);
  int epi_opts = 0;
  if (argc >= 2 && !strcmp(argv[argc - 1], "--meth-epialleles") && (argc == 2 || strcmp(argv[argc - 2], "--meth-epialleles"))) {
    fprintf(stderr, "%s: --meth-epialleles takes the path of the epiallele table to write\n", argv[0]);
    return 2;
  }
  const char *pat_path = NULL; /* --meth-pat out.pat: the per-read CpG pattern table */
  bsc_pat_params ptpar;
  bsc_pat_params_default(&ptpar);
  int pat_opts = 0;
  if (argc >= 2 && !strcmp(argv[argc - 1], "--meth-pat") && (argc == 2 || strcmp(argv[argc - 2], "--meth-pat"))) {
    fprintf(stderr, "%s: --meth-pat takes the path of the pattern table to write\n", argv[0]);
    return 2;
  }
  const char *frags_path = NULL; /* --meth-frags out.tsv: the per-region fragment methylation summary */
  bsc_frag_params frpar;
  bsc_frag_params_default(&frpar);
  int frag_opts = 0;
  if (argc >= 2 && !strcmp(argv[argc - 1], "--meth-frags") && (argc == 2 || strcmp(argv[argc - 2], "--meth-frags"))) {
    fprintf(stderr, "%s: --meth-frags takes the path of the fragment summary to write\n", argv[0]);
    return 2;
  }
  const char *mbias_path = NULL; /* --mbias out.tsv: the M-bias table */
  bsc_mbias_params mbpar;
  bsc_mbias_params_default(&mbpar);
  int mbias_opts = 0;
  if (argc >= 2 && !strcmp(argv[argc - 1], "--mbias") && (argc == 2 || strcmp(argv[argc - 2], "--mbias"))) {
    fprintf(stderr, "%s: --mbias takes the path of the M-bias table to write\n", argv[0]);
    return 2;
  }
  if (argc >= 2 && !strcmp(argv[argc - 1], "--meth-asm") && (argc == 2 || strcmp(argv[argc - 2], "--meth-asm"))) {
    fprintf(stderr, "%s: --meth-asm takes the path of the allele-specific methylation table to write\n", argv[0]);
    return 2;
  }
  if (argc >= 2 && !strcmp(argv[argc - 1], "--meth-reads") && (argc == 2 || strcmp(argv[argc - 2], "--meth-reads"))) {
    fprintf(stderr, "%s: --meth-reads takes the path of the read-level CpG table to write\n", argv[0]);
    return 2;
  }
  if (argc >= 2 && !strcmp(argv[argc - 1], "--meth") && (argc == 2 || strcmp(argv[argc - 2], "--meth"))) {
    fprintf(stderr, "%s: --meth takes the path of the methylation table to write (bedMethyl)\n", argv[0]);
    return 2;
  }
  if (argc >= 2 && !strcmp(argv[argc - 1], "--variants") && (argc == 2 || strcmp(argv[argc - 2], "--variants"))) {
    fprintf(stderr, "%s: --variants takes the path of the variant-only file to write\n", argv[0]);
    return 2;
  }
  if (argc == 2 && !strcmp(argv[1], "-D")) {
    fprintf(stderr, "%s: -D takes the path of a dbSNP index (the file dbSNP_idx writes)\n", argv[0]);
    return 2;
  }
  while (argc > 2 && argv[1][0] == '-' && (argv[1][1] == '-' || argv[1][1] == 'O' || argv[1][1] == 'D')) { /* --rank r --world n | --merge n | -O u|b | -D index */
    if (argv[1][1] == 'D') { /* -D index, -Dindex */
      dbsnp_path = argv[1][2] ? argv[1] + 2 : argv[2];
      const int k = argv[1][2] ? 1 : 2;
      argv[k] = argv[0];
      argv += k;
      argc -= k;
      continue;
    }
    if (argv[1][1] == 'O') { /* -O b, -Ob */
      const char *v = argv[1][2] ? argv[1] + 2 : argv[2];
      if (strcmp(v, "b") && strcmp(v, "u")) {
        fprintf(stderr, "%s: -O takes b (compressed BCF) or u (uncompressed BCF), not '%s'\n", argv[0], v);
        return 2;
      }
      bgzf = v[0] == 'b';
      const int k = argv[1][2] ? 1 : 2;
      argv[k] = argv[0];
      argv += k;
      argc -= k;
      continue;
    }
    if (!strcmp(argv[1], "--meth-asm-pass")) { /* no value */
      aspar.pass_only = 1;
      asm_opts = 1;
      argv[1] = argv[0];
      argv += 1;
      argc -= 1;
      continue;
    }
    if (!strcmp(argv[1], "--variants-pass") || !strcmp(argv[1], "--variants-known")) { /* no value */
      if (argv[1][11] == 'p') vpar.pass_only = 1;
      else vpar.known_only = 1;
      variants_opts = 1;
      argv[1] = argv[0];
      argv += 1;
      argc -= 1;
      continue;
    }
    if (!strcmp(argv[1], "--meth-bigbed-compress") || !strcmp(argv[1], "--meth-bgzf")) { /* no value */
      if (argv[1][8] == 'g') meth_bgzf = 1;
      else bigbed_z = 1;
      argv[1] = argv[0];
      argv += 1;
      argc -= 1;
      continue;
    }
    if (!strcmp(argv[1], "--index") || !strcmp(argv[1], "--meth-all") || !strcmp(argv[1], "--meth-pass") || !strcmp(argv[1], "--meth-merge") ||
        !strcmp(argv[1], "--meth-bigwig-compress")) { /* no value */
      if (argv[1][2] == 'i') index = 1;
      else if (argv[1][7] == 'b') bigwig_z = 1;
      else if (argv[1][7] == 'm') meth_merge = 1;
      else if (argv[1][7] == 'a') mpar.contexts = BSC_METH_ALL;
      else mpar.pass_only = 1;
      argv[1] = argv[0];
      argv += 1;
      argc -= 1;
      continue;
    }
    if (!strcmp(argv[1], "--rank")) rank = atoi(argv[2]);
    else if (!strcmp(argv[1], "--world")) world = atoi(argv[2]);
    else if (!strcmp(argv[1], "--merge")) merge = atoi(argv[2]);
    else if (!strcmp(argv[1], "--meth")) meth_path = argv[2];
    else if (!strcmp(argv[1], "--variants")) variants_path = argv[2];
    else if (!strcmp(argv[1], "--variants-min-qual")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v > 0xfffffffful) {
        fprintf(stderr, "%s: %s takes a count, not '%s'\n", argv[0], argv[1], argv[2]);
        return 2;
      }
      vpar.min_phred = (uint32_t)v;
      variants_opts = 1;
    }
    else if (!strcmp(argv[1], "--meth-reads")) reads_path = argv[2];
    else if (!strcmp(argv[1], "--meth-reads-min-sites") || !strcmp(argv[1], "--meth-reads-min-cov")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      const int sites = argv[1][17] == 's';
      if (!argv[2][0] || *end || argv[2][0] == '-' || v > 0xfffffffful || (sites && !v)) {
        fprintf(stderr, "%s: %s takes a count%s, not '%s'\n", argv[0], argv[1], sites ? ", 1 or more" : "", argv[2]);
        return 2;
      }
      if (sites) crpar.min_sites = (uint32_t)v;
      else crpar.min_cov = (uint32_t)v;
      reads_opts = 1;
    }
    else if (!strcmp(argv[1], "--meth-asm")) asm_path = argv[2];
    else if (!strcmp(argv[1], "--mbias")) mbias_path = argv[2];
    else if (!strcmp(argv[1], "--mbias-cycles")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v < 1 || v > BSC_MBIAS_MAX_CYCLES) {
        fprintf(stderr, "%s: --mbias-cycles takes a count, 1 .. %u, not '%s'\n", argv[0], BSC_MBIAS_MAX_CYCLES, argv[2]);
        return 2;
      }
      mbpar.n_cycles = (uint32_t)v;
      mbias_opts = 1;
    }
    else if (!strcmp(argv[1], "--meth-pat")) pat_path = argv[2];
    else if (!strcmp(argv[1], "--meth-pat-min-sites")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v > 0xfffffffful) {
        fprintf(stderr, "%s: %s takes a count, not '%s'\n", argv[0], argv[1], argv[2]);
        return 2;
      }
      ptpar.min_sites = (uint32_t)v;
      pat_opts = 1;
    }
    else if (!strcmp(argv[1], "--meth-frags")) frags_path = argv[2];
    else if (!strcmp(argv[1], "--meth-frags-min-sites") || !strcmp(argv[1], "--meth-frags-u-max") || !strcmp(argv[1], "--meth-frags-m-min")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v > 0xfffffffful) {
        fprintf(stderr, "%s: %s takes a count, not '%s'\n", argv[0], argv[1], argv[2]);
        return 2;
      }
      if (!strcmp(argv[1], "--meth-frags-min-sites")) frpar.min_sites = (uint32_t)v;
      else if (!strcmp(argv[1], "--meth-frags-u-max")) frpar.u_max_pct = (uint32_t)v;
      else frpar.m_min_pct = (uint32_t)v;
      frag_opts = 1;
    }
    else if (!strcmp(argv[1], "--meth-epialleles")) epi_path = argv[2];
    else if (!strcmp(argv[1], "--meth-epialleles-min-cov")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v > 0xfffffffful) {
        fprintf(stderr, "%s: %s takes a count, not '%s'\n", argv[0], argv[1], argv[2]);
        return 2;
      }
      eppar.min_cov = (uint32_t)v;
      epi_opts = 1;
    }
    else if (!strcmp(argv[1], "--meth-asm-window") || !strcmp(argv[1], "--meth-asm-min-qual") || !strcmp(argv[1], "--meth-asm-min-cov")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      const int window = argv[1][11] == 'w', qual = argv[1][15] == 'q';
      if (!argv[2][0] || *end || argv[2][0] == '-' || v > 0xfffffffful || (window && (v < 1 || v > 65535))) {
        fprintf(stderr, "%s: %s takes a count%s, not '%s'\n", argv[0], argv[1], window ? ", 1 .. 65535" : "", argv[2]);
        return 2;
      }
      if (window) aspar.max_dist = (uint32_t)v;
      else if (qual) aspar.min_phred = (uint32_t)v;
      else aspar.min_cov = (uint32_t)v;
      asm_opts = 1;
    }
    else if (!strcmp(argv[1], "--meth-index")) {
      if (strcmp(argv[2], "tbi") && strcmp(argv[2], "csi")) {
        fprintf(stderr, "%s: --meth-index takes tbi or csi, not '%s'\n", argv[0], argv[2]);
        return 2;
      }
      meth_index = argv[2];
    }
    else if (!strcmp(argv[1], "--meth-regions")) regions_path = argv[2];
    else if (!strcmp(argv[1], "--meth-regions-out")) regions_out_path = argv[2];
    else if (!strcmp(argv[1], "--meth-window")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v < 1 || v > 0xfffffffful) {
        fprintf(stderr, "%s: --meth-window takes a count of bases, 1 or more, not '%s'\n", argv[0], argv[2]);
        return 2;
      }
      meth_window = (uint32_t)v;
    }
    else if (!strcmp(argv[1], "--meth-bigwig")) bigwig_path = argv[2];
    else if (!strcmp(argv[1], "--cov-bigwig")) cov_path = argv[2];
    else if (!strcmp(argv[1], "--meth-bigbed")) bigbed_path = argv[2];
    else if (!strcmp(argv[1], "--meth-bigbed-items") || !strcmp(argv[1], "--meth-bigbed-zoom")) {
      char *end = NULL;
      const int items = argv[1][14] == 'i';
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v < 1 || v > (items ? 65535ul : 0xfffffffful)) {
        fprintf(stderr, "%s: %s takes a count of %s, not '%s'\n", argv[0], argv[1], items ? "sites, 1 .. 65535" : "bases, 1 or more", argv[2]);
        return 2;
      }
      if (items) bbpar.items_per_block = (uint32_t)v;
      else bbpar.reduction = (uint32_t)v;
    }
    else if (!strcmp(argv[1], "--meth-bigwig-section") || !strcmp(argv[1], "--meth-bigwig-zoom")) {
      char *end = NULL;
      const int sec = argv[1][14] == 's';
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v < 1 || v > (sec ? 65535ul : 0xfffffffful)) {
        fprintf(stderr, "%s: %s takes a count of %s, not '%s'\n", argv[0], argv[1], sec ? "sites, 1 .. 65535" : "bases, 1 or more", argv[2]);
        return 2;
      }
      if (sec) bwpar.items_per_section = (uint32_t)v;
      else bwpar.reduction = (uint32_t)v;
    }
    else if (!strcmp(argv[1], "--meth-min-cov") || !strcmp(argv[1], "--meth-min-gq")) {
      char *end = NULL;
      const unsigned long v = strtoul(argv[2], &end, 10);
      if (!argv[2][0] || *end || argv[2][0] == '-' || v > 0xfffffffful) {
        fprintf(stderr, "%s: %s takes a count, not '%s'\n", argv[0], argv[1], argv[2]);
        return 2;
      }
      if (argv[1][11] == 'c') mpar.min_cov = (uint32_t)v;
      else mpar.min_phred = (uint32_t)v;
    }
    else if (!strcmp(argv[1], "--format")) { /* bcf: BCF2 records (the default).  vcf: text lines, encoded on the device as well */
      if (strcmp(argv[2], "bcf") && strcmp(argv[2], "vcf")) {
        fprintf(stderr, "%s: --format takes bcf or vcf, not '%s'\n", argv[0], argv[2]);
        return 2;
      }
      text = argv[2][0] == 'v';
    }
    else break;
    argv[2] = argv[0];
    argv += 2;
    argc -= 2;
  }
  if (argc < 5 || world < 1 || (rank >= 0 && rank >= world)) {
    fprintf(stderr, "usage: %s [-O u|b] [--format bcf|vcf] [--index] [-D dbsnp.idx] [--meth out.bed [--meth-bgzf] [--meth-index tbi|csi] [--meth-merge | --meth-all] [--meth-min-cov n] [--meth-min-gq n] [--meth-pass]] [--meth-regions regions.bed | --meth-window n --meth-regions-out out.tsv] [--meth-bigwig out.bw [--meth-bigwig-section n] [--meth-bigwig-zoom n] [--meth-bigwig-compress: zlib sections, n <= 8157]: the methylation level as a bigWig track, per cytosine even with --meth-merge, under the --meth-* thresholds and --meth-all] [--cov-bigwig cov.bw: the depth of the same sites as a bigWig track, under the same --meth-bigwig-* switches] [--meth-bigbed out.bb [--meth-bigbed-items n] [--meth-bigbed-zoom n] [--meth-bigbed-compress: zlib blocks, n <= 652]] [--variants out: the records with an ALT allele, in the run's format and compression, with out.csi under --index [--variants-min-qual n] [--variants-pass] [--variants-known: dbSNP sites only, with -D]] [--meth-reads out.tsv: the read-level CpG concordance table, a line per reference CpG [--meth-reads-min-sites n] [--meth-reads-min-cov n]] [--mbias out.tsv: methylation by read cycle, from the reads as sequenced [--mbias-cycles n]] [--meth-asm out.tsv: the allele-specific methylation table, a line per heterozygous SNP and CpG near it [--meth-asm-window n] [--meth-asm-min-qual n] [--meth-asm-min-cov n] [--meth-asm-pass]] [--meth-epialleles out.tsv: the epiallele table, a line per window of four reference CpGs [--meth-epialleles-min-cov n]] [--meth-frags out.tsv: fragments per interval of --meth-regions / --meth-window by class U / X / M [--meth-frags-min-sites n] [--meth-frags-u-max pct] [--meth-frags-m-min pct]] [--meth-pat out.pat: the per-read CpG pattern table (PAT: chrom index pattern count, wgbstools-unpinned bytes, the index per contig, 64 CpGs a line at the most) [--meth-pat-min-sites n]] [--rank r --world n | --merge n] in.bam ref.fa out.bcf report.json [sample]\n", argv[0]);
    return 2;
  }
  if (text && (rank >= 0 || merge > 0)) {
    fprintf(stderr, "%s: --format vcf writes a single run's file; a sharded run (--rank / --merge) writes BCF\n", argv[0]);
    return 2;
  }
  if (text && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --format vcf is the device encoder's text: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (bgzf && (rank >= 0 || merge > 0)) {
    fprintf(stderr, "%s: -O b writes a single run's file; a sharded run (--rank / --merge) writes uncompressed BCF (-O u)\n", argv[0]);
    return 2;
  }
  if (index && (!bgzf || rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --index indexes a single run's compressed file: it needs -O b and no --rank / --world / --merge\n", argv[0]);
    return 2;
  }
  if (index && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --index scans the device encoder's streams: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (dbsnp_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: -D is a single run's option; a sharded run (--rank / --world / --merge) has no dbSNP index\n", argv[0]);
    return 2;
  }
  if (dbsnp_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: -D keeps the index on the device, for the device reader's blocks: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (meth_merge && !meth_path) {
    fprintf(stderr, "%s: --meth-merge combines the strands of the table --meth writes: it needs --meth out.bed\n", argv[0]);
    return 2;
  }
  if (meth_merge && mpar.contexts == BSC_METH_ALL) {
    fprintf(stderr, "%s: --meth-merge with --meth-all: only a CpG has a partner strand to combine with\n", argv[0]);
    return 2;
  }
  if (meth_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth writes a single run's table; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (meth_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth encodes what the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (reads_opts && !reads_path) {
    fprintf(stderr, "%s: --meth-reads-min-sites / --meth-reads-min-cov are thresholds of the table --meth-reads writes: they need --meth-reads out.tsv\n", argv[0]);
    return 2;
  }
  if (reads_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-reads writes a single run's table; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (reads_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-reads walks the prepared reads the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (mbias_opts && !mbias_path) {
    fprintf(stderr, "%s: --mbias-cycles sizes the table --mbias writes: it needs --mbias out.tsv\n", argv[0]);
    return 2;
  }
  if (mbias_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --mbias writes a single run's table; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (mbias_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --mbias walks the raw blocks the device reader leaves on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (epi_opts && !epi_path) {
    fprintf(stderr, "%s: --meth-epialleles-min-cov is a threshold of the table --meth-epialleles writes: it needs --meth-epialleles out.tsv\n", argv[0]);
    return 2;
  }
  if (epi_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-epialleles writes a single run's table; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (epi_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-epialleles walks the prepared reads the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (pat_opts && !pat_path) {
    fprintf(stderr, "%s: --meth-pat-min-sites is a threshold of the table --meth-pat writes: it needs --meth-pat out.pat\n", argv[0]);
    return 2;
  }
  if (pat_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-pat writes a single run's table; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (pat_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-pat walks the prepared reads the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (asm_opts && !asm_path) {
    fprintf(stderr, "%s: --meth-asm-window / --meth-asm-min-qual / --meth-asm-min-cov / --meth-asm-pass are thresholds of the table --meth-asm writes: they need --meth-asm out.tsv\n", argv[0]);
    return 2;
  }
  if (asm_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-asm writes a single run's table; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (asm_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-asm reads the records and the prepared reads the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (variants_opts && !variants_path) {
    fprintf(stderr, "%s: --variants-min-qual / --variants-pass / --variants-known select among the records --variants writes: they need --variants out\n", argv[0]);
    return 2;
  }
  if (variants_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --variants writes a single run's file; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (variants_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --variants selects from what the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (meth_bgzf && !meth_path && !reads_path && !asm_path && !epi_path && !pat_path) {
    fprintf(stderr, "%s: --meth-bgzf compresses the table --meth writes: it needs --meth out.bed.gz (or --meth-reads out.tsv.gz, whose table it compresses too)\n", argv[0]);
    return 2;
  }
  if (meth_index && !meth_path) {
    fprintf(stderr, "%s: --meth-index indexes the table --meth writes: it needs --meth out.bed.gz\n", argv[0]);
    return 2;
  }
  if (meth_index && !bgzf && !meth_bgzf) {
    fprintf(stderr, "%s: --meth-index indexes a compressed table: it needs -O b or --meth-bgzf\n", argv[0]);
    return 2;
  }
  if (regions_path && meth_window) {
    fprintf(stderr, "%s: --meth-regions and --meth-window exclude each other: the regions are the BED file's or the fixed tiles\n", argv[0]);
    return 2;
  }
  if ((regions_path || meth_window) && !regions_out_path && !frags_path) {
    fprintf(stderr, "%s: --meth-regions / --meth-window need --meth-regions-out out.tsv, the summary to write\n", argv[0]);
    return 2;
  }
  if (frag_opts && !frags_path) {
    fprintf(stderr, "%s: --meth-frags-min-sites / -u-max / -m-min are thresholds of the summary --meth-frags writes: they need --meth-frags out.tsv\n", argv[0]);
    return 2;
  }
  if (frags_path && !regions_path && !meth_window) {
    fprintf(stderr, "%s: --meth-frags sums over the intervals of --meth-regions regions.bed or --meth-window n: it needs one of them\n", argv[0]);
    return 2;
  }
  if (frags_path && (frpar.min_sites == 0 || frpar.u_max_pct > 100 || frpar.m_min_pct > 100 || frpar.u_max_pct >= frpar.m_min_pct)) {
    fprintf(stderr, "%s: --meth-frags: min-sites is 1 at least, the percentages 100 at the most and u-max below m-min (got %u, %u, %u)\n", argv[0],
            frpar.min_sites, frpar.u_max_pct, frpar.m_min_pct);
    return 2;
  }
  if (frags_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-frags sums a single run's blocks; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (frags_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-frags walks the prepared reads the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (regions_out_path && !regions_path && !meth_window) {
    fprintf(stderr, "%s: --meth-regions-out needs --meth-regions regions.bed or --meth-window n\n", argv[0]);
    return 2;
  }
  if (regions_out_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-regions sums a single run's blocks; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (regions_out_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-regions sums what the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (bigbed_z && !bigbed_path) {
    fprintf(stderr, "%s: --meth-bigbed-compress needs --meth-bigbed\n", argv[0]);
    return 2;
  }
  if (bigbed_z && bbpar.items_per_block > BSC_BB_Z_ITEMS_MAX) {
    fprintf(stderr, "%s: --meth-bigbed-compress: a block of %u sites may be more than 0xFF00 bytes (--meth-bigbed-items %u at the most)\n", argv[0],
            bbpar.items_per_block, BSC_BB_Z_ITEMS_MAX);
    return 2;
  }
  if (bigbed_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-bigbed writes a single run's file; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (bigbed_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-bigbed encodes what the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (bigwig_z && !bigwig_path && !cov_path) {
    fprintf(stderr, "%s: --meth-bigwig-compress needs --meth-bigwig\n", argv[0]);
    return 2;
  }
  if (bigwig_z && bwpar.items_per_section > 8157u) {
    fprintf(stderr, "%s: --meth-bigwig-compress: a section of %u sites is more than 0xFF00 bytes (--meth-bigwig-section 8157 at the most)\n", argv[0],
            bwpar.items_per_section);
    return 2;
  }
  if (bigwig_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --meth-bigwig writes a single run's track; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (bigwig_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --meth-bigwig reduces what the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  if (cov_path && (rank >= 0 || world > 1 || merge > 0)) {
    fprintf(stderr, "%s: --cov-bigwig writes a single run's track; a sharded run (--rank / --world / --merge) has none\n", argv[0]);
    return 2;
  }
  if (cov_path && (getenv("BAM2BCF_HOST_PREP") || getenv("BAM2BCF_HOST_BCF") || getenv("BAM2BCF_HOST_READER"))) {
    fprintf(stderr, "%s: --cov-bigwig reduces what the device reader's blocks leave on the device: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n", argv[0]);
    return 2;
  }
  const char *sample = argc > 5 ? argv[5] : "SAMPLE";
  if (merge > 0) return merge_main(merge, argv, sample);
  bsc_meth_bed *rbed = NULL; /* (before the context: a bad BED file costs no device) */
  if (regions_path) {
    FILE *bf = fopen(regions_path, "rb");
    if (!bf) {
      perror(regions_path);
      return 1;
    }
    char *bt = NULL;
    size_t bn = 0, bcap = 0;
    for (;;) {
      if (bn + 65536 > bcap) bt = xrealloc(bt, bcap = bcap ? bcap * 2 : (size_t)1 << 20);
      const size_t got = fread(bt + bn, 1, bcap - bn, bf);
      if (!got) break;
      bn += got;
    }
    fclose(bf);
    if (bsc_meth_regions_parse_bed(bt, bn, &rbed) < 0) {
      fprintf(stderr, "%s: %s\n", regions_path, bsc_last_error());
      return 1;
    }
    free(bt);
  }
  const int sharded = rank >= 0;
  const int host_prep = getenv("BAM2BCF_HOST_PREP") != NULL;
  const int host_bcf = host_prep || getenv("BAM2BCF_HOST_BCF") != NULL;
  const int host_reader = host_bcf || getenv("BAM2BCF_HOST_READER") != NULL;
  if (sharded && host_reader) {
    fprintf(stderr, "bam2bcf: a sharded run reads through the device reader (its contig selection)\n");
    return 2;
  }
  if (bgzf && host_reader) {
    fprintf(stderr, "bam2bcf: -O b compresses the device encoder's streams: not with BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP\n");
    return 2;
  }
  if (dbsnp_path) CHECK(bsc_dbsnp_open(dbsnp_path, &g_dbsnp)); /* (before the context: a bad index costs no device) */
  const double t_start = now();
  bsc_params prm = {0.01, 0.05, 2.0, 20, 0};
  bsc_context *ctx;
  CHECK(bsc_create(&prm, &ctx));
  const double t_ctx = now() - t_start;
  bsc_bam *bam = NULL;
  bsc_bamdev *dev = NULL;
  if (host_reader) CHECK(bsc_bam_open_threads(argv[1], getenv("BAM2BCF_THREADS") ? atoi(getenv("BAM2BCF_THREADS")) : 4, &bam)); /* BGZF inflate ahead of the parser */
  else if (!sharded) CHECK(bsc_bamdev_open(ctx, argv[1], getenv("BAM2BCF_THREADS") ? atoi(getenv("BAM2BCF_THREADS")) : 0, &dev));
  else { /* this rank's contigs: the stretches of the file that hold them */
    int nr_, *owner;
    const char **nm_;
    uint32_t *ln_;
    bsc_bamstream *hs_;
    header_of(argv[1], &nr_, &nm_, &ln_, &hs_);
    owner = assign_contigs(ln_, nr_, world);
    int32_t *mine = calloc((size_t)nr_ + 2, sizeof *mine);
    uint32_t n_mine = 0;
    for (int i = 0; i < nr_; i++)
      if (owner[i] == rank) mine[n_mine++] = i;
    if (nr_ && owner[nr_ - 1] == rank) mine[n_mine++] = -1; /* the unplaced reads at the file's end go with the last contig's rank */
    CHECK(bsc_bamdev_open_contigs(ctx, argv[1], getenv("BAM2BCF_THREADS") ? atoi(getenv("BAM2BCF_THREADS")) : 0, mine, n_mine, &dev));
    free(mine);
    free(owner);
    free(nm_);
    free(ln_);
    bsc_bamstream_close(hs_);
  }
#define N_REFS() (host_reader ? bsc_bam_n_refs(bam) : bsc_bamdev_n_refs(dev))
#define REF_NAME(i) (host_reader ? bsc_bam_ref_name(bam, (i)) : bsc_bamdev_ref_name(dev, (i)))
#define REF_LEN(i) (host_reader ? bsc_bam_ref_len(bam, (i)) : bsc_bamdev_ref_len(dev, (i)))
  FILE *out = sharded ? NULL : fopen(argv[3], "wb");
  if (!out && !sharded) {
    perror(argv[3]);
    return 1;
  }
  const int n_ref = N_REFS();
  /* the per-region summary: which of the BED's contigs is which of the header's, the file, and the contig whose regions are attached */
  FILE *rout = NULL;
  int64_t *rbed_of = NULL; /* per tid: the BED's contig, or -1 */
  bsc_meth_region *rwin = NULL; /* --meth-window: the current contig's tiles */
  uint64_t r_n = 0, region_lines = 0;
  const bsc_meth_region *r_regs = NULL;
  const char *const *r_names = NULL;
  FILE *fout = NULL; /* --meth-frags: the fragment summary over the same intervals, attached, read and appended where the region summary is */
  uint64_t frag_lines = 0, frag_tot[BSC_FRAG_N_TOTALS] = {0};
  if (frags_path) {
    fout = fopen(frags_path, "wb");
    if (!fout) {
      perror(frags_path);
      return 1;
    }
  }
  if (regions_out_path || frags_path) {
    if (regions_out_path) {
      rout = fopen(regions_out_path, "wb");
      if (!rout) {
        perror(regions_out_path);
        return 1;
      }
    }
    if (rbed) {
      rbed_of = xrealloc(NULL, ((size_t)n_ref + 1) * sizeof *rbed_of);
      for (int i = 0; i < n_ref; i++) rbed_of[i] = -1;
      uint64_t skipped = 0;
      uint32_t skipped_contigs = 0;
      for (uint32_t c = 0; c < rbed->n_contigs; c++) {
        int t = 0;
        while (t < n_ref && strcmp(REF_NAME(t), rbed->contigs[c])) t++;
        if (t < n_ref) rbed_of[t] = c;
        else {
          skipped += rbed->first[c + 1] - rbed->first[c];
          skipped_contigs++;
        }
      }
      if (skipped)
        fprintf(stderr, "bam2bcf: %llu regions on %u contigs the BAM header does not name were skipped\n", (unsigned long long)skipped, skipped_contigs);
    }
  }
  int meth_fd = -1;
  uint64_t meth_at = 0, meth_lines = 0;
  bsc_bgzf *zm = NULL;
  if (meth_path) {
    FILE *mf = fopen(meth_path, "wb");
    if (!mf) {
      perror(meth_path);
      return 1;
    }
    meth_fd = dup(fileno(mf));
    fclose(mf);
    if (bgzf || meth_bgzf) CHECK(bsc_bgzf_open(ctx, &zm));
  }
  int reads_fd = -1; /* --meth-reads: the file, where its next bytes go, its compressor, the sums of the blocks' totals and lines */
  uint64_t reads_at = 0, reads_lines = 0, reads_tot[BSC_CPG_READS_N_TOTALS] = {0};
  bsc_bgzf *zr = NULL;
  if (reads_path) {
    FILE *rf = fopen(reads_path, "wb");
    if (!rf) {
      perror(reads_path);
      return 1;
    }
    reads_fd = dup(fileno(rf));
    fclose(rf);
    if (bgzf || meth_bgzf) CHECK(bsc_bgzf_open(ctx, &zr));
  }
  int asm_fd = -1; /* --meth-asm: the file, where its next bytes go, its compressor, the sums of the blocks' totals and lines */
  uint64_t asm_at = 0, asm_lines = 0, asm_tot[BSC_ASM_N_TOTALS] = {0};
  bsc_bgzf *za = NULL;
  int epi_fd = -1; /* --meth-epialleles: the file, where its next bytes go, its compressor, the sums of the blocks' totals and lines */
  uint64_t epi_at = 0, epi_lines = 0, epi_tot[BSC_EPI_N_TOTALS] = {0};
  bsc_bgzf *ze = NULL;
  int pat_fd = -1; /* --meth-pat: the file, where its next bytes go, its compressor, the sums of the blocks' totals and lines; the sites of the
                    * contig in front of position pat_from */
  uint64_t pat_at = 0, pat_lines = 0, pat_tot[BSC_PAT_N_TOTALS] = {0}, pat_base = 0, pat_from = 1;
  uint64_t pat_room16 = 8 * 16; /* the table's room, sixteenths of a byte a position: 8 bytes at first (30x paired WGBS measured about 5), then a
                                 * quarter more than the last block needed, so that a block is walked, sorted and encoded once */
  bsc_bgzf *zp = NULL;
  FILE *mbias_f = NULL; /* --mbias: opened now, so that a path that cannot be written stops the run before it starts; written at the end */
  uint64_t mbias_tot[BSC_MBIAS_N_TOTALS] = {0};
  int mbias_any = 0;
  if (mbias_path && !(mbias_f = fopen(mbias_path, "wb"))) {
    perror(mbias_path);
    return 1;
  }
  if (asm_path) {
    FILE *af = fopen(asm_path, "wb");
    if (!af) {
      perror(asm_path);
      return 1;
    }
    asm_fd = dup(fileno(af));
    fclose(af);
    const size_t al = strlen(asm_path);
    if (bgzf || meth_bgzf || (al > 3 && !strcmp(asm_path + al - 3, ".gz"))) CHECK(bsc_bgzf_open(ctx, &za));
  }
  if (epi_path) {
    FILE *ef = fopen(epi_path, "wb");
    if (!ef) {
      perror(epi_path);
      return 1;
    }
    epi_fd = dup(fileno(ef));
    fclose(ef);
    const size_t el = strlen(epi_path);
    if (bgzf || meth_bgzf || (el > 3 && !strcmp(epi_path + el - 3, ".gz"))) CHECK(bsc_bgzf_open(ctx, &ze));
  }
  if (pat_path) {
    FILE *pf = fopen(pat_path, "wb");
    if (!pf) {
      perror(pat_path);
      return 1;
    }
    pat_fd = dup(fileno(pf));
    fclose(pf);
    const size_t pl = strlen(pat_path);
    if (bgzf || meth_bgzf || (pl > 3 && !strcmp(pat_path + pl - 3, ".gz"))) CHECK(bsc_bgzf_open(ctx, &zp));
  }
  int var_fd = -1; /* --variants: the file, where its next bytes go, its compressor and index, the sums of the blocks' totals */
  uint64_t var_at = 0, var_tot[BSC_VAR_N_TOTALS] = {0};
  bsc_bgzf *zv = NULL;
  bsc_csi *vcsi = NULL;
  bsc_tbx *tbx = NULL;
  bsc_bgzf *zw = NULL;
  bsc_csi *csi = NULL;
  int bw_fd = -1;
  bsc_bigwig *bw = NULL;
  uint64_t bw_sites = 0;
  int cw_fd = -1; /* --cov-bigwig: the coverage track's file and writer */
  bsc_bigwig *cw = NULL;
  uint64_t cw_sites = 0;
  int bb_fd = -1;
  bsc_bigbed *bb = NULL;
  uint64_t bb_sites = 0;
  if (!sharded) {
    const char **names = calloc((size_t)n_ref + 1, sizeof *names);
    uint32_t *lens = calloc((size_t)n_ref + 1, sizeof *lens);
    for (int i = 0; i < n_ref; i++) {
      names[i] = REF_NAME(i);
      lens[i] = REF_LEN(i);
    }
    if (bigwig_path) { /* the track's file: the blocks' data go in as they come, the header and the indexes at the end (it keeps its own names) */
      FILE *bf = fopen(bigwig_path, "wb");
      if (!bf) {
        perror(bigwig_path);
        return 1;
      }
      bw_fd = dup(fileno(bf));
      fclose(bf);
      CHECK(bsc_bigwig_open(bw_fd, (uint32_t)n_ref, names, lens, &bwpar, &bw));
    }
    if (cov_path) { /* the coverage track's file, as the level track's */
      FILE *bf = fopen(cov_path, "wb");
      if (!bf) {
        perror(cov_path);
        return 1;
      }
      cw_fd = dup(fileno(bf));
      fclose(bf);
      CHECK(bsc_bigwig_open_track(cw_fd, (uint32_t)n_ref, names, lens, &bwpar, BSC_BW_COVERAGE, &cw));
    }
    if (bigbed_path) { /* the bigBed's file, as the track's */
      FILE *bf = fopen(bigbed_path, "wb");
      if (!bf) {
        perror(bigbed_path);
        return 1;
      }
      bb_fd = dup(fileno(bf));
      fclose(bf);
      CHECK(bsc_bigbed_open(bb_fd, (uint32_t)n_ref, names, lens, &bbpar, &bb));
    }
    if (meth_index) /* the table has no header: its index begins with the first block (it keeps its own copy of the names) */
      CHECK(bsc_tbx_open(zm, meth_index[0] == 't' ? BSC_TBX_TBI : BSC_TBX_CSI, 14, n_ref, names, lens, &tbx));
    if (variants_path) { /* the variant-only file: the main file's header, then a block's selected records as they come — its own compressor and
                          * its own index under -O b / --index, as the --meth table has */
      FILE *vf = fopen(variants_path, "wb");
      if (!vf) {
        perror(variants_path);
        return 1;
      }
      if (bgzf) {
        char *hb = NULL;
        size_t hn = 0;
        FILE *hm = open_memstream(&hb, &hn);
        if (!hm) {
          perror("open_memstream");
          return 1;
        }
        write_header(hm, n_ref, names, lens, sample, text);
        if (fclose(hm)) {
          perror("open_memstream");
          return 1;
        }
        CHECK(bsc_bgzf_open(ctx, &zv));
        CHECK(bsc_bgzf_write(zv, hb, hn));
        free(hb);
        if (index) CHECK(bsc_csi_open(zv, text ? BSC_CSI_VCF : BSC_CSI_BCF, 14, n_ref, names, lens, &vcsi));
      } else {
        write_header(vf, n_ref, names, lens, sample, text);
        fflush(vf);
        var_at = (uint64_t)ftello(vf);
      }
      var_fd = dup(fileno(vf));
      fclose(vf);
    }
    if (bgzf) { /* the header into the compressor: its members come out with the first block's */
      char *hb = NULL;
      size_t hn = 0;
      FILE *hm = open_memstream(&hb, &hn);
      if (!hm) {
        perror("open_memstream");
        return 1;
      }
      write_header(hm, n_ref, names, lens, sample, text);
      if (fclose(hm)) {
        perror("open_memstream");
        return 1;
      }
      CHECK(bsc_bgzf_open(ctx, &zw));
      CHECK(bsc_bgzf_write(zw, hb, hn));
      free(hb);
      if (index) CHECK(bsc_csi_open(zw, text ? BSC_CSI_VCF : BSC_CSI_BCF, 14, n_ref, names, lens, &csi)); /* (it keeps its own copy of the names) */
    } else write_header(out, n_ref, names, lens, sample, text);
    free(names);
    free(lens);
  }
  bsc_bcf_ids ids;
  bsc_bcf_default_ids(&ids);
  const bsc_reader_params rpar = {20, 1000, 0, 0, 0, 0, 0, 0}; /* defaults of the reference; no region */
  const bsc_prep_params ppar = {{0, 0}, {0, 0}, 20};

  bsc_contig_totals *ctot = calloc((size_t)n_ref + 1, sizeof *ctot);
  static uint64_t prof_counts[PROF_CAP][4];
  memset(prof_counts, 0, sizeof prof_counts);
  bsc_read_profile prof = {NULL, 0, 0, &prof_counts[0][0], 4096, 0};
  uint64_t base_filter[5] = {0, 0, 0, 0, 0}, passed_reads = 0, passed_bases = 0, before[14], after[14];
  CHECK(bsc_reset_site_stats(ctx));
  CHECK(bsc_get_site_totals(ctx, before));

  uint8_t *codes = NULL, *ref = NULL, *pseq = NULL, *bcf = NULL, *gc = NULL;
  bsc_template *tpl = NULL;
  bsc_vcf_rec *recs = NULL;
  uint64_t codes_len = 0;
  size_t cap_ref = 0, cap_pseq = 0, cap_tpl = 0, cap_recs = 0, cap_bcf = 0;
  int cur_tid = -1;
  uint64_t n_blocks = 0, n_records = 0;
  bsc_read_block blk;
  bsc_dev_read_block dblk;
  static out_writer W;
  static ref_job RJ;
  int out_fd = -1;
  uint64_t file_at = 0;
  if (n_ref > 0) ref_start(&RJ, argv[2], REF_NAME(0), REF_LEN(0), 0); /* the first contig's reference: while the helpers inflate */
  if (!host_reader) { /* the output pieces too: page-locking them takes its time */
    if (out) {
      fflush(out);
      file_at = (uint64_t)ftello(out);
      out_fd = fileno(out);
    } /* else a rank of a sharded run: a file per contig, opened when the contig begins */
    W.ctx = ctx;
    for (int k = 0; k < 2; k++) W.buf[k] = pinned(PIECE);
    pthread_mutex_init(&W.mu, NULL);
    pthread_cond_init(&W.cv, NULL);
    pthread_create(&W.th, NULL, writer_main, &W);
    W.started = 1;
  }
  int r;
  double t_read = 0, t_ref = 0, t_prep = 0, t_gpu = 0, t_enc = 0, t0 = now(), t1;
  for (;;) {
    if (host_reader) r = bsc_bam_next_block(bam, &rpar, &blk);
    else {
      r = bsc_bamdev_next_block(dev, &rpar, &dblk);
      blk.tid = dblk.tid; /* the loop below reads the block's contig, end and first position from blk / x */
      blk.y = dblk.y;
      blk.nr = dblk.nr;
    }
    t_read += (t1 = now()) - t0;
    t0 = t1;
    if (r != 1) break;
    if (blk.tid != cur_tid) { /* contig change: its sequence, and the finished contig's share of the totals */
      if (cur_tid >= 0) {
        CHECK(bsc_get_site_totals(ctx, after));
        uint64_t *d = ctot[cur_tid].snps; /* seven [all, passed] pairs, contiguous */
        for (int i = 0; i < 14; i++) d[i] += after[i] - before[i];
        memcpy(before, after, sizeof before);
      }
      if (rout && cur_tid >= 0) region_lines += regions_flush(ctx, rout, REF_NAME(cur_tid), r_regs, r_names, r_n);
      if (fout && cur_tid >= 0) frag_lines += frags_flush(ctx, fout, REF_NAME(cur_tid), r_regs, r_names, r_n);
      cur_tid = blk.tid;
      pat_base = 0; /* --meth-pat: the index counts the contig's CpGs */
      pat_from = 1;
      ctot[cur_tid].name = REF_NAME(cur_tid);
      if (sharded) { /* this contig's shard; the one before is closed by the output thread behind its last piece */
        if (out_fd >= 0) {
          const out_job cj = {NULL, 0, 0, out_fd, 1};
          writer_push(&W, cj);
        }
        char *sp = malloc(strlen(argv[3]) + 32);
        sprintf(sp, "%s.shard%05d", argv[3], cur_tid);
        FILE *sf = fopen(sp, "wb");
        if (!sf) {
          perror(sp);
          return 1;
        }
        out_fd = dup(fileno(sf));
        fclose(sf);
        free(sp);
        file_at = 0;
      }
      /* its sequence and GC bins (for the report's GC-by-coverage table: load_sequence computes them when a report is asked for): loaded in
       * the background since the previous contig began — or since the program did */
      if (!RJ.running || RJ.tid != cur_tid) {
        if (RJ.running) {
          pthread_join(RJ.th, NULL);
          free(RJ.codes);
          free(RJ.gc);
        }
        ref_start(&RJ, argv[2], REF_NAME(cur_tid), REF_LEN(cur_tid), cur_tid);
      }
      if (RJ.running) pthread_join(RJ.th, NULL);
      RJ.running = 0;
      if (RJ.rc < 0) {
        fprintf(stderr, "reference of %s: %s\n", REF_NAME(cur_tid), RJ.err);
        return 1;
      }
      free(codes);
      free(gc);
      codes = RJ.codes;
      gc = RJ.gc;
      codes_len = RJ.codes_len;
      CHECK(bsc_set_gc_bins_host(ctx, gc, (uint32_t)RJ.n_bins, RJ.gc_start));
      if (g_dbsnp) CHECK(bsc_dbsnp_attach(ctx, g_dbsnp, NULL)); /* what the job loaded behind the reference; the next job may load over it */
      if (rout || fout) { /* this contig's regions, their accumulators zeroed: the BED's, or the fixed tiles */
        r_n = 0;
        r_regs = NULL;
        r_names = NULL;
        if (meth_window) {
          const uint64_t len = REF_LEN(cur_tid);
          r_n = (len + meth_window - 1) / meth_window;
          rwin = xrealloc(rwin, (size_t)r_n * sizeof *rwin);
          for (uint64_t k = 0; k < r_n; k++) {
            rwin[k].start = (uint32_t)(k * meth_window);
            rwin[k].end = (uint32_t)((k + 1) * meth_window < len ? (k + 1) * meth_window : len);
          }
          r_regs = rwin;
        } else if (rbed_of[cur_tid] >= 0) {
          const uint64_t f0 = rbed->first[rbed_of[cur_tid]];
          r_n = rbed->first[rbed_of[cur_tid] + 1] - f0;
          r_regs = rbed->regions + f0;
          r_names = (const char *const *)rbed->names + f0;
        }
        if (rout) CHECK(bsc_meth_regions_attach(ctx, r_regs, r_n));
        if (fout) CHECK(bsc_frag_attach(ctx, r_regs, r_n));
      }
      if (cur_tid + 1 < n_ref) ref_start(&RJ, argv[2], REF_NAME(cur_tid + 1), REF_LEN(cur_tid + 1), cur_tid + 1); /* the next one, meanwhile */
    }
    const uint32_t x = host_reader ? bsc_block_start(&blk.tpl[0]) : dblk.x, y = blk.y, n = y - x + 1;
    if (n + 2 > cap_ref) ref = xrealloc(ref, cap_ref = (size_t)(n + 2) * 2);
    CHECK(bsc_block_reference(codes, codes_len, x, n + 2, ref));
    t_ref += (t1 = now()) - t0;
    t0 = t1;
    /* the process thread's per-template work and call_genotypes_ML in one call: the raw templates go up as the reader left them,
     * the device prepares them (trims, clips, mate overlap, indels; the read profile) and calls the block.  BAM2BCF_HOST_PREP in the
     * environment keeps round 4's split (bsc_prepare_templates_profile on this thread, then bsc_block_records) for comparison. */
    bsc_prep_stats st;
    const bsc_vcf_params vp = {0, 1, (uint32_t)codes_len};
    uint64_t n_out = 0, n_bytes = 0;
    if (!host_reader) { /* the block is in HBM already; its stream stays there too and comes over in pieces, the output thread writing behind */
      /* room for the kept stream: a BCF record is ~113 bytes, a text line ~143 (contig name included), about half the positions of WGBS data
       * write one; a denser block is encoded once more into the room it asks for (bsc_block_bcf_again) */
      uint64_t dev_cap = (uint64_t)n * (text ? 160 : 96) + 4096;
      int rc = text ? bsc_block_vcf_rawdev_keep(ctx, dblk.d_tpl, dblk.nr, dblk.d_seq, dblk.seq_bytes, dblk.d_misms, dblk.n_misms, dblk.ins_pad, &ppar, x, y, ref,
                                                NULL, &vp, 1, REF_NAME(dblk.tid), NULL, dev_cap, &n_bytes, &n_out, &st, &prof)
                    : bsc_block_bcf_rawdev_keep(ctx, dblk.d_tpl, dblk.nr, dblk.d_seq, dblk.seq_bytes, dblk.d_misms, dblk.n_misms, dblk.ins_pad, &ppar, x, y, ref,
                                                NULL, &vp, 1, dblk.tid, &ids, NULL, dev_cap, &n_bytes, &n_out, &st, &prof);
      if (rc == BSC_ERR_ARG && n_bytes > dev_cap) { /* a block of long records: the encoder alone once more, with the room it asks for */
        dev_cap = n_bytes + 4096;
        rc = bsc_block_bcf_again(ctx, NULL, dev_cap, &n_bytes, &n_out);
      }
      CHECK(rc);
      if (mbias_path) { /* the block's raw templates, still in the reader's buffers, into the run's M-bias accumulator */
        CHECK(bsc_block_mbias_rawdev(ctx, dblk.d_tpl, dblk.nr, dblk.d_seq, dblk.seq_bytes, dblk.d_misms, dblk.n_misms, &mbpar, mbias_tot));
        mbias_any = 1;
      }
      t_gpu += (t1 = now()) - t0;
      t0 = t1;
      if (n_bytes && csi) { /* the index's entries of this block, while the encoder's tile offsets are still the stream's: noted at the writer's
                             * logical length, before the stream goes in */
        const bsc_csi_entry *ce = NULL;
        uint64_t cn = 0;
        CHECK(bsc_block_csi_kept(ctx, 14, &ce, &cn, NULL));
        CHECK(bsc_csi_add(csi, dblk.tid, ce, cn, n_bytes));
      }
      if (n_bytes && r_n && rout) CHECK(bsc_block_meth_regions_kept(ctx, &mpar, NULL, NULL)); /* the block's cytosines into the attached regions' sums */
      if (n_bytes && r_n && fout) { /* the block's templates into the attached regions' fragment sums, from the prepared reads the call left on the device */
        uint64_t ft[BSC_FRAG_N_TOTALS];
        CHECK(bsc_block_frag_kept(ctx, &frpar, ft));
        for (int k = 0; k < BSC_FRAG_N_TOTALS; k++) frag_tot[k] += ft[k];
      }
      if (n_bytes && (bw || cw)) { /* the block's bigWig sections and summaries, from the same arrays: a host buffer and a job of its own per
                                    * track.  With --cov-bigwig ONE call reduces the block for every track asked for. */
        uint64_t b_raw = 0, b_sites = 0, b_sec = 0, b_zoom = 0;
        const bsc_bw_sum *sec[2] = {NULL, NULL}, *zoom[2] = {NULL, NULL};
        if (cw)
          CHECK(bsc_block_bigwig_tracks_kept(ctx, (uint32_t)dblk.tid, &mpar, &bwpar, (bw ? BSC_BW_LEVEL : 0u) | BSC_BW_COVERAGE, &b_raw, &b_sites, &b_sec,
                                             &b_zoom, bw ? &sec[0] : NULL, bw ? &zoom[0] : NULL, &sec[1], &zoom[1]));
        else
          CHECK(bsc_block_bigwig_kept(ctx, (uint32_t)dblk.tid, &mpar, &bwpar, &b_raw, &b_sites, &sec[0], &b_sec, &zoom[0], &b_zoom));
        if (bw) bw_sites += b_sites;
        if (cw) cw_sites += b_sites;
        for (int t = 0; t < 2 && b_sec; t++) {
          if (!(t ? cw : bw)) continue;
          uint64_t b_bytes = b_raw;
          out_job j;
          memset(&j, 0, sizeof j);
          j.fd = -1;
          j.n = b_bytes;
          j.bw = t ? cw : bw;
          j.bw_tid = (uint32_t)dblk.tid;
          if (bigwig_z) { /* the sections as zlib streams: the job carries those and their sizes */
            const uint32_t *zs = NULL;
            uint64_t z_bytes = 0, z_sec = 0;
            CHECK((t ? bsc_block_bigwig_cov_deflate : bsc_block_bigwig_deflate)(ctx, &z_bytes, &zs, &z_sec));
            if (z_sec != b_sec) {
              fprintf(stderr, "bam2bcf: %llu zlib streams for %llu bigWig sections\n", (unsigned long long)z_sec, (unsigned long long)b_sec);
              return 1;
            }
            j.n = b_bytes = z_bytes;
            j.bw_zsizes = xrealloc(NULL, (size_t)b_sec * sizeof *zs);
            memcpy(j.bw_zsizes, zs, (size_t)b_sec * sizeof *zs);
          }
          j.bw_data = xrealloc(NULL, (size_t)b_bytes);
          j.bw_sec = xrealloc(NULL, (size_t)b_sec * sizeof **sec);
          j.bw_zoom = xrealloc(NULL, (size_t)b_zoom * sizeof **zoom);
          j.bw_n_sec = b_sec;
          j.bw_n_zoom = b_zoom;
          memcpy(j.bw_sec, sec[t], (size_t)b_sec * sizeof **sec);
          memcpy(j.bw_zoom, zoom[t], (size_t)b_zoom * sizeof **zoom);
          CHECK((t ? (bigwig_z ? bsc_bigwig_cov_zstream_read : bsc_bigwig_cov_stream_read) : (bigwig_z ? bsc_bigwig_zstream_read : bsc_bigwig_stream_read))(
              ctx, 0, b_bytes, j.bw_data));
          CHECK(bsc_synchronize(ctx));
          writer_push(&W, j);
        }
      }
      if (n_bytes && bb) { /* the block's bigBed items and summaries, from the same arrays: a host buffer and a job of its own */
        uint64_t b_bytes = 0, b_sites = 0, b_blk = 0, b_zoom = 0;
        const bsc_bb_sum *blk = NULL, *zoom = NULL;
        CHECK(bsc_block_bigbed_kept(ctx, (uint32_t)dblk.tid, &mpar, &bbpar, &b_bytes, &b_sites, &blk, &b_blk, &zoom, &b_zoom));
        bb_sites += b_sites;
        if (b_blk) {
          out_job j;
          memset(&j, 0, sizeof j);
          j.fd = -1;
          j.n = j.bb_raw = b_bytes;
          j.bb = bb;
          j.bw_tid = (uint32_t)dblk.tid;
          j.bb_blk = xrealloc(NULL, (size_t)b_blk * sizeof *blk); /* copied before the next call: the host copies are good until then */
          j.bb_zoom = xrealloc(NULL, (size_t)b_zoom * sizeof *zoom);
          j.bb_n_blk = b_blk;
          j.bb_n_zoom = b_zoom;
          memcpy(j.bb_blk, blk, (size_t)b_blk * sizeof *blk);
          memcpy(j.bb_zoom, zoom, (size_t)b_zoom * sizeof *zoom);
          if (bigbed_z) { /* the blocks as zlib streams: the job carries those and their sizes */
            const uint32_t *zs = NULL;
            uint64_t z_bytes = 0, z_blk = 0;
            CHECK(bsc_block_bigbed_deflate(ctx, &z_bytes, &zs, &z_blk));
            if (z_blk != b_blk) {
              fprintf(stderr, "bam2bcf: %llu zlib streams for %llu bigBed blocks\n", (unsigned long long)z_blk, (unsigned long long)b_blk);
              return 1;
            }
            j.n = b_bytes = z_bytes;
            j.bb_zsizes = xrealloc(NULL, (size_t)b_blk * sizeof *zs);
            memcpy(j.bb_zsizes, zs, (size_t)b_blk * sizeof *zs);
          }
          j.bb_data = xrealloc(NULL, (size_t)b_bytes);
          CHECK((bigbed_z ? bsc_bigbed_zstream_read : bsc_bigbed_stream_read)(ctx, 0, b_bytes, j.bb_data));
          CHECK(bsc_synchronize(ctx));
          writer_push(&W, j);
        }
      }
      if (n_bytes && meth_path) { /* the block's methylation table, from the arrays the call left on the device: a buffer and a job of its own */
        uint64_t m_cap = (uint64_t)n * (mpar.contexts == BSC_METH_ALL ? 16 : 4) + 4096, m_bytes = 0, m_lines = 0;
        int (*const meth_kept)(bsc_context *, const char *, const bsc_meth_params *, uint64_t, uint64_t *, uint64_t *, uint64_t *) =
            meth_merge ? bsc_block_meth_cpg_kept : bsc_block_meth_kept;
        int mrc = meth_kept(ctx, REF_NAME(dblk.tid), &mpar, m_cap, &m_bytes, &m_lines, NULL);
        if (mrc == BSC_ERR_ARG && m_bytes > m_cap) mrc = meth_kept(ctx, REF_NAME(dblk.tid), &mpar, m_bytes, &m_bytes, &m_lines, NULL);
        CHECK(mrc);
        meth_lines += m_lines;
        if (m_bytes && tbx) { /* the index's entries of this block, while the encoder's tile offsets are still the table's: noted at the
                               * writer's logical length, before the table goes into the compressor */
          const bsc_bed_entry *be = NULL;
          uint64_t bn = 0;
          CHECK(bsc_block_meth_index_kept(ctx, 14, &be, &bn, NULL));
          CHECK(bsc_tbx_add(tbx, dblk.tid, be, bn, m_bytes));
        }
        if (m_bytes) {
          void *d_m = NULL;
          uint64_t n_m = 0;
          CHECK(bsc_meth_stream_detach(ctx, &d_m, &n_m));
          if (zm) {
            CHECK(bsc_bgzf_write_device(zm, d_m, n_m));
            CHECK(bsc_detached_free(ctx, d_m));
            d_m = NULL;
            n_m = 0;
            CHECK(bsc_bgzf_take(zm, &d_m, &n_m));
          }
          if (n_m) {
            const out_job j = {d_m, n_m, meth_at, meth_fd, 0};
            writer_push(&W, j);
          }
          meth_at += n_m;
        }
      }
      if (n_bytes && reads_path) { /* the block's read-level CpG table, from the prepared templates, reads and reference codes the call left on the
                                    * device: a buffer and a job of its own */
        uint64_t r_cap = (uint64_t)n * 2 + 4096, r_bytes = 0, r_lines = 0, rt[BSC_CPG_READS_N_TOTALS];
        int rrc = bsc_block_cpg_reads_kept(ctx, REF_NAME(dblk.tid), &crpar, r_cap, &r_bytes, &r_lines, rt);
        if (rrc == BSC_ERR_ARG && r_bytes > r_cap) rrc = bsc_block_cpg_reads_kept(ctx, REF_NAME(dblk.tid), &crpar, r_bytes, &r_bytes, &r_lines, rt);
        CHECK(rrc);
        reads_lines += r_lines;
        for (int k = 0; k < BSC_CPG_READS_N_TOTALS; k++) reads_tot[k] += rt[k];
        if (r_bytes) {
          void *d_r = NULL;
          uint64_t n_r = 0;
          CHECK(bsc_cpg_reads_stream_detach(ctx, &d_r, &n_r));
          if (zr) {
            CHECK(bsc_bgzf_write_device(zr, d_r, n_r));
            CHECK(bsc_detached_free(ctx, d_r));
            d_r = NULL;
            n_r = 0;
            CHECK(bsc_bgzf_take(zr, &d_r, &n_r));
          }
          if (n_r) {
            const out_job j = {d_r, n_r, reads_at, reads_fd, 0};
            writer_push(&W, j);
          }
          reads_at += n_r;
        }
      }
      if (n_bytes && asm_path) { /* the block's allele-specific methylation table, from the dense records and the prepared reads the call left on the
                                  * device: a buffer and a job of its own */
        uint64_t a_cap = (uint64_t)n / 4 + 65536, a_bytes = 0, a_lines = 0, at8[BSC_ASM_N_TOTALS];
        int arc = bsc_block_asm_kept(ctx, REF_NAME(dblk.tid), &aspar, a_cap, &a_bytes, &a_lines, at8);
        if (arc == BSC_ERR_ARG && a_bytes > a_cap) arc = bsc_block_asm_kept(ctx, REF_NAME(dblk.tid), &aspar, a_bytes, &a_bytes, &a_lines, at8);
        CHECK(arc);
        asm_lines += a_lines;
        for (int k = 0; k < BSC_ASM_N_TOTALS; k++) asm_tot[k] += at8[k];
        if (a_bytes) {
          void *d_a = NULL;
          uint64_t n_a = 0;
          CHECK(bsc_asm_stream_detach(ctx, &d_a, &n_a));
          if (za) {
            CHECK(bsc_bgzf_write_device(za, d_a, n_a));
            CHECK(bsc_detached_free(ctx, d_a));
            d_a = NULL;
            n_a = 0;
            CHECK(bsc_bgzf_take(za, &d_a, &n_a));
          }
          if (n_a) {
            const out_job j = {d_a, n_a, asm_at, asm_fd, 0};
            writer_push(&W, j);
          }
          asm_at += n_a;
        }
      }
      if (n_bytes && epi_path) { /* the block's epiallele table, from the prepared templates, reads and reference codes the call left on the device: a
                                  * buffer and a job of its own */
        uint64_t e_cap = (uint64_t)n + 4096, e_bytes = 0, e_lines = 0, et[BSC_EPI_N_TOTALS];
        int erc = bsc_block_epi_kept(ctx, REF_NAME(dblk.tid), &eppar, e_cap, &e_bytes, &e_lines, et);
        if (erc == BSC_ERR_ARG && e_bytes > e_cap) erc = bsc_block_epi_kept(ctx, REF_NAME(dblk.tid), &eppar, e_bytes, &e_bytes, &e_lines, et);
        CHECK(erc);
        epi_lines += e_lines;
        for (int k = 0; k < BSC_EPI_N_TOTALS; k++) epi_tot[k] += et[k];
        if (e_bytes) {
          void *d_e = NULL;
          uint64_t n_e = 0;
          CHECK(bsc_epi_stream_detach(ctx, &d_e, &n_e));
          if (ze) {
            CHECK(bsc_bgzf_write_device(ze, d_e, n_e));
            CHECK(bsc_detached_free(ctx, d_e));
            d_e = NULL;
            n_e = 0;
            CHECK(bsc_bgzf_take(ze, &d_e, &n_e));
          }
          if (n_e) {
            const out_job j = {d_e, n_e, epi_at, epi_fd, 0};
            writer_push(&W, j);
          }
          epi_at += n_e;
        }
      }
      if (pat_path) { /* the sites of the contig in front of the block: those between the block before, or the contig's start, and this one more */
        uint64_t more = 0;
        CHECK(bsc_pat_count_sites(codes, codes_len, pat_from, x, &more));
        pat_base += more;
        pat_from = x;
      }
      if (n_bytes && pat_path) { /* the block's pattern table, from the prepared templates, reads and reference codes the call left on the device: a
                                  * buffer and a job of its own */
        uint64_t p_cap = (uint64_t)n * pat_room16 / 16 + 4096, p_bytes = 0, p_lines = 0, pt8[BSC_PAT_N_TOTALS];
        int prc = bsc_block_pat_kept(ctx, REF_NAME(dblk.tid), &ptpar, pat_base, p_cap, &p_bytes, &p_lines, pt8);
        if (prc == BSC_ERR_ARG && p_bytes > p_cap) prc = bsc_block_pat_kept(ctx, REF_NAME(dblk.tid), &ptpar, pat_base, p_bytes, &p_bytes, &p_lines, pt8);
        CHECK(prc);
        pat_room16 = p_bytes * 20 / n + 16; /* (n >= 1) */
        pat_lines += p_lines;
        for (int k = 0; k < BSC_PAT_N_TOTALS; k++) pat_tot[k] += pt8[k];
        if (p_bytes) {
          void *d_p = NULL;
          uint64_t n_p = 0;
          CHECK(bsc_pat_stream_detach(ctx, &d_p, &n_p));
          if (zp) {
            CHECK(bsc_bgzf_write_device(zp, d_p, n_p));
            CHECK(bsc_detached_free(ctx, d_p));
            d_p = NULL;
            n_p = 0;
            CHECK(bsc_bgzf_take(zp, &d_p, &n_p));
          }
          if (n_p) {
            const out_job j = {d_p, n_p, pat_at, pat_fd, 0};
            writer_push(&W, j);
          }
          pat_at += n_p;
        }
      }
      if (n_bytes && variants_path) { /* the block's variant-only stream, selected from the same arrays and encoded by the block's own encoder: a
                                       * buffer and a job of its own */
        uint64_t v_cap = (uint64_t)n / 4 + 65536, v_bytes = 0, v_recs = 0, vt[BSC_VAR_N_TOTALS];
        int vrc = bsc_block_variants_kept(ctx, &vpar, v_cap, &v_bytes, &v_recs, vt);
        if (vrc == BSC_ERR_ARG && v_bytes > v_cap) vrc = bsc_block_variants_kept(ctx, &vpar, v_bytes, &v_bytes, &v_recs, vt);
        CHECK(vrc);
        for (int k = 0; k < BSC_VAR_N_TOTALS; k++) var_tot[k] += vt[k];
        if (v_bytes && vcsi) { /* its index entries, by the variant encoder's own tile offsets: noted at the writer's logical length */
          const bsc_csi_entry *ce = NULL;
          uint64_t cn = 0;
          CHECK(bsc_block_variants_csi_kept(ctx, 14, &ce, &cn, NULL));
          CHECK(bsc_csi_add(vcsi, dblk.tid, ce, cn, v_bytes));
        }
        if (v_bytes) {
          void *d_v = NULL;
          uint64_t n_v = 0;
          CHECK(bsc_variants_stream_detach(ctx, &d_v, &n_v));
          if (zv) {
            CHECK(bsc_bgzf_write_device(zv, d_v, n_v));
            CHECK(bsc_detached_free(ctx, d_v));
            d_v = NULL;
            n_v = 0;
            CHECK(bsc_bgzf_take(zv, &d_v, &n_v));
          }
          if (n_v) {
            const out_job j = {d_v, n_v, var_at, var_fd, 0};
            writer_push(&W, j);
          }
          var_at += n_v;
        }
      }
      if (n_bytes) { /* the stream changes hands: the output thread reads it out and writes it while this one goes on to the next block */
        void *d_stream = NULL;
        uint64_t n_det = 0;
        CHECK(bsc_bcf_stream_detach(ctx, &d_stream, &n_det));
        if (zw) { /* compressed on the device; the members completed so far go to the output thread */
          CHECK(bsc_bgzf_write_device(zw, d_stream, n_det));
          CHECK(bsc_detached_free(ctx, d_stream));
          void *d_z = NULL;
          uint64_t n_z = 0;
          CHECK(bsc_bgzf_take(zw, &d_z, &n_z));
          if (n_z) {
            const out_job j = {d_z, n_z, file_at, out_fd, 0};
            writer_push(&W, j);
          }
          file_at += n_z;
          n_bytes = 0;
        } else {
          const out_job j = {d_stream, n_det, file_at, out_fd, 0};
          writer_push(&W, j);
        }
      }
      file_at += n_bytes;
      n_bytes = 0; /* written by the output thread */
    } else if (!host_bcf) { /* the whole block on the device, the encoding included.  Room for 96 bytes per position: a WGBS block writes a
                      * record of ~113 bytes for every second position; a block that needs more says so and is encoded again */
      if ((size_t)n * 96 + 4096 > cap_bcf) {
        bsc_free_host(bcf);
        bcf = pinned(cap_bcf = (size_t)n * 96 + 4096);
      }
      int rc = bsc_block_bcf_raw(ctx, blk.tpl, blk.nr, blk.seq, blk.seq_bytes, blk.misms, blk.n_misms, &ppar, x, y, ref, NULL, &vp, 1, blk.tid, &ids, NULL, bcf,
                                 cap_bcf, &n_bytes, &n_out, &st, &prof);
      if (rc == BSC_ERR_ARG && n_bytes > cap_bcf) { /* a block of long records: the encoder alone once more, with the room it asks for */
        bsc_free_host(bcf);
        bcf = pinned(cap_bcf = (size_t)n_bytes + 4096);
        rc = bsc_block_bcf_again(ctx, bcf, cap_bcf, &n_bytes, &n_out);
      }
      CHECK(rc);
    } else if (!host_prep) {
      if (n > cap_recs) recs = xrealloc(recs, (cap_recs = (size_t)n * 2) * sizeof *recs);
      CHECK(bsc_block_records_raw(ctx, blk.tpl, blk.nr, blk.seq, blk.seq_bytes, blk.misms, blk.n_misms, &ppar, x, y, ref, NULL, &vp, 1, recs,
                                  cap_recs, &n_out, &st, &prof));
    } else {
      if (n > cap_recs) recs = xrealloc(recs, (cap_recs = (size_t)n * 2) * sizeof *recs);
      uint64_t pad = 0;
      for (uint64_t i = 0; i < blk.n_misms; i++)
        if (blk.misms[i].type == BSC_MISMS_INS) pad += blk.misms[i].size;
      if (blk.seq_bytes + pad + 16 > cap_pseq) pseq = xrealloc(pseq, cap_pseq = (size_t)(blk.seq_bytes + pad + 16) * 2);
      if (blk.nr > cap_tpl) tpl = xrealloc(tpl, (cap_tpl = (size_t)blk.nr * 2) * sizeof *tpl);
      uint64_t used = 0;
      prof.ref = ref;
      prof.x = x;
      prof.n_ref = n + 2;
      CHECK(bsc_prepare_templates_profile(blk.tpl, blk.nr, blk.seq, blk.seq_bytes, blk.misms, blk.n_misms, &ppar, tpl, pseq, cap_pseq, &used, &st,
                                          &prof));
      t_prep += (t1 = now()) - t0;
      t0 = t1;
      CHECK(bsc_block_records(ctx, tpl, blk.nr, pseq, used, x, y, ref, NULL, &vp, 1, recs, cap_recs, &n_out));
    }
    base_filter[0] += st.base_none;
    base_filter[1] += st.base_trim;
    base_filter[2] += st.base_clip;
    base_filter[3] += st.base_overlap;
    base_filter[4] += st.base_lowqual;
    passed_reads += st.reads;
    passed_bases += st.read_bases;
    t_gpu += (t1 = now()) - t0;
    t0 = t1;
    if (host_bcf) {
      if (n_out * 256 + 64 > cap_bcf) {
        bsc_free_host(bcf);
        bcf = pinned(cap_bcf = (size_t)(n_out * 256 + 64) * 2);
      }
      uint64_t done = 0;
      const long nb = bsc_bcf_block(recs, n_out, blk.tid, &ids, NULL, bcf, cap_bcf, &done);
      CHECK(nb);
      if (done != n_out) {
        fprintf(stderr, "BCF buffer too small\n");
        return 1;
      }
      n_bytes = (uint64_t)nb;
    }
    if (n_bytes) fwrite(bcf, 1, (size_t)n_bytes, out);
    n_blocks++;
    n_records += n_out;
    t_enc += (t1 = now()) - t0;
    t0 = t1;
  }
  CHECK(r);
  if (zw) { /* the last member and the end-of-file marker */
    void *d_z = NULL;
    uint64_t n_z = 0;
    CHECK(bsc_bgzf_close(zw, &d_z, &n_z));
    zw = NULL;
    if (n_z) {
      const out_job j = {d_z, n_z, file_at, out_fd, 0};
      writer_push(&W, j);
    }
    file_at += n_z;
    if (csi) { /* the members' sizes are all there: the index's virtual offsets, and the .csi file */
      const long need = bsc_csi_finish(csi, NULL, 0);
      CHECK(need);
      uint8_t *ib = xrealloc(NULL, (size_t)need);
      CHECK(bsc_csi_finish(csi, ib, (uint64_t)need));
      char *ip = xrealloc(NULL, strlen(argv[3]) + 8);
      sprintf(ip, "%s.csi", argv[3]);
      FILE *fi = fopen(ip, "wb");
      if (!fi || fwrite(ib, 1, (size_t)need, fi) != (size_t)need || fclose(fi)) {
        perror(ip);
        return 1;
      }
      free(ip);
      free(ib);
      bsc_csi_close(csi);
      csi = NULL;
    }
  }
  if (zm) { /* the table's last member and its end-of-file marker */
    void *d_z = NULL;
    uint64_t n_z = 0;
    CHECK(bsc_bgzf_close(zm, &d_z, &n_z));
    zm = NULL;
    if (n_z) {
      const out_job j = {d_z, n_z, meth_at, meth_fd, 0};
      writer_push(&W, j);
    }
    meth_at += n_z;
    if (tbx) { /* the members' sizes are all there: the index's virtual offsets, and the .tbi / .csi file beside the table */
      const long need = bsc_tbx_finish(tbx, NULL, 0);
      CHECK(need);
      uint8_t *ib = xrealloc(NULL, (size_t)need);
      CHECK(bsc_tbx_finish(tbx, ib, (uint64_t)need));
      char *ip = xrealloc(NULL, strlen(meth_path) + 8);
      sprintf(ip, "%s.%s", meth_path, meth_index);
      FILE *fi = fopen(ip, "wb");
      if (!fi || fwrite(ib, 1, (size_t)need, fi) != (size_t)need || fclose(fi)) {
        perror(ip);
        return 1;
      }
      free(ip);
      free(ib);
      bsc_tbx_close(tbx);
      tbx = NULL;
    }
  }
  if (zr) { /* the read-level table's last member and its end-of-file marker */
    void *d_z = NULL;
    uint64_t n_z = 0;
    CHECK(bsc_bgzf_close(zr, &d_z, &n_z));
    zr = NULL;
    if (n_z) {
      const out_job j = {d_z, n_z, reads_at, reads_fd, 0};
      writer_push(&W, j);
    }
    reads_at += n_z;
  }
  if (za) { /* the allele-specific table's last member and its end-of-file marker */
    void *d_z = NULL;
    uint64_t n_z = 0;
    CHECK(bsc_bgzf_close(za, &d_z, &n_z));
    za = NULL;
    if (n_z) {
      const out_job j = {d_z, n_z, asm_at, asm_fd, 0};
      writer_push(&W, j);
    }
    asm_at += n_z;
  }
  if (ze) { /* the epiallele table's last member and its end-of-file marker */
    void *d_z = NULL;
    uint64_t n_z = 0;
    CHECK(bsc_bgzf_close(ze, &d_z, &n_z));
    ze = NULL;
    if (n_z) {
      const out_job j = {d_z, n_z, epi_at, epi_fd, 0};
      writer_push(&W, j);
    }
    epi_at += n_z;
  }
  if (zp) { /* the pattern table's last member and its end-of-file marker */
    void *d_z = NULL;
    uint64_t n_z = 0;
    CHECK(bsc_bgzf_close(zp, &d_z, &n_z));
    zp = NULL;
    if (n_z) {
      const out_job j = {d_z, n_z, pat_at, pat_fd, 0};
      writer_push(&W, j);
    }
    pat_at += n_z;
  }
  if (zv) { /* the variant file's last member and its end-of-file marker; its index */
    void *d_z = NULL;
    uint64_t n_z = 0;
    CHECK(bsc_bgzf_close(zv, &d_z, &n_z));
    zv = NULL;
    if (n_z) {
      const out_job j = {d_z, n_z, var_at, var_fd, 0};
      writer_push(&W, j);
    }
    var_at += n_z;
    if (vcsi) {
      const long need = bsc_csi_finish(vcsi, NULL, 0);
      CHECK(need);
      uint8_t *ib = xrealloc(NULL, (size_t)need);
      CHECK(bsc_csi_finish(vcsi, ib, (uint64_t)need));
      char *ip = xrealloc(NULL, strlen(variants_path) + 8);
      sprintf(ip, "%s.csi", variants_path);
      FILE *fi = fopen(ip, "wb");
      if (!fi || fwrite(ib, 1, (size_t)need, fi) != (size_t)need || fclose(fi)) {
        perror(ip);
        return 1;
      }
      free(ip);
      free(ib);
      bsc_csi_close(vcsi);
      vcsi = NULL;
    }
  }
  if (W.started) { /* the output thread writes what it still holds, then goes */
    pthread_mutex_lock(&W.mu);
    W.quit = 1;
    pthread_cond_broadcast(&W.cv);
    pthread_mutex_unlock(&W.mu);
    pthread_join(W.th, NULL);
    if (W.failed) {
      fprintf(stderr, "writing %s failed\n", argv[3]);
      return 1;
    }
    t_enc += (t1 = now()) - t0;
    t0 = t1;
  }
  if (meth_fd >= 0 && close(meth_fd)) {
    perror(meth_path);
    return 1;
  }
  if (mbias_f) { /* the run's one M-bias table: the accumulator of every block, read, formatted and written here */
    const size_t cells = (size_t)BSC_MBIAS_N_BINS * mbpar.n_cycles * 2u;
    uint64_t *mb_counts = calloc(cells, sizeof *mb_counts);
    if (!mb_counts) {
      fprintf(stderr, "%s: out of memory\n", argv[0]);
      return 1;
    }
    if (mbias_any) CHECK(bsc_mbias_read(ctx, mb_counts, mbias_tot)); /* (a run without a block has no accumulator: the header alone) */
    const long mb_need = bsc_mbias_format(mb_counts, &mbpar, NULL, 0);
    char *mb_text = mb_need > 0 ? malloc((size_t)mb_need) : NULL;
    if (!mb_text || bsc_mbias_format(mb_counts, &mbpar, mb_text, (size_t)mb_need) != mb_need ||
        fwrite(mb_text, 1, (size_t)mb_need, mbias_f) != (size_t)mb_need || fclose(mbias_f)) {
      perror(mbias_path);
      return 1;
    }
    mbias_f = NULL;
    free(mb_text);
    free(mb_counts);
  }
  if (reads_fd >= 0 && close(reads_fd)) {
    perror(reads_path);
    return 1;
  }
  if (asm_fd >= 0 && close(asm_fd)) {
    perror(asm_path);
    return 1;
  }
  if (epi_fd >= 0 && close(epi_fd)) {
    perror(epi_path);
    return 1;
  }
  if (pat_fd >= 0 && close(pat_fd)) {
    perror(pat_path);
    return 1;
  }
  if (var_fd >= 0 && close(var_fd)) {
    perror(variants_path);
    return 1;
  }
  if (bw) { /* every block's data are in: the section count, the indexes, the zoom levels, the summary and the header */
    CHECK(bsc_bigwig_finish(bw));
    bsc_bigwig_close(bw);
    if (close(bw_fd)) {
      perror(bigwig_path);
      return 1;
    }
  }
  if (cw) { /* the coverage track's, likewise */
    CHECK(bsc_bigwig_finish(cw));
    bsc_bigwig_close(cw);
    if (close(cw_fd)) {
      perror(cov_path);
      return 1;
    }
  }
  if (bb) { /* every block's items are in: the item count, the indexes, the zoom levels, the summary and the header */
    CHECK(bsc_bigbed_finish(bb));
    bsc_bigbed_close(bb);
    if (close(bb_fd)) {
      perror(bigbed_path);
      return 1;
    }
  }
  if (fout) { /* the last contig's lines */
    if (cur_tid >= 0) frag_lines += frags_flush(ctx, fout, REF_NAME(cur_tid), r_regs, r_names, r_n);
    if (fclose(fout)) {
      perror(frags_path);
      return 1;
    }
  }
  if (rout) { /* the last contig's lines */
    if (cur_tid >= 0) region_lines += regions_flush(ctx, rout, REF_NAME(cur_tid), r_regs, r_names, r_n);
    if (fclose(rout)) {
      perror(regions_out_path);
      return 1;
    }
  }
  if (rout || fout) {
    free(rwin);
    free(rbed_of);
    bsc_meth_bed_free(rbed);
  }
  const double t_loop_end = now();
  if (cur_tid >= 0) {
    CHECK(bsc_get_site_totals(ctx, after));
    uint64_t *d = ctot[cur_tid].snps;
    for (int i = 0; i < 14; i++) d[i] += after[i] - before[i];
  }
  if (out && fclose(out) && bgzf) {
    perror(argv[3]);
    return 1;
  } else if (!out && out_fd >= 0) close(out_fd);

  /* the report */
  static bsc_site_stats total;
  CHECK(bsc_get_site_stats(ctx, &total));
  bsc_report rep;
  memset(&rep, 0, sizeof rep);
  rep.under_conv = prm.under_conv;
  rep.over_conv = prm.over_conv;
  rep.mapq_thresh = 20;
  rep.min_qual = 20;
  rep.day = 1, rep.month = 1, rep.year = 2000; /* a fixed date: reproducible output */
  if (host_reader) bsc_bam_filter_counts(bam, rep.filter_cts, rep.filter_bases);
  else CHECK(bsc_bamdev_filter_counts(dev, rep.filter_cts, rep.filter_bases));
  const unsigned long long malformed = host_reader ? bsc_bam_malformed(bam) : bsc_bamdev_malformed(dev);
  if (malformed)
    fprintf(stderr, "bam2bcf: warning: %llu BAM records dropped, their CIGAR does not cover the sequence (damaged input?)\n", malformed);
  rep.filter_cts[0] += passed_reads;
  rep.filter_bases[0] += passed_bases;
  memcpy(rep.base_filter, base_filter, sizeof base_filter);
  rep.total = &total;
  rep.have_dbsnp = g_dbsnp != NULL;
  CHECK(bsc_set_gc_bins_host(ctx, NULL, 0, 0));
  uint64_t *gc_table = xrealloc(NULL, (size_t)BSC_COV_CAP * 101 * sizeof(uint64_t));
  CHECK(bsc_get_gc_stats(ctx, gc_table));
  rep.gc = gc_table;
  rep.read_profile = &prof_counts[0][0];
  rep.n_read_profile = prof.used;
  /* contigs in header order, as the reference lists them */
  bsc_contig_totals *listed = calloc((size_t)n_ref + 1, sizeof *listed);
  uint32_t nl = 0;
  for (int i = 0; i < n_ref; i++)
    if (ctot[i].name) listed[nl++] = ctot[i];
  rep.contigs = listed;
  rep.n_contigs = nl;
  if (sharded) { /* this rank's share of every sum, for bam2bcf --merge */
    rank_sums *rs_ = calloc(1, sizeof *rs_);
    rs_->magic = SUMS_MAGIC;
    rs_->n_ref = (uint64_t)n_ref;
    rs_->n_blocks = n_blocks;
    rs_->n_records = n_records;
    rs_->malformed = malformed;
    memcpy(rs_->filter_cts, rep.filter_cts, sizeof rs_->filter_cts);
    memcpy(rs_->filter_bases, rep.filter_bases, sizeof rs_->filter_bases);
    memcpy(rs_->base_filter, base_filter, sizeof rs_->base_filter);
    rs_->prof_used = prof.used;
    memcpy(rs_->prof, prof_counts, sizeof rs_->prof);
    rs_->total = total;
    uint64_t *ct = calloc((size_t)n_ref * 15 + 1, 8);
    for (int i = 0; i < n_ref; i++)
      if (ctot[i].name) {
        ct[(size_t)i * 15] = 1;
        memcpy(ct + (size_t)i * 15 + 1, ctot[i].snps, 14 * 8);
      }
    char *sp = malloc(strlen(argv[3]) + 32);
    sprintf(sp, "%s.rank%05d.sums", argv[3], rank);
    FILE *fs = fopen(sp, "wb");
    if (!fs || fwrite(rs_, sizeof *rs_, 1, fs) != 1 || fwrite(gc_table, 8, (size_t)BSC_COV_CAP * 101, fs) != (size_t)BSC_COV_CAP * 101 ||
        fwrite(ct, 8, (size_t)n_ref * 15, fs) != (size_t)n_ref * 15 || fclose(fs)) {
      perror(sp);
      return 1;
    }
    printf("rank %d of %d: %llu blocks, %llu records written\n", rank, world, (unsigned long long)n_blocks, (unsigned long long)n_records);
  } else {
    const long need = bsc_report_json(&rep, NULL, 0);
    CHECK(need);
    char *text = xrealloc(NULL, (size_t)need + 1);
    bsc_report_json(&rep, text, (size_t)need + 1);
    FILE *fr = fopen(argv[4], "w");
    if (!fr) {
      perror(argv[4]);
      return 1;
    }
    fwrite(text, 1, (size_t)need, fr);
    fclose(fr);
    printf("%llu blocks, %llu records written\n", (unsigned long long)n_blocks, (unsigned long long)n_records);
    if (meth_path) printf("%llu methylation table lines written\n", (unsigned long long)meth_lines);
    if (regions_out_path) printf("%llu methylation region lines written\n", (unsigned long long)region_lines);
    if (bigwig_path) printf("%llu methylation bigWig sites written\n", (unsigned long long)bw_sites);
    if (cov_path) printf("%llu coverage bigWig sites written\n", (unsigned long long)cw_sites);
    if (bigbed_path) printf("%llu bedMethyl bigBed items written\n", (unsigned long long)bb_sites);
    if (variants_path)
      printf("%llu variant records written (snp %llu, multi %llu, het %llu, pass %llu, known %llu, ts %llu, tv %llu)\n", (unsigned long long)var_tot[0],
             (unsigned long long)var_tot[1], (unsigned long long)var_tot[2], (unsigned long long)var_tot[3], (unsigned long long)var_tot[4],
             (unsigned long long)var_tot[5], (unsigned long long)var_tot[7], (unsigned long long)var_tot[8]);
    if (reads_path)
      printf("%llu CpG sites in the read-level table, %llu lines written (eligible templates %llu, discordant %llu)\n", (unsigned long long)reads_tot[0],
             (unsigned long long)reads_lines, (unsigned long long)reads_tot[5], (unsigned long long)reads_tot[6]);
    if (asm_path)
      printf("%llu heterozygous SNPs in the allele-specific methylation table, %llu SNP-CpG pairs, %llu lines written (allele observations %llu)\n",
             (unsigned long long)asm_tot[0], (unsigned long long)asm_tot[1], (unsigned long long)asm_lines, (unsigned long long)asm_tot[2]);
    if (epi_path)
      printf("%llu windows of four CpGs in the epiallele table, %llu lines written (patterns %llu, templates with one %llu)\n",
             (unsigned long long)epi_tot[0], (unsigned long long)epi_lines, (unsigned long long)epi_tot[1], (unsigned long long)epi_tot[2]);
    if (pat_path)
      printf("%llu records in the per-read CpG pattern table, %llu lines written (pieces %llu, templates %llu, C %llu T %llu)\n",
             (unsigned long long)pat_tot[0], (unsigned long long)pat_lines, (unsigned long long)pat_tot[1], (unsigned long long)pat_tot[2],
             (unsigned long long)pat_tot[3], (unsigned long long)pat_tot[4]);
    if (frags_path)
      printf("%llu fragment summary lines written (templates with a CpG state %llu; fragments in regions %llu: U %llu, X %llu, M %llu, discordant %llu)\n",
             (unsigned long long)frag_lines, (unsigned long long)frag_tot[0], (unsigned long long)frag_tot[1], (unsigned long long)frag_tot[2],
             (unsigned long long)frag_tot[3], (unsigned long long)frag_tot[4], (unsigned long long)frag_tot[7]);
    if (mbias_path)
      printf("M-bias table: %llu reads walked, %llu bytes mapped, %llu counted, %llu beyond the table, CpG %llu meth %llu unmeth, %llu reads skipped\n",
             (unsigned long long)mbias_tot[0], (unsigned long long)mbias_tot[1], (unsigned long long)mbias_tot[2], (unsigned long long)mbias_tot[3],
             (unsigned long long)mbias_tot[4], (unsigned long long)mbias_tot[5], (unsigned long long)mbias_tot[6]);
  }
  if (getenv("BAM2BCF_TIMING")) {
    uint64_t rc4[4] = {0, 0, 0, 0};
    double rs[2] = {0, 0};
    if (dev) bsc_bamdev_run_stats(dev, rc4, rs);
    fprintf(stderr,
            "{\"reader\": \"%s\", \"context_s\": %.3f, \"reader_s\": %.3f, \"reference_s\": %.3f, \"host_prep_s\": %.3f, \"block_call\": \"%s\", "
            "\"block_call_s\": %.3f, \"encode_write_s\": %.3f, \"report_s\": %.3f, \"wall_s\": %.3f, \"wall_without_context_s\": %.3f, "
            "\"device_reader\": {\"passes\": %llu, \"replay_passes\": %llu, \"records\": %llu, \"inflated_bytes\": %llu, \"waiting_for_inflate_s\": %.3f, "
            "\"device_passes_s\": %.3f}, \"output_thread\": {\"waiting_for_a_block_s\": %.3f, \"waiting_for_copies_s\": %.3f, \"pwrite_s\": %.3f}}\n",
            host_reader ? "host (csrc/bamio.c)" : "device (csrc/bamstream.c + csrc/bamdev.hip)", t_ctx, t_read, t_ref, t_prep,
            host_prep ? "bsc_block_records" : (host_bcf ? "bsc_block_records_raw" : (host_reader ? "bsc_block_bcf_raw" : (text ? "bsc_block_vcf_rawdev" : "bsc_block_bcf_rawdev"))), t_gpu, t_enc,
            now() - t_loop_end, now() - t_start, now() - t_start - t_ctx, (unsigned long long)rc4[0], (unsigned long long)rc4[1], (unsigned long long)rc4[2],
            (unsigned long long)rc4[3], rs[0], rs[1], W.t_idle, W.t_wait, W.t_write);
  }
  if (RJ.running) { /* a contig prefetched and never reached */
    pthread_join(RJ.th, NULL);
    free(RJ.codes);
    free(RJ.gc);
  }
  if (bam) bsc_bam_close(bam);
  if (dev) bsc_bamdev_close(dev);
  bsc_destroy(ctx);
  bsc_dbsnp_close(g_dbsnp);
  return 0;
}
