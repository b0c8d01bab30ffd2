/*
 * bscall_amd.h — C ABI of libbscall_amd.so: bs_call's per-site genotype + methylation calling path
 * (pile-up -> gt_meth) as hand-written gfx950 (MI355X) HIP kernels.
 *
 * Plain C, plain pointers and sizes; no C++/torch types.  Every entry point names the piece of the
 * reference (heathsc/bs_call v2.1.7) it stands in for; INTEGRATION.md shows the replacement
 * src/call_genotypes.c a maintainer would compile inside the reference tree against this header.
 *
 * The record layouts are the reference's own, byte for byte, so host arrays of the reference's
 * `pileup` / `gt_meth` can be passed without conversion.
 *
 * All functions return BSC_OK (0) or a negative BSC_ERR_* code; bsc_last_error() gives the text (per thread).
 * Threading: a context is used by one thread at a time, like the reference's calc pool is driven by its single
 * process thread; calls on one context must be ordered on one stream (the context owns a heterozygous-site list and
 * counters that successive launches reuse).  Independent work = independent contexts (e.g. one per GPU).
 * There is NO CPU fallback: without a usable gfx950 device bsc_create() fails with BSC_ERR_NO_DEVICE.
 *
 * MAP OF THE ENTRIES.  A caller picks ONE level — where a block enters the library and what comes back; the other ~120 names are the same
 * computation cut at another place, fed from another kind of memory, or the readers / writers / counters around it.
 *
 *   level                          in -> out                                            entry                                   replaces (reference)
 *   1   the calc threads           pileup[] -> gt_meth[] / gt_vcf[]                      bsc_call_sites                          call_thread's loop (src/call_genotypes.c:43-115)
 *   2a  + the accumulate loop      templates + reads -> gt_vcf[]                         bsc_call_block                          call_genotypes_ML (:155-273)
 *       ... the printer's records  templates + reads -> written records, packed          bsc_block_records                       + _print_vcf_entry up to the encoding (src/print_vcf.c:32-594)
 *   2b  + the print thread         templates + reads -> the block's BCF bytes            bsc_block_bcf                           + bcf_enc_* / bcf_write (:160-222,267-378)
 *   3   + the process thread       raw templates + mismatch lists -> BCF bytes           bsc_block_bcf_raw                       + process_template (src/process_template.c:36-111)
 *   4   + the reader thread        a BAM file -> blocks in HBM -> BCF bytes              bsc_bamdev_next_block + bsc_block_bcf_rawdev[_keep]   + read_input (src/get_template_vector.c:49-389)
 *
 *   The suffixes say WHERE THE BUFFERS LIVE and WHEN THE CALL RETURNS, nothing else: (none) the caller's ordinary memory, staged by the
 *   library, results on return; _inplace: the caller's page-locked memory (bsc_alloc_host), no staging copy; _submit / _fetch: the call in two
 *   halves, the host thread returns while the GPU works (one block in flight per context, as the reference hands a block to its calc
 *   threads); _to: results into caller-provided page-locked memory; _device: everything HBM-resident, asynchronous on the caller's stream;
 *   bsc_blocks_*: several small blocks in one launch sequence (records, gt_vcf images, or — bsc_blocks_bcf_* — one BCF stream).
 *   Below the levels: their device-resident pieces for callers that keep whole contigs in HBM (bsc_accumulate_device, bsc_chain_device,
 *   bsc_reads_chain[_len]_device, bsc_vcf_*_device, bsc_bcf_*_device: what bench.py and bs_call_amd/genome.py drive); host-side readers and
 *   writers (bsc_bam_*, bsc_bamstream_*, bsc_dbsnp_*, bsc_fasta_contig, bsc_prepare_templates, bsc_bcf_record, bsc_vcf_format,
 *   bsc_report_json); statistics and inspection (bsc_get_*, bsc_reset_*, bsc_last_*_ms).  INTEGRATION.md section 1 lists every name.
 */
#ifndef BSCALL_AMD_H
#define BSCALL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSC_ABI_VERSION 2

#define BSC_OK 0
#define BSC_ERR_ARG (-1)       /* bad argument (the reference would assert: src/call_genotypes.c:158,186,188) */
#define BSC_ERR_HIP (-2)       /* a HIP runtime call failed */
#define BSC_ERR_NOMEM (-3)     /* host or device allocation failed */
#define BSC_ERR_NO_DEVICE (-4) /* no gfx950 device / kernels not loadable */
#define BSC_ERR_RANGE (-5)     /* an input beyond what a fixed-size device table holds: the result would be incomplete */
#define BSC_WARN_INEXACT 1     /* results written, but some pile-up sums left the range where float sums are exact */

/* `pileup`, include/bs_call.h:174-182 — 104 bytes */
typedef struct {
  uint32_t counts[2][8]; /* [orientation][class]; classes 0-3 non-informative ACGT, 4-7 informative ACGT */
  uint32_t n;            /* bases that passed the quality filter */
  float quality[8];      /* sum of base qualities per class */
  float mapq2;           /* sum of MAPQ^2 */
} bsc_pileup;

/* `gt_meth`, include/bs_call.h:152-160 — 200 bytes */
typedef struct {
  uint64_t counts[8];
  int32_t qual[8];      /* rounded mean quality per class */
  double gt_prob[10];   /* log10 posterior, order AA AC AG AT CC CG CT GG GT TT */
  double fisher_strand; /* log10 Fisher strand-bias p (0 for homozygous calls) */
  int32_t mq;           /* RMS mapping quality */
  int32_t aq;           /* mean base quality */
  uint8_t max_gt;       /* argmax of gt_prob (first maximum) */
} bsc_gt_meth;

/* One template (read pair) flattened out of `align_details`, include/bs_call.h:64-73 — 40 bytes.
 * Read k holds len[k] bytes of base|qual<<2 (GET_BASE/GET_QUAL, include/bs_call.h:41-42) at seq+off[k],
 * already trimmed/clipped/normalised by the host so that byte j sits at genome position pos[k]+j. */
typedef struct {
  uint32_t pos[2];     /* forward_position, reverse_position; 0 = none */
  uint32_t len[2];     /* 0 = read absent */
  uint64_t off[2];     /* byte offsets into the block's concatenated read buffer */
  uint8_t mapq[2];
  uint8_t orientation; /* gt_strand: 0 FORWARD, 1 REVERSE */
  uint8_t bs_strand;   /* gt_bs_strand: 0 NON_CONVERTED, 1 STRAND_C2T, 2 STRAND_G2A */
  uint32_t flags;      /* 0, or BSC_TPL_* (ABI 2; the field was padding, required to be 0, before); any other bit: BSC_ERR_ARG */
} bsc_template;

/*
 * bsc_template.flags.  HOT LOOP A flips the orientation for read 1 only if read 0 "was walked": if it holds a base whose
 * quality is neither 0 nor 63 (the scan of src/call_genotypes.c:198-211 and the `continue`s in front of :224).  A host that
 * writes the read bytes knows that bit and can hand it over; otherwise (flags = 0) the device finds it out itself, which costs
 * it a 128-byte memory line per template for the one byte that usually decides.  BSC_TPL_WALK_KNOWN without a correct
 * BSC_TPL_WALKED0 gives a pile-up the reference would not: use bsc_template_walk_flags().
 */
#define BSC_TPL_WALK_KNOWN 1u /* BSC_TPL_WALKED0 is valid */
#define BSC_TPL_WALKED0 2u    /* read 0 has a base with 0 < quality < 63 */
uint32_t bsc_template_walk_flags(const uint8_t *read0, uint32_t len0); /* host C (csrc/prep.c): stops at the first countable base */

/* Model parameters: sr_param.under_conv/over_conv/ref_bias/min_qual (include/bs_call.h:320-324;
 * defaults src/init_param.c:26-31 = 0.01, 0.05, 2, 20; min_qual is clamped to [1,43] as in
 * src/parse_args.c:170-171). */
typedef struct {
  double under_conv;
  double over_conv;
  double ref_bias;
  int32_t min_qual;
  int32_t device; /* HIP device ordinal; -1 = current device */
} bsc_params;

/* Per-context counters, summed over every call since creation / bsc_reset_stats().  These are the
 * fixed-size blocks that ranks all-reduce at the end of a sharded run. */
#define BSC_STATS_WORDS 16
typedef struct {
  uint64_t sites;      /* positions processed */
  uint64_t covered;    /* positions with n > 0 (not skipped) */
  uint64_t gt_hist[10];/* called genotype histogram over covered positions */
  uint64_t het_calls;  /* covered positions whose call is heterozygous (Fisher test evaluated) */
  uint64_t reserved[3];
} bsc_stats;

typedef struct bsc_context bsc_context;

int bsc_abi_version(void);
const char *bsc_last_error(void);
void bsc_params_default(bsc_params *p);

/*
 * bsc_create: replaces fill_base_prob_table() + init_calc_threads() (src/process.c:165-166;
 * src/genotype_model.c:10-21; src/call_genotypes.c:124-138) and the lfact_store / gt_het tables of
 * init_param() (src/init_param.c:16,52-55).  Builds the tables on the host with libm exactly as the
 * reference does, uploads them verbatim, creates the context's HIP stream and workspaces.
 * BSC_NUM_CUS in the environment, an integer in [1, the device's CU count], lowers the CU count that this context's grids and the
 * workspaces sized from them follow (for tests of the grid-stride rounds; any other value is ignored, and it never raises the count).
 */
int bsc_create(const bsc_params *params, bsc_context **out);

/* bsc_destroy: replaces join_calc_threads() (src/call_genotypes.c:140-153). */
int bsc_destroy(bsc_context *ctx);

/* Copies the host-built tables out: q_prob as [44][5] doubles (e,k,ln_k,ln_k_half,ln_k_one;
 * include/bs_call.h:148-150) and lfact_store[256] (src/stats_utils.c:14-21). */
int bsc_get_tables(const bsc_context *ctx, double *q_prob_44x5, double *lfact_256);

/*
 * The QUAL staircase the fused chain reads instead of evaluating src/print_vcf.c:140-148's log: phred = (int)(-10 *
 * log(om) / LOG10) capped at 255 is, as a function of om = 1 - exp(LOG10 * gt_prob[max_gt]), a staircase; for the binade
 * e = 1023 - exponent(om) (0 .. 63) of om, phred = base_64[e] + the number of thr_64x4[e][0..3] that om does not exceed.
 * Built on the host by bisection with the operations the kernels' log path runs (a context builds the same table and fails
 * if the staircase is not monotone).  No GPU involved: what tests/test_phred_table.py checks against libm double by double
 * around every step.  Returns BSC_OK or BSC_ERR_ARG.
 */
int bsc_phred_table(double *thr_64x4, unsigned char *base_64);

/*
 * bsc_call_sites: the call_thread() loop over one block (src/call_genotypes.c:43-115): per site the
 * quality/MAPQ summary, calc_gt_prob(), the strand table + fisher() for heterozygous calls.
 *   cts[n]  pile-ups (host memory)
 *   ref[n]  reference codes 0..4 = N,A,C,G,T for the same positions (src/get_sequence.c:20-54)
 *   out     n records of `out_stride` bytes each, out_stride = 200 (a gt_meth array) or 208 (a gt_vcf array,
 *           include/bs_call.h:162-166: gt_meth, then ready = 0 at byte 200 and skip at byte 201); the first 200
 *           bytes of record i are the gt_meth of site i (all zero for a skipped site).
 *   skip[n] 1 where n == 0 (gt_vcf.skip), else 0
 * Synchronous: returns when `out` and `skip` are filled.
 */
int bsc_call_sites(bsc_context *ctx, const bsc_pileup *cts, const uint8_t *ref, uint64_t n, void *out,
                   uint32_t out_stride, uint8_t *skip);

/* Pinned (page-locked) host memory for buffers passed to the host-buffer entries: with it the copies of
 * bsc_call_sites are true DMA transfers that overlap the kernels (three-stage pipeline over 1 Mi-site chunks);
 * pageable memory works too but is staged by the runtime.  E.g. allocate work->vcf with it. */
void *bsc_alloc_host(uint64_t bytes);
void bsc_free_host(void *p);

/*
 * Same computation on device-resident buffers; asynchronous on `stream` (a hipStream_t; NULL = HIP's default
 * stream, e.g. what torch.cuda.current_stream().cuda_stream returns for PyTorch's default stream).  The caller
 * orders its own work against that stream.  d_cts/d_out must be 16-byte aligned.  Used by bench.py and by
 * pipelines that keep pile-ups in HBM.
 */
int bsc_call_sites_device(bsc_context *ctx, const void *d_cts, const void *d_ref, uint64_t n, void *d_out,
                          uint32_t out_stride, void *d_skip, void *stream);

/*
 * bsc_accumulate: HOT LOOP A of call_genotypes_ML (src/call_genotypes.c:178-226) on the device: scatter the
 * block's reads into the pile-up of positions x..y (inclusive, 1-based genome positions as in the reference).
 *   tpl[nr]   templates in any order, like the reference's align_list (the sums do not depend on the order; the
 *             device orders them by leftmost position for its own tiling)
 *   seq       the concatenated read bytes the templates point into (seq_bytes long)
 *   out       y - x + 1 pile-ups (host memory), zero where nothing is covered
 * Returns BSC_ERR_ARG where the reference asserts (y < x; a template starting left of x; orientation > 1) or
 * where a template points outside seq — the templates are checked by the kernel that reads them, before anything
 * they point at is touched, and nothing is written to `out` for a bad block; BSC_WARN_INEXACT if a position's quality or MAPQ^2 sum exceeded 2^24
 * (the reference's float sums are order-dependent there).  Uses ctx min_qual.
 */
int bsc_accumulate(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                   uint32_t x, uint32_t y, bsc_pileup *out);

/*
 * bsc_accumulate_device: the same stage on device-resident inputs — d_tpl[nr] (bsc_template, 8-byte aligned), d_seq
 * (seq_bytes read bytes) -> d_cts, the pile-ups of x .. y (16-byte aligned; room for y - x + 1 rounded up to a whole
 * number of 64-position tiles, x 104 bytes: the last tile is written whole).  Asynchronous on `stream`.  The templates
 * are validated by the kernel that reads them; bsc_block_status() waits for `stream` and returns the verdict of the
 * block queued last: BSC_OK, BSC_WARN_INEXACT or BSC_ERR_ARG naming the first template that breaks one of the
 * reference's asserts (src/call_genotypes.c:186-188) — such a template contributes nothing to the pile-up.
 * bsc_last_accumulate_ms (with bsc_set_profiling): device time of the stage's launches (template checks + read
 * descriptors, ordering, tile search, accumulate) of the most recent call, from HIP events on its stream.
 */
int bsc_accumulate_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x,
                          uint32_t y, void *d_cts, void *stream);
int bsc_block_status(bsc_context *ctx, void *stream);
int bsc_last_accumulate_ms(bsc_context *ctx, float *ms);

/*
 * bsc_call_block: the compute of one call_genotypes_ML() invocation (src/call_genotypes.c:155-273) without its
 * thread hand-offs: accumulate (above) followed by the per-site calling of bsc_call_sites(), the pile-up never
 * leaving the device.  ref[i] is the reference code of position x + i; out / out_stride / skip as in
 * bsc_call_sites().  INTEGRATION.md shows the replacement call_genotypes_ML() built on this.
 */
int bsc_call_block(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                   uint32_t x, uint32_t y, const uint8_t *ref, void *out, uint32_t out_stride, uint8_t *skip);

/*
 * Asynchronous form of bsc_call_block, mirroring how call_genotypes_ML() dispatches a block to the calc threads and
 * returns at once (src/call_genotypes.c:260-272) so that the process thread can prepare the next block meanwhile:
 *   bsc_block_submit  copies the block's inputs into pinned staging (tpl / seq / ref may be recycled when it
 *                     returns, as the reference's align_list is), queues copy + accumulate + call, returns;
 *   bsc_block_fetch   waits for that block and copies its records into out / skip (sizes as submitted); returns
 *                     BSC_WARN_INEXACT like bsc_accumulate.  The templates are checked on the device (see
 *                     bsc_accumulate), so a block that breaks one of the reference's asserts is reported here,
 *                     BSC_ERR_ARG, with nothing written — not by bsc_block_submit.
 * One block in flight per context, as in the reference (src/call_genotypes.c:161-168).
 */
int bsc_block_submit(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                     uint32_t x, uint32_t y, const uint8_t *ref, uint32_t out_stride);
int bsc_block_fetch(bsc_context *ctx, void *out, uint8_t *skip);
/* bsc_block_submit with the destination named up front: the copy-out is queued right behind the kernels, so the records
 * travel to the host while the caller prepares its next block, and bsc_block_fetch(ctx, NULL, NULL) only waits and
 * reports.  out / skip should come from bsc_alloc_host (with pageable memory the call waits for the block instead of
 * returning at once); their contents are undefined until the fetch has returned, and after a fetch that failed. */
int bsc_block_submit_to(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                        uint32_t x, uint32_t y, const uint8_t *ref, void *out, uint32_t out_stride, uint8_t *skip);

/*
 * VCF record formation: what the reference's print thread derives from a block's gt_meth records before it hands a
 * record to htslib (_print_vcf_entry, src/print_vcf.c:32-381, with the 5-site window of print_vcf_entry /
 * flush_vcf_entries, :529-594).  One 64-byte bsc_vcf_core per position; a host formatter turns the records with
 * emit = 1 into VCF/BCF lines.  Not covered: dbSNP names (pass rs_found per position in `dbsnp`, or NULL), the JSON
 * statistics, the header.
 */
typedef struct {
  uint32_t pos;     /* 1-based position; 0 in an all-zero record = nothing called here */
  uint8_t emit;     /* 1: the reference would write a record (not hom-ref AA/TT unless all_positions or dbSNP, in region) */
  uint8_t gt;       /* called genotype 0..9 (first-max argmax of gt_prob, src/print_vcf.c:584-591) */
  uint8_t ref_code; /* REF base code 0..4 as the printer sees it (an N up to two positions before blanks it, :570-577) */
  uint8_t gt_enc;   /* FORMAT GT: two BCF allele codes ((allele+1)<<1), high and low nibble (reference gt_int table) */
  uint8_t flt;      /* 1 q20, 2 qd2, 4 fs60, 8 mq40 (FILTER fail / FT names), 128 mac1; 0 = PASS */
  uint8_t phred;    /* QUAL and FORMAT GQ; 0 in a record with emit = 0 (the printer computes it for every position,
                       src/print_vcf.c:140-148, and reads it behind `skip` only, :185-217,382-398; round 5) */
  uint8_t n_gl;     /* number of FORMAT GL values */
  char cg;          /* FORMAT CG: 'C' (= "CG"), 'H', 'N', '?', '.' */
  char alt[2];      /* ALT alleles, 0-padded */
  char cx_ref[5];   /* INFO CX: reference context */
  char cx_gt[5];    /* FORMAT CX: IUPAC context of the called genotypes */
  int32_t fs;       /* FORMAT FS (the reference writes it for heterozygous genotypes only) */
  uint32_t qd;      /* FORMAT QD; 0 where emit = 0, like phred */
  uint32_t dp;      /* FORMAT DP (non-informative depth) */
  float gl[6];      /* FORMAT GL */
  uint32_t _pad;
} bsc_vcf_core;

typedef struct {
  int32_t all_positions; /* sr_param.all_positions (-A) */
  uint32_t reg_start;    /* emit only reg_start <= position <= reg_stop: ctg->curr_reg, or 1 .. ctg->end_pos */
  uint32_t reg_stop;
} bsc_vcf_params;

/* Host buffers: gtm = n records of gtm_stride bytes (200 or 208) for positions x .. x+n-1, skip[n], ref[n+2] = the
 * reference codes of x .. x+n+1 (work->ref), dbsnp[n] = rs_found (0/1/3) per position or NULL; out[n]. */
int bsc_vcf_records(bsc_context *ctx, const void *gtm, uint32_t gtm_stride, const uint8_t *skip, const uint8_t *ref,
                    const uint8_t *dbsnp, uint32_t n, uint32_t x, const bsc_vcf_params *params, bsc_vcf_core *out);
/* Same on device-resident buffers, asynchronous on `stream` (chains behind bsc_call_sites_device). */
int bsc_vcf_records_device(bsc_context *ctx, const void *d_gtm, uint32_t gtm_stride, const void *d_skip,
                           const void *d_ref, const void *d_dbsnp, uint32_t n, uint32_t x,
                           const bsc_vcf_params *params, void *d_out, void *stream);

/*
 * Written records only, packed — what a host that renders VCF/BCF needs from a block: for every position with
 * emit = 1, in position order, its bsc_vcf_core and the gt_meth fields the encoder still reads (MC8 = counts,
 * AMQ = qual, MQ; src/print_vcf.c:306-359).  64 bytes per position on average on WGBS data instead of the 201 of a
 * gt_vcf entry, which is what bounds the host-buffer paths (PCIe).
 */
typedef struct {
  bsc_vcf_core core;  /* 64 bytes */
  uint32_t counts[8]; /* gt_meth.counts (a count beyond 2^32 - 1 saturates) */
  uint8_t qual[8];    /* gt_meth.qual, 0..43 */
  int32_t mq, aq;     /* gt_meth.mq, gt_meth.aq */
  uint8_t max_gt;     /* gt_meth.max_gt */
  uint8_t rs_found;   /* the dbSNP flag that was passed for the position (0 without dbSNP) */
  uint8_t _pad[14];
} bsc_vcf_rec;

/* d_core[n] / d_gtm[n] (device) -> d_out[min(*count, out_cap)] packed records and the number of written records of the
 * block in *d_count (a device u64; records beyond out_cap are counted, not stored).  Asynchronous on `stream`.
 * gtm_stride = 0: d_gtm is the d_aux array of bsc_reads_chain_device (64 bytes per position, already the second half of
 * the packed record; d_dbsnp is then unused: the flag is in it). */
int bsc_vcf_compact_device(bsc_context *ctx, const void *d_core, const void *d_gtm, uint32_t gtm_stride,
                           const void *d_dbsnp, uint32_t n, void *d_out, uint64_t out_cap, void *d_count, void *stream);

/*
 * One block from reads to written records, nothing else crossing PCIe on the way back: what call_genotypes_ML hands to
 * the calc threads (src/call_genotypes.c:180-226 -> :260-272) and the print thread makes of their output
 * (src/process.c:87-104 -> src/print_vcf.c:32-594), on the reads-in chain (bsc_reads_chain_device: neither the pile-up nor
 * gt_meth in HBM), then the packing — every launch and copy queued back to back, ONE wait for the templates' verdict, the
 * record count and the records together.  ref[y - x + 3] = reference codes of x .. y + 2 (work->ref1 as the reference fills
 * it, src/process_template.c:29-30); dbsnp = rs_found per position or NULL; with_stats != 0: the site statistics too.
 * out[out_cap]: pinned or pageable; *n_out = records written.  BSC_ERR_ARG if out_cap is too small (*n_out then holds
 * the number needed) or a template breaks one of the reference's asserts (the contents of out are then unspecified);
 * BSC_WARN_INEXACT as bsc_accumulate.
 * The reference aborts on such a template (asserts enabled in release builds, src/call_genotypes.c:186-188); here the block is
 * queued before its verdict is known (one wait per block), so when BSC_ERR_ARG names a template the context's site statistics,
 * CpG carry and position counters already hold what the block's other reads gave: they are undefined from there on — a
 * caller that goes on after the error calls bsc_reset_site_stats() (and bsc_reset_stats()) first.
 * One block in flight per context across ALL host-buffer block entries (bsc_accumulate, bsc_call_block, bsc_block_submit[_to],
 * bsc_block_records[_submit[_inplace]]): they share the staging area, the device workspaces and the verdict counters, and
 * each refuses with BSC_ERR_ARG while a submitted block has not been fetched.
 *
 * bsc_block_records_submit / _fetch: the same split where the reference splits it — submit returns once the block is queued,
 * as call_genotypes_ML returns once its calc threads are dispatched (src/call_genotypes.c:260-272), its inputs copied to a
 * pinned staging area (the caller's buffers are free at once); fetch is the wait at the top of the next call (:161-168) and
 * completes the block into the `out` named at submit (which must stay valid until then).  One block in flight per context.
 * bsc_block_records_submit_inplace: no staging copy — the inputs are read where they lie (page-locked buffers from
 * bsc_alloc_host make the upload a true DMA) and must stay unchanged until the fetch, as the reference's align_list stays
 * untouched until the next hand-off (src/process.c:61,68).  A host that flattens block k + 1 into a second set of buffers
 * while block k is in flight on another context keeps both PCIe directions busy (tools/bench_two_contexts.py).
 */
int bsc_block_records(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                      uint32_t x, uint32_t y, const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params,
                      int with_stats, bsc_vcf_rec *out, uint64_t out_cap, uint64_t *n_out);

int bsc_block_records_submit(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x,
                             uint32_t y, const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats,
                             bsc_vcf_rec *out, uint64_t out_cap);
int bsc_block_records_submit_inplace(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                                     uint32_t x, uint32_t y, const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params,
                                     int with_stats, bsc_vcf_rec *out, uint64_t out_cap);
int bsc_block_records_fetch(bsc_context *ctx, uint64_t *n_out);

/*
 * Several blocks in ONE launch sequence.  The reference calls call_genotypes_ML once per maximal run of overlapping templates
 * (src/get_template_vector.c:141-147: 10^2 .. 10^7 positions a call) and its calc threads cost nothing to start; a GPU block
 * costs a dozen launches, four copies and a wait whatever its size, which a 10 000-position block does not repay.  A host that
 * holds blocks back (integration/call_genotypes_amd_overlap.c: until 1 M positions or 65 536 blocks are pending, or the run ends;
 * a batch may mix contigs — every block carries its own)
 * hands them over together: one upload, one grouping pass over all their reads, the reads-in chain over all their tiles, one
 * packing pass, one copy-out, one wait.  Every block is still a block of its own — its printer state flushed at its end
 * (src/print_vcf.c:529-546), its first two and last two positions without the neighbours' context — so the records and the
 * statistics are those of bsc_block_records called on the blocks one after another, in order.
 *   blocks[n_blocks]  x .. y and the number of templates of every block, in the order their records are wanted (genome order
 *                     on one contig: the CpG pairing across blocks, src/print_vcf.c:447-455, follows this order)
 *   tpl, seq          the templates of all blocks, block after block (off[] index the one read buffer `seq`)
 *   ref               the blocks' reference codes one block after another: y - x + 3 codes each (x .. y + 2)
 *   dbsnp             NULL, or rs_found per position, block after block (y - x + 1 each)
 *   out[out_cap]      the written records of all blocks, block after block; block_counts[n_blocks] (optional) = how many each
 *                     block wrote
 * At most 2^28 - 1 positions (each block rounded up to a multiple of 64) and 65 536 blocks a call.  Errors as
 * bsc_block_records (a bad template is named by its index among the call's templates); one call in flight per context,
 * shared with the single-block entries.  bsc_blocks_records_submit copies the inputs to the pinned staging area: the caller's
 * buffers are free when it returns; `out` must stay valid until the fetch.
 */
typedef struct {
  uint32_t x, y; /* first and last position of the block */
  uint32_t nr;   /* its templates: the next nr of tpl[] */
  uint32_t _pad;
} bsc_block_desc;
int bsc_blocks_records_submit(bsc_context *ctx, const bsc_block_desc *blocks, uint32_t n_blocks, const bsc_template *tpl,
                              const uint8_t *seq, uint64_t seq_bytes, const uint8_t *ref, const uint8_t *dbsnp,
                              const bsc_vcf_params *params, int with_stats, bsc_vcf_rec *out, uint64_t out_cap);
/* no staging copy of templates, reads and reference codes: read where they lie (page-locked buffers from bsc_alloc_host make the
 * upload a true DMA), unchanged until the fetch — the form for a host that flattens its blocks straight into such buffers */
int bsc_blocks_records_submit_inplace(bsc_context *ctx, const bsc_block_desc *blocks, uint32_t n_blocks, const bsc_template *tpl,
                                      const uint8_t *seq, uint64_t seq_bytes, const uint8_t *ref, const uint8_t *dbsnp,
                                      const bsc_vcf_params *params, int with_stats, bsc_vcf_rec *out, uint64_t out_cap);
int bsc_blocks_records_fetch(bsc_context *ctx, uint64_t *n_out, uint64_t *block_counts);
int bsc_blocks_records(bsc_context *ctx, const bsc_block_desc *blocks, uint32_t n_blocks, const bsc_template *tpl, const uint8_t *seq,
                       uint64_t seq_bytes, const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats,
                       bsc_vcf_rec *out, uint64_t out_cap, uint64_t *n_out, uint64_t *block_counts);

/*
 * The gt_meth / gt_vcf form: bsc_block_submit_to for several blocks in ONE launch sequence — same block list, same joined
 * template / read / reference arrays (ref: y - x + 3 codes per block, of which the first y - x + 1 are used).  One upload, one
 * grouping pass over all the blocks' reads, one accumulate launch and one launch of the calling kernel over all positions, one
 * copy-out.  In `out` (page-locked; out_stride = 200 or 208) and `skip` every block starts on a multiple of 64 positions:
 * block b's images from image block_off[b] on (returned; each block takes its positions rounded up to 64, and out / skip
 * must hold the sum); the positions in between are images of nothing (skip = 1).  bsc_block_fetch(ctx, NULL, NULL) completes it;
 * counters and errors as for one block (a bad template is named by its index among the call's templates).  The drop-in glue
 * (integration/amd_overlap_protocol.h) holds small blocks back and hands them over through this entry.
 */
int bsc_blocks_submit_to(bsc_context *ctx, const bsc_block_desc *blocks, uint32_t n_blocks, const bsc_template *tpl, const uint8_t *seq,
                         uint64_t seq_bytes, const uint8_t *ref, void *out, uint32_t out_stride, uint8_t *skip, uint64_t *block_off);
/* The same without the staging copy (round 5): templates, reads and reference codes are uploaded from where they lie — page-locked
 * buffers from bsc_alloc_host make that a true DMA — and must stay unchanged until bsc_block_fetch, as the reference's align_list
 * stays untouched until the next hand-off (src/process.c:61,68).  The form for a host that builds its batch straight in such
 * buffers (integration/amd_overlap_protocol.h since round 5): the staged form from ordinary memory runs at a third of its rate
 * (profiles/r05_small_blocks.txt). */
int bsc_blocks_submit_to_inplace(bsc_context *ctx, const bsc_block_desc *blocks, uint32_t n_blocks, const bsc_template *tpl,
                                 const uint8_t *seq, uint64_t seq_bytes, const uint8_t *ref, void *out, uint32_t out_stride, uint8_t *skip,
                                 uint64_t *block_off);

/* bsc_vcf_format for a packed record. */
int bsc_vcf_format_rec(const bsc_vcf_rec *r, const char *contig, const char *id, char *buf, size_t cap);

/*
 * One written record as a BCF2 record (host C; csrc/bcf.c): the bytes bcf_write() emits for the record the reference
 * assembles with htslib's typed-value encoders (src/print_vcf.c:160-222, :267-378) — 32 bytes of fixed fields, the shared
 * block (ID, REF, ALT, FILTER, INFO CX) and the per-sample block (GT FT DP MQ GQ QD GL MC8 [AMQ] CS CG CX [FS]).
 * `ids` = the header dictionary indices of the keys (bsc_bcf_default_ids: the header print_vcf_header writes,
 * src/print_vcf.c:712-731); rid = the contig's index among the header's ##contig lines; id / id_len = the dbSNP name as
 * bsc_dbsnp_name returns it (id_len 0: no ID).  Returns the record's length (> cap: buf too small, nothing usable
 * written), 0 for a record that is not written (emit == 0), -1 on a bad argument.  The typed-value rules are the BCF2
 * specification's; byte parity with htslib itself is not pinned in this image.
 */
typedef struct {
  int32_t pass, fail, mac1, info_cx;
  int32_t fmt_gt, fmt_ft, fmt_gl, fmt_gq, fmt_dp, fmt_mq, fmt_qd, fmt_mc8, fmt_amq, fmt_cs, fmt_cg, fmt_cx, fmt_fs;
} bsc_bcf_ids;
void bsc_bcf_default_ids(bsc_bcf_ids *ids);
long bsc_bcf_record(const bsc_vcf_rec *r, int32_t rid, const char *id, size_t id_len, const bsc_bcf_ids *ids, uint8_t *buf,
                    size_t cap);
/* The written records of a block one after the other, named from the dbSNP index where rs_found is set (db may be NULL);
 * stops in front of the first record that does not fit: *n_done = records consumed.  Returns the bytes written. */
struct bsc_dbsnp;
long bsc_bcf_block(const bsc_vcf_rec *recs, uint64_t n, int32_t rid, const bsc_bcf_ids *ids, const struct bsc_dbsnp *db, uint8_t *buf,
                   size_t cap, uint64_t *n_done);

/*
 * Site statistics: the sums the reference's printer adds to bs_stats for every position that reaches
 * _print_vcf_entry (src/print_vcf.c:382-526; types include/bs_call.h:75-95,120-146) — the payload of the one
 * collective of a sharded run (every field is a sum, so shards add).  Computed on the device
 * from the bsc_vcf_core records of a block and the gt_meth records they were made from, accumulated in the context.
 * Faithful to the reference including its quirks: by the time the statistics are taken `alt` has been walked to its
 * terminator (:177-181), so every written record counts as a SNP (`alt[0] != '.'`, `alt[1] != ','`) and none as
 * multi-allelic; a CpG is counted when a '-' strand call directly follows a '+' strand call (prev_cpg_x, which
 * persists from block to block — pass the blocks of a contig in order).  Not covered: the per-coverage GC
 * histogram (gt_cov_stats.gc_pcent needs the reference's GC bins), indels (the path calls none), the coverage
 * table beyond BSC_COV_CAP - 1 (deeper positions share the last row), negative FS values (the reference indexes
 * its fs_stats vector with them: undefined behaviour there, ignored here).
 * Integer fields are exact; the methylation profiles are sums of doubles whose order differs from the reference's
 * position order (relative differences ~1e-15).
 */
#define BSC_COV_CAP 4096
typedef struct {
  uint64_t snps[2], indels[2], multi[2], dbSNP_sites[2], dbSNP_var[2], CpG_ref[2], CpG_nonref[2]; /* [all, passed] */
  uint64_t mut_counts[12][2], dbSNP_mut_counts[12][2]; /* stats_mut order AC AG AT CA CG CT GA GC GT TA TC TG */
  uint64_t qual[4][256];          /* qual_cat: all sites, variant sites, CpG ref, CpG non-ref; index = phred */
  uint64_t filter_counts[2][32];  /* [het genotype][flt & 31] */
  uint64_t qd_stats[256][2], fs_stats[256][2], mq_stats[256][2]; /* index = QD / FS / MQ value; [hom, het] */
  uint64_t cov[BSC_COV_CAP][6];   /* gt_cov_stats by coverage: all, var, CpG[2] (index = total depth), CpG_inf[2]
                                     (index = informative depth) */
  double CpG_ref_meth[2][101], CpG_nonref_meth[2][101]; /* [all, passed][methylation %] */
} bsc_site_stats;

/* Adds the statistics of n positions to the context's block: d_core[n] = the bsc_vcf_core records of the block (as
 * written by bsc_vcf_records_device), d_gtm the gt_meth records they came from, d_dbsnp = rs_found per position or
 * NULL.  Asynchronous on `stream`. */
int bsc_vcf_stats_device(bsc_context *ctx, const void *d_core, const void *d_gtm, uint32_t gtm_stride,
                         const void *d_dbsnp, uint32_t n, void *stream);
/* Host-buffer form (copies in, runs, returns when done). */
int bsc_vcf_stats(bsc_context *ctx, const bsc_vcf_core *core, const void *gtm, uint32_t gtm_stride, const uint8_t *dbsnp,
                  uint32_t n);
/* Device -> host (synchronises the device first) / back to zero, the CpG carry included. */
int bsc_get_site_stats(bsc_context *ctx, bsc_site_stats *out);
int bsc_reset_site_stats(bsc_context *ctx);

/*
 * GC content by coverage (gt_cov_stats.gc_pcent, src/print_vcf.c:394-398; the report's "GC" object): with the bins of the
 * contig being walked set, every bsc_chain_device(with_stats) call also adds its positions that reached the printer to
 * table[total depth][G+C count of the position's 100-base bin].  The bins are the reference's ctg_stats->gc
 * (src/read_reference.c:44-131): bsc_gc_bins computes them on the host from the contig's reference codes.
 *   bsc_set_gc_bins   d_gc[n_bins] in device memory (the caller keeps it alive while set), start_pos = the contig's first
 *                     A/C/G/T position; d_gc NULL switches the table off.  Call at every contig change.
 *   bsc_get_gc_stats  out[BSC_COV_CAP][101] (synchronises the device); zeroed by bsc_reset_site_stats.
 * bsc_vcf_stats_device / bsc_vcf_stats / bsc_block_records(with_stats) feed the same table (depth = the sum of the gt_meth counts).
 */
int bsc_gc_bins(const uint8_t *codes, uint64_t n, uint32_t *start_pos, uint8_t *out, uint64_t out_cap, uint64_t *n_bins);
int bsc_set_gc_bins(bsc_context *ctx, const void *d_gc, uint32_t n_bins, uint32_t start_pos);
/* the same from host memory: the context keeps its own device copy (synchronises the device) */
int bsc_set_gc_bins_host(bsc_context *ctx, const uint8_t *gc, uint32_t n_bins, uint32_t start_pos);
int bsc_get_gc_stats(bsc_context *ctx, uint64_t *out);

/* The first 14 words of the statistics block — snps, indels, multi, dbSNP_sites, dbSNP_var, CpG_ref, CpG_nonref, each
 * [all, passed] — as they stand now (synchronises the device).  The reference keeps a copy of these seven pairs per contig
 * (gt_ctg_stats, include/bs_call.h:124-135): a caller that walks contig after contig takes the difference of two reads. */
int bsc_get_site_totals(bsc_context *ctx, uint64_t out[14]);

/*
 * The JSON report of a run (host C; csrc/report.c): the text output_stats() writes at the end of a run
 * (src/stats.c:19-298), byte for byte, from the statistics this library accumulates and the counters of the stages in
 * front of it.  bsc_report_json returns the length of the full text (like snprintf: a return >= cap means buf was too
 * small; call with cap = 0 to size it), -1 on a NULL argument.
 */
typedef struct { /* gt_ctg_stats (include/bs_call.h:124-135) without the GC bins */
  const char *name;
  uint64_t snps[2], indels[2], multi[2], dbSNP_sites[2], dbSNP_var[2], CpG_ref[2], CpG_nonref[2];
} bsc_contig_totals;
typedef struct {
  double under_conv, over_conv;  /* the "source" line (src/stats.c:29) */
  int32_t mapq_thresh, min_qual;
  int32_t day, month, year;      /* the "date" line; year 0 = today (local time, as the reference) */
  int32_t have_dbsnp;            /* a dbSNP index was loaded: the dbSNP totals are reported */
  uint64_t filter_cts[15], filter_bases[15]; /* reads / bases by the reader's verdict, gt_filter_reason order
                                                (include/bs_call.h:50; [14] = "PairNotFound"); [0] = passed */
  uint64_t base_filter[5];       /* base_filter_types order: passed, trimmed, clipped, overlapping, low quality */
  const bsc_site_stats *total;
  const uint64_t *gc;            /* [BSC_COV_CAP][101]: positions by coverage and GC percent of their 100-base bin
                                    (gt_cov_stats.gc_pcent), or NULL = all zero */
  const uint64_t *read_profile;  /* [n_read_profile][4]: bs_stats.meth_profile, element 0 included (never reported) */
  uint32_t n_read_profile;
  uint32_t n_contigs;
  const bsc_contig_totals *contigs;
} bsc_report;
long bsc_report_json(const bsc_report *r, char *buf, size_t cap);

/*
 * The fused chain — pile-up -> call -> VCF record -> site statistics in ONE pass, the 200-byte gt_meth records never
 * reaching HBM: what the print thread consumes from a block (src/process.c:87-104 feeding src/print_vcf.c:32-594),
 * computed from what the process thread produces (src/call_genotypes.c:178-226).  Same bytes as
 * bsc_call_sites_device -> bsc_vcf_records_device (-> bsc_vcf_stats_device) over the whole block.
 *
 * A call handles one WINDOW of a block (the reference's unit: x .. y of one call_genotypes_ML, whose printer state is
 * flushed at its end), so that a long block — a whole contig — can be walked in fixed windows with HBM-resident
 * inputs; the windows of a block, passed in order, give exactly the block's records and statistics.  The printer's
 * record of a position looks at the called genotypes of 2 positions and the reference bases of up to 4 / 2 positions
 * either side, so the window's buffers carry that much context where the block has it:
 *   d_cts    pile-ups of block positions first - lc .. first + n + rc - 1, lc = min(2, first),
 *            rc = min(2, n_block - first - n)                                   [(lc + n + rc) x 104 bytes]
 *   d_ref    reference codes of block positions first - lr .. first + n + 1, lr = min(4, first)  (a block's
 *            reference has n_block + 2 codes: x .. y + 2, src/process_template.c:29-30)
 *   d_dbsnp  rs_found (0/1/3) of block positions first .. first + n - 1, or NULL
 *   d_core   n bsc_vcf_core records (16-byte aligned)
 * Asynchronous on `stream`; counters (bsc_get_stats) and, with_stats != 0, the site statistics accumulate in the context.
 */
typedef struct {
  uint32_t x;       /* genome position (1-based) of the block's first position */
  uint32_t n_block; /* positions in the block (y - x + 1) */
  uint32_t first;   /* block-relative index of the window's first position */
  uint32_t n;       /* positions in the window */
} bsc_window;
int bsc_chain_device(bsc_context *ctx, const void *d_cts, const void *d_ref, const void *d_dbsnp, const bsc_window *w,
                     const bsc_vcf_params *params, int with_stats, void *d_core, void *stream);
/*
 * bsc_reads_chain_device: one whole block from reads to records in the chain's single pass — the block's templates are
 * checked, described and ordered like bsc_accumulate_device's, then every 60-position tile is piled up in the LDS of the
 * wave that calls it: HOT LOOP A (src/call_genotypes.c:180-226), the calc threads (:43-115) and what the print thread
 * derives from their output (src/process.c:87-104 -> src/print_vcf.c:32-594) with neither the pile-up nor gt_meth in HBM.
 *   d_tpl[nr], d_seq   device-resident templates (8-byte aligned) and read bytes of the block x .. y
 *   d_ref              reference codes of x .. y + 2 (y - x + 3 bytes: work->ref1, src/process_template.c:29-30)
 *   d_dbsnp            rs_found per position or NULL
 *   d_core             y - x + 1 bsc_vcf_core records (16-byte aligned): the bytes bsc_accumulate_device + bsc_chain_device give
 *   d_aux              NULL, or 64 bytes per position (16-byte aligned): the second half of a bsc_vcf_rec — counts[8], qual[8],
 *                      mq, aq, max_gt, rs_found — of every position with a record, zero elsewhere
 * Asynchronous on `stream`; bsc_block_status() returns the templates' verdict (an invalid template contributes nothing);
 * counters and, with_stats != 0, the site statistics accumulate in the context.  bsc_last_reads_chain_ms (with
 * bsc_set_profiling): device time of all of its launches.
 */
int bsc_reads_chain_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x,
                           uint32_t y, const void *d_ref, const void *d_dbsnp, const bsc_vcf_params *params, int with_stats,
                           void *d_core, void *d_aux, void *stream);
int bsc_last_reads_chain_ms(bsc_context *ctx, float *ms);
/* How bsc_reads_chain_device / bsc_block_records get from reads to records.  0 (default): TWO kernels — the accumulate kernel's
 * summary form leaves 48 bytes per position in HBM (per class its count and the forward-strand part of it, 16 bits each, and the
 * per-site summary of src/call_genotypes.c:44-59; the context's own workspace; a block with a position deeper than 65 535 reads
 * of one class is flagged on the device and done by the reads-in kernel queued behind as a stand-in) and the chain kernel's summary-in form starts from them: the faster form (the walk alone runs at 24
 * waves to a CU and hides its byte loads — inside the 128-register chain kernel it waits for them — and the summary's arithmetic
 * runs where there are issue slots to spare), taken whenever that workspace can be allocated.  1: always the ONE-kernel form
 * (reads-in chain: nothing per position in HBM but the records).  Same records and statistics either way.  (bsc_blocks_records
 * always runs the one-kernel form: small blocks are bound by launches and PCIe, not by the walk.)  Memory: the two-kernel form
 * keeps 48 bytes per position of the largest block seen so far in the context (grow-only; 2.4 GB for a 50 M-position block, 13 GB
 * for a maximal one of 2^28) — a context that must stay lean sets 1. */
int bsc_set_reads_fused(bsc_context *ctx, int fused);
/* Test hook (tests/test_gpu_reads_chain.py): on != 0 makes the summaries' allocation of the two-kernel form fail for real — an absurd
 * request the runtime refuses — so that the quiet fall-back to the one-kernel form can be exercised.  Off in every new context; nothing
 * in the environment switches it (the switches that are read from the environment — BSC_NO_H2D_TURNS, BSC_NO_EMIT_BYTES,
 * BSC_STAGE_TIMING, BSC_MAX_LAUNCH_SITES, BSC_NUM_CUS: A/B measurements and tests — are read ONCE, by bsc_create). */
int bsc_debug_fail_summary_alloc(bsc_context *ctx, int on);
/* Window sizes for a caller that cuts a resident contig into windows of its own choosing (the reference's blocks are data
 * dependent, src/process_template.c:24-28; SURVEY.md 8d fixes 4 Mi).  bsc_chain_window_size: the largest window <= limit in
 * which every resident wave runs the same number of tiles and the main launch covers the window exactly — CUs x waves per
 * workgroup x (60 + 62 k): the first tile of a wave's run forms 60 records, every further one 62.  bsc_chain_window_quantum:
 * the smallest such window (k = 0).  0 if ctx is NULL. */
uint32_t bsc_chain_window_size(const bsc_context *ctx, uint32_t limit);
uint32_t bsc_chain_window_quantum(const bsc_context *ctx);
/* with bsc_set_profiling: device time of the most recent bsc_chain_device call (all of its launches) */
int bsc_last_chain_ms(bsc_context *ctx, float *ms);

/*
 * Read pre-processing (host C; csrc/prep.c): from the templates the reader hands over to the templates bsc_accumulate /
 * bsc_call_block / bsc_block_records consume — what process_template_vector does to every template of a block before it
 * calls call_genotypes_ML (src/process_template.c:36-111): the fixed trims (trim_read, src/read_utils.c:13-26), the
 * soft clips (trim_soft_clips, src/al_utils.c:122-162), the overlap of the two mates (handle_overlap, :164-318) and the
 * normalisation of indels (a deletion from the reference becomes bytes 0, an insertion is removed).
 *
 * A raw template is `align_details` (include/bs_call.h:64-73) with its gt_vectors flattened: read k = len[k] bytes
 * base|qual<<2 at seq + off[k]; its mismatch list = n_misms[k] entries at misms + misms_off[k], as get_bam_misms builds
 * it from the CIGAR (src/input_sam.c:90-136; note the reference's naming: CIGAR D -> INS, CIGAR I -> DEL).
 */
#define BSC_MISMS_MISMS 0u /* gt_misms_t, include/bs_call.h:54 */
#define BSC_MISMS_INS 1u
#define BSC_MISMS_DEL 2u
#define BSC_MISMS_SOFT 3u
typedef struct {
  uint32_t type;     /* BSC_MISMS_* */
  uint32_t position; /* offset in the read */
  uint32_t size;
} bsc_misms; /* gt_misms, include/bs_call.h:55-62 */
typedef struct {
  uint32_t pos[2];            /* forward_position, reverse_position; 0 = none */
  uint32_t reference_span[2];
  uint32_t len[2];            /* 0 = read absent */
  uint32_t n_misms[2];
  uint64_t off[2];            /* byte offsets of the reads in seq */
  uint64_t misms_off[2];      /* index of each read's first entry in misms */
  uint8_t mapq[2];
  uint8_t orientation;        /* gt_strand: 0 FORWARD, 1 REVERSE */
  uint8_t bs_strand;          /* gt_bs_strand */
  uint32_t _pad;
} bsc_raw_template;
typedef struct {
  int32_t left_trim[2], right_trim[2]; /* sr_param.left_trim / right_trim: [0] read 1, [1] read 2 (-L / -R) */
  int32_t min_qual;                    /* only for the base counters below */
} bsc_prep_params;
typedef struct { /* the base_filter / filter_cts counters of bs_stats this stage feeds (src/process_template.c:50-59) */
  uint64_t base_none, base_trim, base_clip, base_overlap, base_lowqual; /* base_filter[] */
  uint64_t reads, read_bases;                                           /* filter_cts / filter_bases[gt_flt_none] */
} bsc_prep_stats;
/* tpl_out[nr] and the prepared read bytes in seq_out (capacity seq_out_cap: the input bytes plus the padded deletions
 * always fit in seq_bytes + sum of INS sizes); *seq_out_used = bytes written.  BSC_ERR_ARG where the reference aborts
 * (a soft clip that is not at the end of its read or swallows it), naming the template. */
int bsc_prepare_templates(const bsc_raw_template *raw, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                          const bsc_misms *misms, uint64_t n_misms, const bsc_prep_params *par, bsc_template *tpl_out,
                          uint8_t *seq_out, uint64_t seq_out_cap, uint64_t *seq_out_used, bsc_prep_stats *stats);
/* The same, and the non-CpG read profile of the templates (meth_profile, src/meth_profile.c:48-77: by position in the
 * original read, C / G of the reference outside a CpG seen converted or not — bs_stats.meth_profile, the report's
 * "NonCpGreadProfile").  ref = reference codes 0..4 of genome positions x .. x + n_ref - 1, covering every template
 * and one base either side (the block's work->ref1: x .. y + 2); counts[cap][4] and used persist from call to call
 * (used = the reference vector's length: elements 1 .. used - 1 are reported, element i + 1 = read position i). */
typedef struct {
  const uint8_t *ref;
  uint32_t x, n_ref;
  uint64_t *counts;
  uint32_t cap, used;
} bsc_read_profile;
int bsc_prepare_templates_profile(const bsc_raw_template *raw, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                                  const bsc_misms *misms, uint64_t n_misms, const bsc_prep_params *par, bsc_template *tpl_out,
                                  uint8_t *seq_out, uint64_t seq_out_cap, uint64_t *seq_out_used, bsc_prep_stats *stats,
                                  bsc_read_profile *profile);
/*
 * bsc_prepare_templates ON THE DEVICE (round 5; csrc/prepdev.hip): the same bytes — prepared templates incl. their flags, prepared
 * reads in template order, the statistics — from device-resident inputs into device-resident outputs, ready for
 * bsc_accumulate_device / bsc_reads_chain_device without a host pass: one thread per template plans the trims, clips, the mate
 * overlap and the indel normalisation on the mismatch lists alone, a prefix sum places the reads, a wave per 64 reads writes
 * them (a dword per lane).  d_raw (bsc_raw_template[nr], 8-byte aligned), d_seq, d_misms (bsc_misms[n_misms]); d_tpl_out (bsc_template[nr]) and
 * d_seq_out (seq_out_cap bytes: seq_bytes + the sizes of all BSC_MISMS_INS entries always suffice).  Queued on `stream`, then
 * waited for: *seq_out_used, *stats (may be NULL) and the verdict come back with the call — BSC_ERR_ARG where the host form
 * fails, naming the lowest offending template with the host form's own message.  Workspaces (88 bytes per read + the lists)
 * stay with the context.  profile (may be NULL): the non-CpG read profile as bsc_prepare_templates_profile makes it — here
 * profile->ref is a DEVICE pointer to the codes of x .. x + n_ref - 1, counts / cap / used are the host's (counts[cap][4] receives
 * this call's counts, used grows, with the host form's clearing of what lies behind the old end).
 */
int bsc_prepare_templates_device(bsc_context *ctx, const void *d_raw, uint32_t nr, const void *d_seq, uint64_t seq_bytes,
                                 const void *d_misms, uint64_t n_misms, const bsc_prep_params *par, void *d_tpl_out, void *d_seq_out,
                                 uint64_t seq_out_cap, uint64_t *seq_out_used, bsc_prep_stats *stats, bsc_read_profile *profile,
                                 void *stream);
/*
 * bsc_block_records from what the READER delivers (bsc_read_block: raw templates, their reads and mismatch lists, host buffers):
 * uploaded as they are, prepared on the device, then grouped, walked and called like bsc_block_records — the process thread's
 * per-template work (src/process_template.c:36-111) on no host core.  x .. y = the block as the reader found it (x =
 * bsc_block_start(raw), y = bsc_read_block.y); ref = the codes of x .. y + 2.  prep_stats (may be NULL) = the base counters the
 * pre-processing feeds; profile (may be NULL) = the read profile, counts / cap / used as in bsc_read_profile (ref, x, n_ref are
 * taken from the block).  Same records as bsc_prepare_templates[_profile] + bsc_block_records; two host waits (the prepared
 * size, the records) instead of one.
 */
int bsc_block_records_raw(bsc_context *ctx, const bsc_raw_template *raw, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes,
                          const bsc_misms *misms, uint64_t n_misms, const bsc_prep_params *prep, uint32_t x, uint32_t y, const uint8_t *ref,
                          const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats, bsc_vcf_rec *out, uint64_t out_cap,
                          uint64_t *n_out, bsc_prep_stats *prep_stats, bsc_read_profile *profile);
/*
 * The BCF stream of a block, encoded ON THE DEVICE (round 5, csrc/bcfdev.hip): what the output thread hands to bcf_write for the block's
 * written records — the typed values of src/print_vcf.c:160-222,267-378 behind bcf_write's fixed fields, byte for byte what
 * bsc_bcf_block (host C, the checker) makes of the same packed records — so that the record formation's tail never touches a host core
 * and ~113 bytes per written record cross PCIe instead of 128.
 *   bsc_bcf_names            the dbSNP names of the block's flagged positions (host arrays; the block entries — bsc_block_bcf*, the split
 *                            forms included — copy them into a page-locked area of the context's and upload them with the block's other
 *                            inputs, ahead of its kernels: the arrays are the caller's again when the call returns; the device-level
 *                            entries bsc_bcf_block_device / bsc_bcf_sites[_len]_device queue the upload from the caller's arrays on the
 *                            caller's stream: keep them unchanged until that stream has passed the call, page-locked for a true DMA):
 *                            pos[n] ascending
 *                            1-based positions, off[n + 1] offsets into bytes; bsc_dbsnp_names fills one from the loaded contig.  A
 *                            record whose rs_found flag is set and whose position the table lists carries that ID (at most 63 bytes of it)
 *   bsc_bcf_block_device     d_recs[<= max_recs] packed records in HBM, *d_n_recs of them (a device u64: the count bsc_vcf_compact_device
 *                            left) -> d_out[<= out_cap] bytes; d_totals = three device u64 {length of the stream, records bsc_bcf_record
 *                            refuses (gt > 9 or n_gl > 6: counted, written with the values clamped), records written}; a stream longer
 *                            than out_cap is cut at a 64-record boundary, its full length still in d_totals[0].  Asynchronous on `stream`.
 *                            d_out must be 16-byte aligned (BSC_ERR_ARG otherwise): the write kernel owns whole 16-byte pieces of the stream
 *   bsc_bcf_sites_device     the same from the per-position arrays bsc_reads_chain_device leaves — d_core[n] and d_aux[n] (64 bytes each
 *                            per position, 16-byte aligned) — with no packing pass in between: a position without a record costs 16 bytes
 *   bsc_block_bcf[_raw]      bsc_block_records[_raw] with the encoder in the packing's place: out[out_cap] receives the block's BCF bytes,
 *                            *n_bytes their number (BSC_ERR_ARG and the number needed when out_cap is too small), *n_records the records
 *                            in them; one wait per block as before
 */
typedef struct {
  const uint32_t *pos;
  const uint32_t *off;
  const char *bytes;
  uint32_t n;
} bsc_bcf_names;
/* the names of the flagged positions of x0 .. x0 + n - 1 of the loaded contig, as bsc_dbsnp_name returns them (length = *rs_len);
 * pos / off / bytes may be NULL to ask for the sizes: *n_names entries, *n_bytes bytes.  BSC_ERR_ARG if a capacity is too small. */
int bsc_dbsnp_names(const struct bsc_dbsnp *db, uint32_t x0, uint32_t n, uint32_t *pos, uint32_t *off, char *bytes, uint32_t cap_names,
                    uint64_t cap_bytes, uint32_t *n_names, uint64_t *n_bytes);
int bsc_bcf_block_device(bsc_context *ctx, const void *d_recs, const void *d_n_recs, uint64_t max_recs, int32_t rid, const bsc_bcf_ids *ids,
                         const bsc_bcf_names *names, void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_bcf_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, int32_t rid, const bsc_bcf_ids *ids,
                         const bsc_bcf_names *names, void *d_out, uint64_t out_cap, void *d_totals, void *stream);
/* Round 6: the chain kernel leaves every written record's BCF2 LENGTH in a byte per position (0: no record; 255: heterozygous, dbSNP-flagged or
 * longer than 254 bytes — ask the record), so that the encoder's size pass reads a byte per position and the records are read once, by the
 * write kernel (the block entries above do this between themselves).  d_len: y - x + 1 bytes, zeroed by the chain's call. */
int bsc_reads_chain_len_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x, uint32_t y,
                               const void *d_ref, const void *d_dbsnp, const bsc_vcf_params *params, int with_stats, void *d_core, void *d_aux,
                               void *d_len, void *stream);
int bsc_bcf_sites_len_device(bsc_context *ctx, const void *d_core, const void *d_aux, const void *d_len, uint32_t n, int32_t rid, const bsc_bcf_ids *ids,
                             const bsc_bcf_names *names, void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_block_bcf(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y,
                  const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats, int32_t rid, const bsc_bcf_ids *ids,
                  const bsc_bcf_names *names, uint8_t *out, uint64_t out_cap, uint64_t *n_bytes, uint64_t *n_records);
/* the split form (as bsc_block_records_submit / _submit_inplace / _fetch; one block in flight per context): queue and return, then wait.
 * _submit copies the inputs into the context's staging area (the caller's buffers are free at once); _submit_inplace reads them where
 * they lie (page-locked buffers: a true DMA) and they must stay unchanged until the fetch */
int bsc_block_bcf_submit(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y,
                         const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats, int32_t rid, const bsc_bcf_ids *ids,
                         const bsc_bcf_names *names, uint8_t *out, uint64_t out_cap);
int bsc_block_bcf_submit_inplace(bsc_context *ctx, const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x,
                                 uint32_t y, const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats, int32_t rid,
                                 const bsc_bcf_ids *ids, const bsc_bcf_names *names, uint8_t *out, uint64_t out_cap);
int bsc_block_bcf_fetch(bsc_context *ctx, uint64_t *n_bytes, uint64_t *n_records);
/* SEVERAL blocks in one launch sequence, their BCF bytes back as ONE stream (round 6; bsc_blocks_records' block list and joined arrays, see
 * there): the records of the blocks in the blocks' order — what bsc_block_bcf gives block after block, concatenated — for a caller whose blocks
 * are small (the reference's unit is a run of overlapping templates, 10^2 .. 10^7 positions; a launch sequence costs ~0.2 ms whatever its size).
 * The blocks lie on ONE contig (rid) in genome order; `names` lists the flagged positions of all of them.  _submit stages the inputs (the
 * caller's buffers are free on return), _submit_inplace reads them where they lie (page-locked: bsc_alloc_host) until the fetch; one submission in
 * flight per context.  A stream longer than out_cap: BSC_ERR_ARG with *n_bytes = the room needed, then bsc_block_bcf_again. */
int bsc_blocks_bcf_submit(bsc_context *ctx, const bsc_block_desc *blocks, uint32_t n_blocks, const bsc_template *tpl, const uint8_t *seq,
                          uint64_t seq_bytes, const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats, int32_t rid,
                          const bsc_bcf_ids *ids, const bsc_bcf_names *names, uint8_t *out, uint64_t out_cap);
int bsc_blocks_bcf_submit_inplace(bsc_context *ctx, const bsc_block_desc *blocks, uint32_t n_blocks, const bsc_template *tpl, const uint8_t *seq,
                                  uint64_t seq_bytes, const uint8_t *ref, const uint8_t *dbsnp, const bsc_vcf_params *params, int with_stats,
                                  int32_t rid, const bsc_bcf_ids *ids, const bsc_bcf_names *names, uint8_t *out, uint64_t out_cap);
int bsc_blocks_bcf_fetch(bsc_context *ctx, uint64_t *n_bytes, uint64_t *n_records);
/* After a BCF block entry (bsc_block_bcf, _raw, _rawdev[_keep], bsc_block_bcf_fetch) has answered BSC_ERR_ARG with *n_bytes > out_cap — the
 * block's stream is longer than the room given — and before anything else is asked of the context: the ENCODER alone once more, from the
 * per-position arrays the block left in HBM, into out[out_cap] (out == NULL: the stream stays on the device, bsc_bcf_stream_read, out_cap
 * its room there).  Nothing of the block is computed, counted (bsc_get_stats, the site statistics, the read profile) or uploaded a second
 * time; the status the refused call would have returned (BSC_OK / BSC_WARN_INEXACT) comes back. */
int bsc_block_bcf_again(bsc_context *ctx, uint8_t *out, uint64_t out_cap, uint64_t *n_bytes, uint64_t *n_records);
/* A stream left on the device (bsc_block_bcf_rawdev_keep) handed over to the caller, so that it can be read out and written WHILE the context
 * calls the next block: _detach (on the thread that drives the context, after the _keep call has returned) gives the buffer and its length
 * and the context forgets it; _read queues a copy of bytes [off, off + n) to dst (page-locked for a true DMA) on a stream of the context's
 * that nothing else uses, _wait waits for the copies queued so far, _free gives the buffer back — to a small pool the next blocks take
 * their buffers from, so a run in its steady state neither allocates nor frees device memory (both are device-wide waits).  _read / _wait /
 * _free may be called from ONE other thread, concurrently with the driving thread's calls; at most four streams out at a time are pooled. */
int bsc_bcf_stream_detach(bsc_context *ctx, void **d_stream, uint64_t *n_bytes);
int bsc_detached_read(bsc_context *ctx, const void *d_stream, uint64_t off, uint64_t n, void *dst);
int bsc_detached_wait(bsc_context *ctx);
int bsc_detached_free(bsc_context *ctx, void *d_stream);
int bsc_block_bcf_raw(bsc_context *ctx, const bsc_raw_template *raw, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, const bsc_misms *misms,
                      uint64_t n_misms, const bsc_prep_params *prep, uint32_t x, uint32_t y, const uint8_t *ref, const uint8_t *dbsnp,
                      const bsc_vcf_params *params, int with_stats, int32_t rid, const bsc_bcf_ids *ids, const bsc_bcf_names *names, uint8_t *out,
                      uint64_t out_cap, uint64_t *n_bytes, uint64_t *n_records, bsc_prep_stats *prep_stats, bsc_read_profile *profile);
/* x of the block a template list starts: the first template's start - 2, at least 1 (src/process_template.c:22-28) */
uint32_t bsc_block_start(const bsc_raw_template *first);
/* get_al_qual (src/al_utils.c:19-35): the score duplicate resolution compares, with the reference's sq[k] indexing */
uint32_t bsc_template_qual(const bsc_raw_template *t, const uint8_t *seq);

/*
 * The reference sequence of a block (host C + zlib; csrc/refseq.c).
 *   bsc_fasta_contig     one contig of a FASTA file (plain / gzip / bgzip, read sequentially) as reference codes 0 = N,
 *                        1..4 = ACGT, position 1 first: load_sequence (src/read_reference.c:44-131).  *len = its length
 *                        (BSC_ERR_ARG with *len set when cap is too small: call again with a larger buffer).
 *   bsc_block_reference  get_sequence_string (src/get_sequence.c:20-54): out[sz] = codes of positions x .. x + sz - 1
 *                        (a block's work->ref1: sz = y - x + 3); positions at or beyond the contig's last one read 0, as
 *                        in the reference (its walk stops in front of end_pos).
 */
int bsc_fasta_contig(const char *path, const char *name, uint8_t *codes, uint64_t cap, uint64_t *len);
int bsc_block_reference(const uint8_t *codes, uint64_t contig_len, uint32_t x, uint32_t sz, uint8_t *out);

/*
 * BAM in, blocks of templates out (host C + zlib, no htslib; csrc/bamio.c): the reader thread of the reference —
 * read_input (src/get_template_vector.c:49-389) over get_next_align_details (src/input_sam.c:222-312).  A block is what
 * read_input queues for process_template_vector: the templates of one stretch of overlapping alignments of one contig
 * (mates joined, duplicates resolved), ready for bsc_prepare_templates -> bsc_accumulate / bsc_block_records, with
 * y = the rightmost covered position (x = bsc_block_start of the first template).
 *   bsc_bam_open[_threads]  a coordinate-sorted BAM or SAM file; the header text and the @SQ list are available at once
 *   bsc_bam_next_block  1 = *blk filled (valid until the next call), 0 = end of input, < 0 = error (bsc_last_error)
 *   bsc_bam_filter_counts  bs_stats.filter_cts / filter_bases as the reader leaves them: reads and bases by verdict,
 *                       gt_filter_reason order, [14] = "PairNotFound" ([0], the passed reads, is counted by
 *                       bsc_prepare_templates: bsc_prep_stats.reads / read_bases)
 * SAM text (plain or BGZF-compressed) is accepted as well: the kind is found out from the first bytes.
 * Not covered: CRAM input, seeking through a .bai index (a region is served by scanning), contig include / exclude lists.
 */
typedef struct bsc_bam bsc_bam;
typedef struct {
  uint32_t mapq_thresh;       /* sr_param.mapq_thresh (20) */
  uint64_t max_template_len;  /* sr_param.max_template_len (1000) */
  int32_t keep_unmatched, ignore_duplicates, keep_duplicates; /* -u / -d / -k */
  /* One region (the reference's -r contig:start-stop, region_t): only the alignments that overlap positions
   * region_start .. region_stop (1-based, inclusive) of contig region_tid reach the reader, as with the reference's index
   * query sam_itr_queryi(idx, tid, start - 1, stop) (src/get_template_vector.c:69-74) — found here by scanning, no index.
   * region_stop = 0: no region.  Pass the same bounds to the record formation (bsc_vcf_params.reg_start / reg_stop). */
  int32_t region_tid;
  uint32_t region_start, region_stop;
} bsc_reader_params;
typedef struct {
  int32_t tid;  /* index of the contig in the BAM header */
  uint32_t y;   /* rightmost position covered by the block's alignments */
  uint32_t nr;
  const bsc_raw_template *tpl;
  const uint8_t *seq;
  uint64_t seq_bytes;
  const bsc_misms *misms;
  uint64_t n_misms;
} bsc_read_block;
int bsc_bam_open(const char *path, bsc_bam **out); /* helper threads from the environment: BSC_BAM_THREADS (default 0) */
/* n_threads helpers (0 .. 16) inflate the BGZF blocks ahead of the parser: blocks are independent gzip members */
int bsc_bam_open_threads(const char *path, int n_threads, bsc_bam **out);
void bsc_bam_close(bsc_bam *b);
int bsc_bam_n_refs(const bsc_bam *b);
const char *bsc_bam_ref_name(const bsc_bam *b, int i);
uint32_t bsc_bam_ref_len(const bsc_bam *b, int i);
const char *bsc_bam_header_text(const bsc_bam *b);
int bsc_bam_next_block(bsc_bam *b, const bsc_reader_params *par, bsc_read_block *blk);
void bsc_bam_filter_counts(const bsc_bam *b, uint64_t cts[15], uint64_t bases[15]);
/* BAM records the reader dropped because their CIGAR does not cover l_seq query bases (htslib hands such a record over as it
 * is and the reference walks outside the read; SAM text with the same defect is an error, as in htslib's parser): not part of
 * the reference's counters — a caller should tell its user when this is not 0 (integration/bam2bcf.c does) */
uint64_t bsc_bam_malformed(const bsc_bam *b);

/*
 * The reader ON THE DEVICE (round 6; csrc/bamstream.c + csrc/bamdev.hip): the same blocks as bsc_bam_next_block, formed in HBM from the
 * inflated bytes of a BAM file — what the reference's reader thread does with a record (get_next_align_details, src/input_sam.c:222-312;
 * read_input, src/get_template_vector.c:49-389) runs as kernels, the host only inflates.
 *
 *   bsc_bamstream_*        the host half, usable on its own: the file as a stream of INFLATED bytes in page-locked slabs, with the offset
 *                          of every alignment record (hts_open + bgzf_read's inflate + the block_size chain of bam_read1).  n_threads
 *                          helpers (<= 0: one per core this process may run on, at most 64) inflate straight into the slabs;
 *                          slab_bytes / n_slabs 0 = 16 MiB x 6.  bsc_bamstream_next: 1 = *out filled (valid until it is released),
 *                          0 = end of the stream, < 0 = error.  BAM only.
 *   bsc_bamdev_open        a reader over `path` bound to ctx's device and stream
 *   bsc_bamdev_next_block  1 = *blk describes the next block, its templates / reads / lists DEVICE-resident (valid until the next call)
 *                          and laid out as bsc_prepare_templates_device / bsc_block_bcf_rawdev take them; 0 = end of input; < 0 = error.
 *                          Byte for byte the templates, reads, lists, y and filter counters of bsc_bam_next_block (tests/test_gpu_bamdev.py),
 *                          read offsets apart (a template's reads lie where their records came, block-relative).  Input the parallel
 *                          kernels are not exact for (re-used read names, unsorted records ...) goes through a one-lane replay of the
 *                          reference's loop on the device: slow, same bytes.  Divergences from csrc/bamio.c: a record of one base that a
 *                          duplicate comparison looks at reads quality 0 for the byte behind it (bamio.c reads its buffer's next byte).
 *   bsc_bamdev_fetch_block the block's arrays on the host (bsc_read_block's view)
 *   bsc_block_bcf_rawdev / bsc_block_records_rawdev    bsc_block_bcf_raw / bsc_block_records_raw from device-resident raw templates
 *                          (d_raw 8-byte, d_misms 4-byte aligned; ins_pad >= the sizes of all BSC_MISMS_INS entries: room for the
 *                          padded deletions).  ref / dbsnp / names are host arrays as before.
 */
/* csrc/inflate_fast.c: raw DEFLATE of one whole block (in -> exactly out_len bytes; 0, or -1 for an invalid stream) and zlib's CRC-32 */
int bsc_inflate_raw(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len);
uint32_t bsc_crc32(const uint8_t *p, size_t n);
typedef struct bsc_bamstream bsc_bamstream;
typedef struct {
  const uint8_t *bytes;     /* page-locked */
  uint64_t stream_off;      /* offset of bytes[0] in the inflated file */
  uint32_t n_bytes;
  const uint32_t *rec_off;  /* page-locked: where the records that START in this slab start, relative to bytes */
  uint32_t n_recs;
  int32_t last;             /* the stream ends with this slab */
  uint64_t seq;
} bsc_bam_slab;
int bsc_bamstream_open(const char *path, int n_threads, uint64_t slab_bytes, int n_slabs, bsc_bamstream **out);
/* the stream of a SELECTION of contigs (tids of the header's list; -1 = the unplaced reads at the file's end) — what the reference reads through
 * sam_index_load + sam_itr_queryi per region (src/process.c:125, src/get_template_vector.c:69-99), without an index file: the file is sorted, so a
 * binary search over its BGZF blocks (one block inflated per probe) finds the stretches that hold the selected contigs' records; records of other
 * contigs inside a stretch are for the record parser's contig filter (bsc_bamdev_open_contigs applies it).  Blocks need not start at a record
 * (htsjdk's writer cuts records where a block is full): the first record start of a probed block is found by a chain of checked record headers, a
 * stretch begins there and ends with the tail of its last record in the following block(s).  n_tids = 0: an empty stream. */
int bsc_bamstream_open_contigs(const char *path, int n_threads, uint64_t slab_bytes, int n_slabs, const int32_t *tids, int n_tids, bsc_bamstream **out);
void bsc_bamstream_close(bsc_bamstream *b);
int bsc_bamstream_next(bsc_bamstream *b, bsc_bam_slab *out);
int bsc_bamstream_release(bsc_bamstream *b, const bsc_bam_slab *slab);
int bsc_bamstream_n_refs(const bsc_bamstream *b);
const char *bsc_bamstream_ref_name(const bsc_bamstream *b, int i);
uint32_t bsc_bamstream_ref_len(const bsc_bamstream *b, int i);
const char *bsc_bamstream_header_text(const bsc_bamstream *b);
uint64_t bsc_bamstream_first_record(const bsc_bamstream *b); /* stream offset of the first alignment record */
int bsc_bamstream_threads(const bsc_bamstream *b);
int bsc_bamstream_default_threads(void);

typedef struct bsc_bamdev bsc_bamdev;
typedef struct {
  int32_t tid;
  uint32_t x, y;           /* the block as the process thread sees it: x = bsc_block_start of the first template */
  uint32_t nr;
  const void *d_tpl;       /* bsc_raw_template[nr] */
  const void *d_seq;
  uint64_t seq_bytes;
  const void *d_misms;     /* bsc_misms[n_misms] */
  uint64_t n_misms;
  uint64_t ins_pad;
} bsc_dev_read_block;
int bsc_bamdev_open(bsc_context *ctx, const char *path, int n_threads, bsc_bamdev **out);
/* the reader of a SELECTION of contigs (bsc_bamstream_open_contigs + the record parser's contig filter): what one rank of a sharded run reads —
 * its blocks and filter counters are exactly the whole file's reader's for those contigs, so the ranks' outputs concatenate and their counters add */
int bsc_bamdev_open_contigs(bsc_context *ctx, const char *path, int n_threads, const int32_t *tids, int n_tids, bsc_bamdev **out);
void bsc_bamdev_close(bsc_bamdev *r);
int bsc_bamdev_n_refs(const bsc_bamdev *r);
const char *bsc_bamdev_ref_name(const bsc_bamdev *r, int i);
uint32_t bsc_bamdev_ref_len(const bsc_bamdev *r, int i);
const char *bsc_bamdev_header_text(const bsc_bamdev *r);
int bsc_bamdev_next_block(bsc_bamdev *r, const bsc_reader_params *par, bsc_dev_read_block *blk);
int bsc_bamdev_fetch_block(bsc_bamdev *r, const bsc_dev_read_block *blk, bsc_raw_template *tpl, uint8_t *seq, bsc_misms *misms);
int bsc_bamdev_filter_counts(bsc_bamdev *r, uint64_t cts[15], uint64_t bases[15]);
uint64_t bsc_bamdev_malformed(bsc_bamdev *r);
/* counts: {device passes, passes the one-lane replay decided, records parsed, bytes uploaded}; seconds: {waiting for inflated slabs, in device passes} */
void bsc_bamdev_run_stats(const bsc_bamdev *r, uint64_t counts[4], double seconds[2]);
int bsc_block_records_rawdev(bsc_context *ctx, const void *d_raw, uint32_t nr, const void *d_seq, uint64_t seq_bytes, const void *d_misms, uint64_t n_misms,
                             uint64_t ins_pad, const bsc_prep_params *prep, uint32_t x, uint32_t y, const uint8_t *ref, const uint8_t *dbsnp,
                             const bsc_vcf_params *params, int with_stats, bsc_vcf_rec *out, uint64_t out_cap, uint64_t *n_out, bsc_prep_stats *prep_stats,
                             bsc_read_profile *profile);
int bsc_block_bcf_rawdev(bsc_context *ctx, const void *d_raw, uint32_t nr, const void *d_seq, uint64_t seq_bytes, const void *d_misms, uint64_t n_misms,
                         uint64_t ins_pad, const bsc_prep_params *prep, uint32_t x, uint32_t y, const uint8_t *ref, const uint8_t *dbsnp,
                         const bsc_vcf_params *params, int with_stats, int32_t rid, const bsc_bcf_ids *ids, const bsc_bcf_names *names, uint8_t *out,
                         uint64_t out_cap, uint64_t *n_bytes, uint64_t *n_records, bsc_prep_stats *prep_stats, bsc_read_profile *profile);
/* BGZF on the device (csrc/bgzfdev.hip; SAM specification section 4.1): a writer that turns a byte stream — the BCF magic and header from the
 * host, then the blocks' streams as they are on the device — into BGZF members.  Member k holds exactly bytes [k 0xFF00, (k + 1) 0xFF00) of
 * the LOGICAL stream (only the last is shorter), whatever the pieces the writes came in; each is one final DEFLATE block with dynamic
 * Huffman codes, or a stored block where that would not be smaller than the input.  The bytes depend on the logical stream alone.
 *   bsc_bgzf_open          a writer on the context (close it before the context is destroyed)
 *   bsc_bgzf_write         n host bytes;  bsc_bgzf_write_device: n bytes in HBM (ready when the call is made: work the context queued
 *                          is ordered before; a detached BCF stream may be freed when the call returns).  The bytes short of a member
 *                          wait in HBM for the next write.
 *   bsc_bgzf_take          the members completed so far (NULL and 0 when there are none), handed over like bsc_bcf_stream_detach:
 *                          bsc_detached_read / _wait, then bsc_detached_free (they count against the four pooled buffers out)
 *   bsc_bgzf_close         the last, short member and the 28-byte end-of-file marker (an empty stream is the marker alone), handed
 *                          over the same way; frees the writer whatever it returns
 * A NULL or closed writer, or a NULL pointer with bytes behind it: BSC_ERR_ARG. */
typedef struct bsc_bgzf bsc_bgzf;
int bsc_bgzf_open(bsc_context *ctx, bsc_bgzf **out);
int bsc_bgzf_write(bsc_bgzf *z, const void *src, uint64_t n);
int bsc_bgzf_write_device(bsc_bgzf *z, const void *d_src, uint64_t n);
int bsc_bgzf_take(bsc_bgzf *z, void **d_out, uint64_t *n_bytes);
int bsc_bgzf_close(bsc_bgzf *z, void **d_out, uint64_t *n_bytes);
/* what an index beside the file needs of the writer: *n_logical = the bytes written into the logical stream so far, *n_members = the members
 * completed so far (their compressed sizes are kept as they are produced; bsc_csi_finish reads them).  Either pointer may be NULL. */
int bsc_bgzf_tell(const bsc_bgzf *z, uint64_t *n_logical, uint64_t *n_members);

/*
 * A CSI index (CSIv1) of a compressed BCF / VCF file, made WHILE the file is written: the record-level work runs on the device
 * (csrc/csidev.hip, csrc/csidev_core.h), the host never walks the output stream.  The writer cuts members at fixed logical offsets, so a
 * record's virtual offset is arithmetic on its offset u in the uncompressed stream: voff(u) = coff[u / 0xFF00] << 16 | u % 0xFF00, coff[k] the
 * file offset of member k and coff[n_members] that of the end-of-file marker.
 *
 *   bsc_csi_entry          a run of consecutive records of one block's stream that share a window (0-based position >> min_shift): the
 *                          window, the records, the offset of the first one in the block's stream
 *   bsc_csi_scan_device    d_stream[0, n_bytes): whole BCF2 records of one contig in position order (BSC_CSI_BCF) or whole VCF data lines
 *                          (BSC_CSI_VCF); d_sync[n_sync + 1]: ascending offsets, each a record start or n_bytes, d_sync[0] = 0 and
 *                          d_sync[n_sync] = n_bytes (equal neighbours: an empty interval) — what the encoders leave as tile offsets; NULL
 *                          (n_sync is then ignored): one interval, walked by one lane, for small streams.  A lane walks an interval.
 *                          d_entries[<= cap_entries] in stream order; a run that continues across an interval boundary comes out as ADJACENT
 *                          entries with the same window, one per interval it touches (bsc_csi_add merges them).  d_totals: three device u64
 *                          {entries there are — also when that exceeds cap_entries: none is written beyond it —, records walked, error bits:
 *                          not 0 when a record left its interval (1), a position went backwards inside an interval (2), a text line had no
 *                          position (4) or the offsets were not ascending (8); the walk of that interval stops there}.  0 <= min_shift <= 31.
 *                          Asynchronous on `stream`; uses workspaces of the context (one scan in flight per context).
 *   bsc_block_csi_kept     the follow-up of bsc_block_bcf_rawdev_keep / bsc_block_vcf_rawdev_keep / bsc_block_bcf_again, BEFORE the stream is
 *                          detached: scans the kept stream by the encoder's own tile offsets on the context's stream, waits, and returns the
 *                          entries in memory of the context (valid until the next call of this function on it).  A malformed stream
 *                          (never seen: the encoder wrote it) is BSC_ERR_ARG.
 *   bsc_csi_open           an index beside the file writer z writes (BSC_ERR_ARG for a NULL or closed writer); names / lens: the header's
 *                          contigs.  depth = the smallest d with 2^(min_shift + 3 d) >= the longest contig + 256.
 *   bsc_csi_open_detached  the same without a writer, for a file compressed elsewhere with members cut every 0xFF00 bytes: the logical
 *                          stream starts with header_bytes bytes and grows by every block added; bsc_csi_members hands over the members'
 *                          compressed sizes (all of them, once, after the last block) in the place of bsc_bgzf_close
 *   bsc_csi_add            the entries of a block of contig tid whose n_bytes-long stream is written NEXT: the writer's logical length is
 *                          the block's base.  Adjacent entries with one window — inside the block or across blocks — become one.  Blocks in
 *                          file order: tid never descends, windows never descend within a contig, u_beg ascends from 0 and stays below
 *                          n_bytes, every entry has records; anything else is BSC_ERR_ARG and leaves the index as it was.
 *   bsc_csi_finish         after bsc_bgzf_close (before: BSC_ERR_ARG): the .csi file's bytes — itself BGZF, one stored member per 0xFF00
 *                          bytes and the end-of-file marker — into buf[cap]; returns their number; buf NULL / cap too small: the size needed
 *                          and nothing written
 *   bsc_csi_close          frees the index (NULL: nothing)
 * Contents, one rule for every builder: header "CSI\1", min_shift, depth, l_aux, aux, n_ref; l_aux = 0 for BCF, for VCF the tabix block
 * {format 2, col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, l_nm} and the NUL-terminated names.  Per contig the leaf bins that hold
 * records, ascending: bin = ((1 << 3 depth) - 1) / 7 + window, loffset = its one chunk's begin, the chunk [voff(first record's start),
 * voff(last record's end)]; then the pseudo-bin ((1 << 3 (depth + 1)) - 1) / 7 + 1, loffset 0, chunks (voff of the contig's first record,
 * voff behind its last) and (records, 0).  A contig without records: n_bin = 0.  n_no_coor = 0.  Sparse bins are NOT folded into their
 * parents as htslib does — a size optimisation the format does not require.
 */
#define BSC_CSI_BCF 0
#define BSC_CSI_VCF 1
typedef struct {
  uint32_t window, n_records;
  uint64_t u_beg;
} bsc_csi_entry;
typedef struct bsc_csi bsc_csi;
int bsc_csi_scan_device(bsc_context *ctx, int format, const void *d_stream, uint64_t n_bytes, const void *d_sync, uint32_t n_sync, int min_shift,
                        void *d_entries, uint64_t cap_entries, void *d_totals, void *stream);
int bsc_block_csi_kept(bsc_context *ctx, int min_shift, const bsc_csi_entry **entries, uint64_t *n_entries, uint64_t *n_records);
int bsc_csi_open(bsc_bgzf *z, int format, int min_shift, int n_refs, const char *const *names, const uint32_t *lens, bsc_csi **out);
int bsc_csi_open_detached(int format, int min_shift, int n_refs, const char *const *names, const uint32_t *lens, uint64_t header_bytes, bsc_csi **out);
int bsc_csi_members(bsc_csi *ix, const uint64_t *sizes, uint64_t n_members);
int bsc_csi_add(bsc_csi *ix, int32_t tid, const bsc_csi_entry *entries, uint64_t n, uint64_t n_bytes);
long bsc_csi_finish(bsc_csi *ix, void *buf, uint64_t cap);
void bsc_csi_close(bsc_csi *ix);

/*
 * A tabix (.tbi) or CSI (.csi) index of a BGZF-compressed methylation table (bam2bcf --meth, --meth-merge), made WHILE the table is written:
 * the line-level work runs on the device (csrc/beddev.hip, csrc/bedidx_core.h), the host never walks the table.  No reading tool was at
 * hand when this was written (no tabix, no pysam): the bytes are pinned by the rule below, from which the kernel, the host form
 * (bsc_bed_entries_host), the writer (csrc/tabix.c) and an independent Python builder (tests/tabix_ref.py) are each written.
 *
 * Line     the bytes up to and including '\n': chrom '\t' start '\t' end '\t' ...; start and end plain decimal of 1 .. 10 digits, 0-based
 *          half open, 0 <= start < end <= 2^32.  A stream is one contig's lines with start non-descending.  With s = min_shift (0 .. 31):
 *          wb = start >> s, wl = (end - 1) >> s.  A BED line is an interval: a combined-strand CpG line covers two bases, and one whose
 *          start is 2^s - 1 (mod 2^s) lies in two windows.
 * Entry    (what the device makes) a run: a maximal sequence of consecutive lines inside one interval of the stream that share (wb, wl).
 *          bsc_bed_entry {win_beg, win_last, n_lines, zero, u_beg}: 24 bytes, u_beg the offset of the run's first line in the block's stream.
 *          Entries come out in stream order whatever the launch geometry; a run that continues across an interval border comes out as
 *          adjacent entries with equal (win_beg, win_last); an empty interval gives none.
 * bsc_bed_scan_device   the twin of bsc_csi_scan_device, with its d_sync contract (NULL: one interval, walked by one lane).  d_totals: three
 *          device u64 {entries there are — also beyond cap_entries: nothing is written beyond it —, lines walked, error bits: a line that
 *          leaves its interval (1), a start below the one before it inside an interval (2), a line without two tab-separated decimal
 *          columns after the first, or end <= start, or end > 2^32, or more than 10 digits (4), interval offsets that descend or lie beyond
 *          the stream (8); the walk of that interval stops at the first error}.  Asynchronous on `stream`; uses workspaces of the context.
 * bsc_bed_entries_host  the same on the host, from the same statements (csrc/bedidx_core.h): the kernel's checker.  totals: three u64.
 * bsc_block_meth_index_kept   the follow-up of bsc_block_meth_kept / bsc_block_meth_cpg_kept, BEFORE bsc_meth_stream_detach: scans the
 *          context's table by the encoder's own tile offsets on the context's stream, waits, and returns the entries in memory of the
 *          context (valid until the next call of this function on it); *n_lines = what the table call returned.  No table on the context
 *          (none made, or detached), or error bits: BSC_ERR_ARG.  Nothing else the context keeps changes.
 * Bin      with depth D: k the smallest k >= 0 with wb >> 3k == wl >> 3k; bin = ((1 << 3 (D - k)) - 1) / 7 + (wb >> 3k).  k > D, or
 *          wl >= 1 << 3 D: refused.
 * Chunks   an entry's extent is [base + u_beg, base + u_next): base the logical length of the file before the block, u_next the next
 *          entry's u_beg or the block's n_bytes.  Per bin, in file order: an extent that begins exactly where the bin's last chunk ends
 *          extends it, anything else opens a new chunk — parent bins may hold several, and so may a leaf bin that a straddling line
 *          interrupts.  A chunk is (voff(begin), voff(end)), voff the arithmetic of bsc_csi_* on members cut every 0xFF00 logical bytes.
 * Linear   n_intv = 1 + the largest wl of the contig's lines (0 for a contig without lines); ioff[w] = voff of the first line with
 *          wb <= w <= wl; a window no line overlaps takes the value of the next window that has one.
 * Pseudo-bin   ((1 << 3 (D + 1)) - 1) / 7 + 1 (37450 at D = 5): chunks (voff of the contig's first line, voff behind its last), (lines, 0).
 * .tbi     "TBI\1", n_ref, format 0x10000, col_seq 1, col_beg 2, col_end 3, meta '#', skip 0, l_nm, the NUL-terminated names of ALL header
 *          contigs in order; per contig n_bin, the bins ascending {bin u32, n_chunk i32, chunks}, the pseudo-bin last where the contig has
 *          lines, then n_intv and ioff[]; then n_no_coor (u64) 0.  min_shift is 14 and D is 5; a contig longer than 2^29 is refused at
 *          open with a message that names csi.
 * .csi     "CSI\1", min_shift, depth (the rule of bsc_csi_open), l_aux = 28 + l_nm, aux = the same seven ints and the names, n_ref; per
 *          contig n_bin, the bins {bin, loffset u64, n_chunk, chunks}: loffset = ioff[first window of the bin] under the linear rule at
 *          min_shift, 0 for the pseudo-bin; then n_no_coor 0.
 * Both files are BGZF as the .csi of a BCF is: one stored member per 0xFF00 bytes and the end-of-file marker.
 *   bsc_tbx_open / _open_detached / _members / _finish / _close   as their bsc_csi_* namesakes; kind: BSC_TBX_TBI (min_shift must be 14) or
 *          BSC_TBX_CSI (1 .. 31); z: the TABLE's writer.
 *   bsc_tbx_add   the entries of the block of contig tid whose n_bytes-long table is written NEXT.  A descending tid; within a contig a
 *          win_beg below the last one; a u_beg that does not ascend from 0 or reaches n_bytes; an entry without lines; win_last < win_beg;
 *          a bin out of range: BSC_ERR_ARG, and the index stays as it was.
 */
#define BSC_TBX_TBI 0
#define BSC_TBX_CSI 1
typedef struct {
  uint32_t win_beg, win_last, n_lines, zero;
  uint64_t u_beg;
} bsc_bed_entry;
typedef struct bsc_tbx bsc_tbx;
int bsc_bed_scan_device(bsc_context *ctx, const void *d_stream, uint64_t n_bytes, const void *d_sync, uint32_t n_sync, int min_shift, void *d_entries,
                        uint64_t cap_entries, void *d_totals, void *stream);
int bsc_bed_entries_host(const void *stream, uint64_t n_bytes, const uint64_t *sync, uint32_t n_sync, int min_shift, bsc_bed_entry *entries,
                         uint64_t cap_entries, uint64_t totals[3]);
int bsc_block_meth_index_kept(bsc_context *ctx, int min_shift, const bsc_bed_entry **entries, uint64_t *n_entries, uint64_t *n_lines);
int bsc_tbx_open(bsc_bgzf *z, int kind, int min_shift, int n_refs, const char *const *names, const uint32_t *lens, bsc_tbx **out);
int bsc_tbx_open_detached(int kind, int min_shift, int n_refs, const char *const *names, const uint32_t *lens, uint64_t header_bytes, bsc_tbx **out);
int bsc_tbx_members(bsc_tbx *ix, const uint64_t *sizes, uint64_t n_members);
int bsc_tbx_add(bsc_tbx *ix, int32_t tid, const bsc_bed_entry *entries, uint64_t n, uint64_t n_bytes);
long bsc_tbx_finish(bsc_tbx *ix, void *buf, uint64_t cap);
void bsc_tbx_close(bsc_tbx *ix);
/* bsc_block_bcf_rawdev with the stream left on the device (room: dev_cap bytes; BSC_ERR_ARG and the length needed in *n_bytes when it does
 * not fit), and bytes [off, off + n) of that stream -> dst, queued on the context's stream (bsc_synchronize before dst is read): a contig-sized
 * block's stream is gigabytes — read in pieces through a small page-locked buffer it costs no page-locking of its own */
int bsc_block_bcf_rawdev_keep(bsc_context *ctx, const void *d_raw, uint32_t nr, const void *d_seq, uint64_t seq_bytes, const void *d_misms, uint64_t n_misms,
                              uint64_t ins_pad, const bsc_prep_params *prep, uint32_t x, uint32_t y, const uint8_t *ref, const uint8_t *dbsnp,
                              const bsc_vcf_params *params, int with_stats, int32_t rid, const bsc_bcf_ids *ids, const bsc_bcf_names *names, uint64_t dev_cap,
                              uint64_t *n_bytes, uint64_t *n_records, bsc_prep_stats *prep_stats, bsc_read_profile *profile);
int bsc_bcf_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);

/*
 * VCF TEXT on the device (csrc/vcftextdev.hip): for every record with emit != 0, in position order, the line bsc_vcf_format_rec writes
 * for it and '\n' — the data lines of the reference's -O v; through a bsc_bgzf writer, its -O z.  The host formatter is the checker: the
 * bytes are the same for ANY record contents (gt > 9 prints as genotype 0, at most six GL values, "%.5s" of the context strings stops at
 * a NUL; FORMAT GL is printf's "%g" of each float, in integer arithmetic: csrc/fmtg_dev.h).
 *   contig               CHROM: 1 .. 255 bytes without a tab or a newline (BSC_ERR_ARG otherwise).  The longest line is the contig's name
 *                        + 410 bytes (at most 665).
 *   names                the table the BCF encoder takes (bsc_bcf_names above) and its rule: the ID of a record whose rs_found flag is
 *                        set and whose position the table lists, at most 63 bytes of it (up to a NUL, as "%s" prints); "." otherwise
 *   bsc_vcf_text_block_device   d_recs[<= max_recs] packed records in HBM, *d_n_recs of them (a device u64) -> d_out[<= out_cap] bytes
 *                        (16-byte aligned, as the BCF encoder's); d_totals = three device u64 {length of the stream, records written
 *                        with a clamped gt / n_gl, records written}; a stream longer than out_cap is cut at a 64-record boundary, its
 *                        full length still in d_totals[0].  Asynchronous on `stream`.
 *   bsc_vcf_text_sites_device   the same from the per-position arrays bsc_reads_chain_device leaves (d_core[n], d_aux[n]); a position
 *                        without a record costs the 16 bytes that hold its emit flag (the chain's length byte is not used: it holds BCF
 *                        lengths)
 *   bsc_fmt_g[_device]   the number formatter alone, 16 bytes per value: the characters, zero padding, the length in byte 15.  The host
 *                        form is the C library's snprintf("%g"); the device form gives the same bytes for every one of the 2^32 patterns.
 *   bsc_block_vcf_rawdev_keep   bsc_block_bcf_rawdev_keep with the text encoder in the BCF encoder's place: the block's lines stay on the
 *                        device and are handed over with bsc_bcf_stream_detach / bsc_detached_* / bsc_bcf_stream_read; dev_cap too small:
 *                        BSC_ERR_ARG with *n_bytes = the room needed, and bsc_block_bcf_again then runs the TEXT encoder once more.
 *                        Like the BCF block entries, it REFUSES (BSC_ERR_ARG) a block with a record whose gt > 9 or n_gl > 6 — records the
 *                        chain never forms — although the device-level entries above write such records clamped and count them.
 * The other bsc_block_bcf* / bsc_blocks_bcf* entries have no text twin yet: inside, the request that names the encoder (a format tag and
 * the contig's name) is the only difference, so each can be added on the same field.
 */
int bsc_vcf_text_block_device(bsc_context *ctx, const void *d_recs, const void *d_n_recs, uint64_t max_recs, const char *contig,
                              const bsc_bcf_names *names, void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_vcf_text_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, const char *contig, const bsc_bcf_names *names,
                              void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_fmt_g(const float *v, uint64_t n, uint8_t *out16);
int bsc_fmt_g_device(bsc_context *ctx, const void *d_v, uint64_t n, void *d_out16, void *stream);
int bsc_block_vcf_rawdev_keep(bsc_context *ctx, const void *d_raw, uint32_t nr, const void *d_seq, uint64_t seq_bytes, const void *d_misms, uint64_t n_misms,
                              uint64_t ins_pad, const bsc_prep_params *prep, uint32_t x, uint32_t y, const uint8_t *ref, const uint8_t *dbsnp,
                              const bsc_vcf_params *params, int with_stats, const char *contig, const bsc_bcf_names *names, uint64_t dev_cap,
                              uint64_t *n_bytes, uint64_t *n_records, bsc_prep_stats *prep_stats, bsc_read_profile *profile);
/*
 * The per-cytosine methylation table (bedMethyl) on the device (csrc/methdev.hip; the host form csrc/methbed.c is its checker): the
 * third encoder over a block's records, and the first whose output is the caller's result rather than a serialisation of it.  The
 * reference has the rule for its report's CpG_ref_meth / CpG_nonref_meth histograms only (src/print_vcf.c:442-515); a record gives a
 * line iff
 *   core.emit != 0;  core.gt == 4 (CC, strand '+') or 7 (GG, strand '-');  core.cg == 'C', or 'H' with contexts == BSC_METH_ALL;
 *   a + b >= max(1, min_cov), a the non-converted and b the converted count of the strand: counts[5], counts[7] for '+',
 *   counts[6], counts[4] for '-' (:450-451, :472-473, and the reference's `if(a + b)`);  core.phred >= min_phred;
 *   !pass_only || core.flt == 0.
 * The line: 15 tab-separated columns and '\n', every number plain decimal —
 *   chrom  start = pos - 1  end = pos  name  score = min(a + b, 1000)  strand  start  end  itemRgb  a + b  pct  a  b  GQ = phred  FILTER
 *   name      "CG" for cg == 'C'; else by the called second neighbour (cx_gt[4] for '+', cx_gt[0] for '-'): "CHG" when it is 'G' ('+') /
 *             'C' ('-'), "CHH" for one of the other three of A C G T, "CHN" for anything else
 *   pct       (200 a + (a + b)) / (2 (a + b)) in 64 bits: 100 a / (a + b) rounded half up
 *   itemRgb   entry pct / 10 of 0,255,0 55,255,0 105,255,0 155,255,0 205,255,0 255,255,0 255,205,0 255,155,0 255,105,0 255,55,0 255,0,0
 *   FILTER    the text bsc_vcf_format_rec writes in that column: PASS, mac1 (flt & 128), fail
 * contig: 1 .. 255 bytes without a tab or a newline (BSC_ERR_ARG otherwise).  The longest line is the contig's name + 111 bytes.
 *   bsc_meth_format_rec     the host form: returns the length written (no NUL), 0 when the record gives no line, the length needed —
 *                           and nothing written — when cap is too small, < 0 for a bad argument
 *   bsc_meth_block_device   d_recs[<= max_recs] packed records in HBM, *d_n_recs of them (a device u64) -> d_out[<= out_cap] bytes
 *                           (16-byte aligned); d_totals = four device u64 {length of the stream, lines, sum of a, sum of b}; a stream
 *                           longer than out_cap is cut at a 64-record boundary, its full length still in d_totals[0].  Asynchronous
 *                           on `stream`; uses workspaces of the context (one encoding in flight per context).
 *   bsc_meth_sites_device   the same from the per-position arrays bsc_reads_chain_device leaves (d_core[n], d_aux[n]); a position
 *                           without a record costs the 16 bytes that hold its emit flag
 *   bsc_block_meth_kept     the follow-up of bsc_block_bcf_rawdev_keep / bsc_block_vcf_rawdev_keep (and of bsc_block_bcf_again behind
 *                           them): the table of THAT block, from the per-position arrays it left in HBM, into a buffer of the
 *                           context's own (room: dev_cap bytes).  The kept BCF / text stream, its tile offsets and bsc_block_csi_kept
 *                           are untouched, before or after.  dev_cap too small: BSC_ERR_ARG with *n_bytes = the room needed, and the
 *                           call may be repeated.  sums = {sum of a, sum of b} (may be NULL).  BSC_ERR_ARG when the last call on the
 *                           context left no single block's arrays: nothing kept, a block pending, the batched entries.  Waits.
 *   bsc_meth_stream_read    bytes [off, off + n) of that table -> dst, queued on the context's stream (bsc_bcf_stream_read's twin)
 *   bsc_meth_stream_detach  the table handed over like bsc_bcf_stream_detach hands the kept stream over: bsc_detached_read / _wait /
 *                           _free or bsc_bgzf_write_device on it (it counts against the four pooled buffers out); the context forgets it
 * Not built: the batched and host-buffer block entries.  (The combined-strand line per CpG dinucleotide: bsc_meth_cpg_*, the bigWig track:
 * bsc_bigwig_*, both below.)
 */
#define BSC_METH_CPG 0
#define BSC_METH_ALL 1
typedef struct {
  int32_t contexts;   /* BSC_METH_CPG: CpG cytosines only; BSC_METH_ALL: CHG / CHH too */
  uint32_t min_cov;   /* a + b at least this (and at least 1) */
  uint32_t min_phred; /* core.phred at least this */
  int32_t pass_only;  /* not 0: records with FILTER PASS only */
} bsc_meth_params;
void bsc_meth_params_default(bsc_meth_params *p); /* {BSC_METH_CPG, 1, 0, 0} */
long bsc_meth_format_rec(const bsc_vcf_rec *r, const char *contig, const bsc_meth_params *p, char *buf, size_t cap);
int bsc_meth_block_device(bsc_context *ctx, const void *d_recs, const void *d_n_recs, uint64_t max_recs, const char *contig,
                          const bsc_meth_params *params, void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_meth_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, const char *contig, const bsc_meth_params *params,
                          void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_block_meth_kept(bsc_context *ctx, const char *contig, const bsc_meth_params *p, uint64_t dev_cap, uint64_t *n_bytes, uint64_t *n_lines,
                        uint64_t sums[2]);
int bsc_meth_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_meth_stream_detach(bsc_context *ctx, void **d_stream, uint64_t *n_bytes);
/*
 * The combined-strand CpG table (csrc/methdev.hip: bsc_meth_cpg_size_kernel / _write_kernel; the host form csrc/methcpg.c is its checker):
 * one line per CpG dinucleotide, both strands' counts added.  A CpG is one site read from two strands: the C at p shows on the '+' strand,
 * the G at p + 1 is the '-' strand's C.  The reference pairs the two for its report only (prev_cpg_x, src/print_vcf.c:442-475).  This is the
 * one encoder whose line depends on a record's neighbours.  The rule, from which the host form, the tests' Python form and the kernels are
 * each written:
 *   HALVES   a record is a half iff it passes the per-cytosine rule with contexts = BSC_METH_CPG, except the coverage threshold:
 *            core.emit != 0;  core.gt == 4 (plus half) or 7 (minus half);  core.cg == 'C';  core.phred >= min_phred;
 *            !pass_only || core.flt == 0;  a + b >= 1 (a, b as above: counts[5], counts[7] for plus, counts[6], counts[4] for minus).
 *   PAIRS    a plus half at position p and a minus half at p + 1 (compared in 64 bits: 2^32 - 1 has no partner) that is the NEXT record
 *            form a pair.  Packed form: record i + 1 with pos == p + 1.  Per-position form: index i + 1, with the same pos test, and its
 *            emit byte not 0 where that array is given.  Every other half is a single.  A record is a half of at most one pair (CC and GG
 *            exclude each other).  Records at or beyond the count (*d_n_recs, n) do not exist, whatever their bytes hold.
 *   LINES    a pair gives ONE line, placed at its plus half; a single gives one line; a minus half that belongs to a pair gives none.
 *            A and B are the sums of the halves' a and b, in 64 bits.  The line is written iff A + B >= max(1, min_cov): the threshold
 *            is on the sum (a pair below it gives no line at all).
 *   COLUMNS  the 15 columns of the per-cytosine table:
 *            start    the plus position - 1; for a single minus half at q: q - 2.  Modulo 2^32, as pos - 1 above.
 *            end      start + 2, in 64 bits (2^32 + 1 at most); thick start / thick end repeat start / end
 *            name     CG
 *            strand   '.' for a pair, '+' or '-' for a single
 *            score    min(A + B, 1000);  coverage A + B;  pct and itemRgb from A and A + B exactly as above;  then A, B
 *            GQ       the smaller phred of the halves
 *            FILTER   from the OR of the halves' flt: fail if flt & 127, else mac1 if flt & 128, else PASS
 * Consequences: lines come out in record order with strictly increasing start (positions increase); no carry between blocks is needed —
 * the reader starts a new block only where two positions or more are uncovered (src/get_template_vector.c:141-147), so two adjacent
 * positions that both have records lie in one block.  contexts == BSC_METH_ALL is refused (BSC_ERR_ARG; -1 from the host form): only a CpG
 * has a partner strand here.  The longest line is the contig's name + 111 bytes, as above: the name is a byte shorter, A + B (2^34 - 4 at
 * most) a digit longer.
 *   bsc_meth_cpg_format_recs   the host form: the table of recs[0 .. n) in order -> buf; returns the length written, the length needed —
 *                              and nothing written — when cap is too small, < 0 for a bad argument.  totals (may be NULL) = {length,
 *                              lines, sum of A, sum of B, pairs written}
 *   bsc_meth_cpg_block_device  bsc_meth_block_device's twin;  d_totals = FIVE device u64 {length, lines, sum of A, sum of B, pairs written}
 *   bsc_meth_cpg_sites_device  bsc_meth_sites_device's twin
 *   bsc_block_meth_cpg_kept    bsc_block_meth_kept's twin: the same source arrays, the same emit-byte gate, the same conditions, into the same
 *                              buffer of the context — bsc_meth_stream_read / _detach serve it unchanged.  sums = {sum of A, sum of B,
 *                              pairs written} (may be NULL)
 */
long bsc_meth_cpg_format_recs(const bsc_vcf_rec *recs, size_t n, const char *contig, const bsc_meth_params *p, char *buf, size_t cap,
                              uint64_t totals[5]);
int bsc_meth_cpg_block_device(bsc_context *ctx, const void *d_recs, const void *d_n_recs, uint64_t max_recs, const char *contig,
                              const bsc_meth_params *params, void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_meth_cpg_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, const char *contig, const bsc_meth_params *params,
                              void *d_out, uint64_t out_cap, void *d_totals, void *stream);
int bsc_block_meth_cpg_kept(bsc_context *ctx, const char *contig, const bsc_meth_params *p, uint64_t dev_cap, uint64_t *n_bytes, uint64_t *n_lines,
                            uint64_t sums[3]);
/*
 * The per-region methylation summary (csrc/methregionsdev.hip: bsc_meth_regions_tile_kernel / _region_kernel; the host form
 * csrc/methregions.c is its checker): the first output that is a REDUCTION over positions — per interval of a BED file (promoters, CpG
 * islands, fixed tiles), the cytosines inside it added up, instead of a table of every cytosine pulled off the device and mapped on the
 * host.  The rule, from which the host form, the tests' Python form and the kernels are each written:
 *   SITE      a record that gives a line under the per-cytosine rule of bsc_meth_format_rec with the given bsc_meth_params (contexts,
 *             min_cov, min_phred, pass_only: exactly as written there).  Its values: a, the non-converted count, and b, the converted
 *             count (counts[5] / counts[7] for CC, counts[6] / counts[4] for GG), and pct = (200 a + (a + b)) / (2 (a + b)) in 64 bits.
 *             The summary counts cytosines, not dinucleotides: a CpG that straddles a region's border gives the half that lies inside;
 *             sum of a and sum of b are those of either table.
 *   REGION    bsc_meth_region {start, end}: 0-based and half-open, as in BED.  It contains the site at 1-based position pos iff
 *             start < pos <= end — the site's bedMethyl start pos - 1 lies in [start, end).  pos == 0 belongs to no region;
 *             start == end is legal and empty; start > end is refused.  Regions may overlap, nest and repeat: each is summed alone.
 *   SUMS      four u64 per region: {sites, A = sum of a, B = sum of b, P = sum of pct}.  All integers, added in 64 bits from the first
 *             add (a lane's a may be 2^32 - 1).
 *   LINE      ten tab-separated columns and '\n', plain decimal, no header:
 *               chrom  start  end  name  sites  A + B  A  B  level  mean
 *             name: the BED's fourth column, or "." when there is none;  level = (200 A + (A + B)) / (2 (A + B)), the pct formula on
 *             the sums (the pooled level; "." when A + B == 0, which sites != 0 excludes);  mean = (2 P + sites) / (2 sites), the
 *             sites' mean pct rounded half up;  level and mean are "." when sites == 0.
 * Host forms (csrc/methregions.c):
 *   bsc_meth_regions_sum_recs   adds the rule over packed records recs[0 .. n) into acc[n_regions][4] (NOT zeroed here); a plain loop
 *   bsc_meth_regions_format     the lines of regions[0 .. n) of one contig -> buf; names: n strings, NULL or a NULL entry = ".".  Returns
 *                               the length written, the length needed — and nothing written — when cap is too small, < 0 for a bad
 *                               argument (a contig or a name that is empty, longer than 255 bytes or holds a tab or a newline)
 *   bsc_meth_regions_parse_bed  BED text -> *out (bsc_meth_bed_free).  A line is three or more columns separated by tabs — or, where the
 *                               line holds no tab, by single spaces; the fourth column is the name.  '#', "track" and "browser" lines and
 *                               empty lines are skipped, a '\r' before the '\n' is dropped.  Anything else is refused (BSC_ERR_ARG) with
 *                               the 1-based line number in bsc_last_error: fewer than three columns, a coordinate that is not all digits
 *                               or is >= 2^32, start > end, an empty contig name (or one longer than 255 bytes), a final line without
 *                               '\n'.  The result lists the contigs in order of first appearance; contig c's regions are
 *                               regions[first[c] .. first[c + 1]), STABLY sorted by (start, end), names[] beside them.
 * On the device the per-position arrays are dense — entry i is position x0 + i — so an interval is a difference of two prefix sums,
 * whatever its length and however regions overlap: a tile pass (one wave per 64 positions: the four sums of the tile), an exclusive scan
 * of the four planes, and a region pass (one wave per CANDIDATE region: prefix(i_hi) - prefix(i_lo), the partial tiles at the two ends
 * evaluated again) that adds into the region's accumulators.  Candidates: the attached regions whose index lies in [lo, hi), from two
 * binary searches on the host over the starts and the running maximum of the ends — a superset; a chromosome-long region listed first
 * makes lo = 0 for every block.
 *   bsc_meth_regions_attach        regions[0 .. n) of ONE contig, sorted by (start, end), uploaded; their accumulators zeroed.  n == 0
 *                                  detaches.  Unsorted input, start > end or n > 2^27: BSC_ERR_ARG, and the previous attachment stays.
 *                                  As bsc_dbsnp_attach: once per contig; freed by bsc_destroy.  Waits.
 *   bsc_meth_regions_sites_device  accumulates from d_core[n] / d_aux[n]: entry i is position x0 + i (x0 >= 1, x0 + n - 1 < 2^32), and
 *                                  where it gives a site its core.pos equals that — what bsc_reads_chain_device leaves.  Asynchronous on
 *                                  `stream`; a region's accumulators are read, added to and stored by ONE wave per call, so calls must
 *                                  be ordered one behind the other (one stream).  BSC_ERR_ARG with nothing attached.
 *   bsc_block_meth_regions_kept    the follow-up of the _keep block calls: preconditions and refusals of bsc_block_meth_kept; from the
 *                                  arrays that block left in HBM, by the chain's emit byte per position, with the block's own x.
 *                                  sums (may be NULL) = the block's {sites, sum of a, sum of b} whether or not a region holds them;
 *                                  *n_sites (may be NULL) = sums[0].  The kept stream, the methylation table, bsc_block_csi_kept and
 *                                  the report are untouched; before or after them.  Waits.
 *   bsc_meth_regions_read          the accumulators -> acc_host[n][4], n = the attached count; waits for the context's stream and the
 *                                  stream of the last accumulating call
 *   bsc_meth_regions_reset         zeroes them (waits likewise)
 * Not built: a packed-records device form (packed records are not dense in position), the batched and host-buffer block entries.
 */
typedef struct {
  uint32_t start, end; /* 0-based, half-open */
} bsc_meth_region;
typedef struct {
  uint32_t n_contigs;
  char **contigs;           /* in order of first appearance */
  uint64_t *first;          /* n_contigs + 1 */
  uint64_t n_regions;
  bsc_meth_region *regions; /* contig by contig, each sorted by (start, end), stably */
  char **names;             /* beside them: the fourth column, or "." */
} bsc_meth_bed;
int bsc_meth_regions_sum_recs(const bsc_vcf_rec *recs, size_t n, const bsc_meth_params *p, const bsc_meth_region *regions, size_t n_regions,
                              uint64_t *acc);
long bsc_meth_regions_format(const char *contig, const bsc_meth_region *regions, const char *const *names, const uint64_t *acc, size_t n, char *buf,
                             size_t cap);
int bsc_meth_regions_parse_bed(const char *text, size_t len, bsc_meth_bed **out);
void bsc_meth_bed_free(bsc_meth_bed *bed);
int bsc_meth_regions_attach(bsc_context *ctx, const bsc_meth_region *regions, uint64_t n);
int bsc_meth_regions_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, uint32_t x0, const bsc_meth_params *params,
                                  void *stream);
int bsc_block_meth_regions_kept(bsc_context *ctx, const bsc_meth_params *params, uint64_t *n_sites, uint64_t sums[3]);
int bsc_meth_regions_read(bsc_context *ctx, uint64_t *acc_host, uint64_t n);
int bsc_meth_regions_reset(bsc_context *ctx);
/*
 * The methylation bigWig track (csrc/bigwigdev.hip: the bsc_bigwig_*_kernel family; csrc/bigwig.c holds the host form, which is their
 * checker, and the writer of the file): the file genome browsers and deepTools open — the methylation level per cytosine with its
 * zoom pyramid —, made from the per-position arrays a block call left in HBM.  The reference's users get it from a second program that
 * reads the BCF back.  Every number is an exact integer until the moment a float is written; no result depends on an order of summation;
 * blocks merge exactly.  The rule, from which the host form, the tests' Python forms and the kernels are each written:
 *   SITE      a record that gives a line under the per-cytosine rule of bsc_meth_format_rec with the given bsc_meth_params (contexts —
 *             BSC_METH_ALL included —, min_cov, min_phred, pass_only: exactly as written there), with the same a and b.
 *             start = pos - 1.  Sites come in record order, their starts strictly increasing.
 *   VALUE     m = (2000 a + (a + b)) / (2 (a + b)) in 64 bits: 1000 a / (a + b) rounded half up, 0 .. 1000, tenths of a percent.  The float
 *             written is (float)(m / 10.0): C double division, then the conversion.  The host makes the table of these 1001 floats once
 *             and the device copies entries of it: the device does no floating-point arithmetic here.
 *   SUMMARY   bsc_bw_sum, 40 bytes, of a run of sites: start = the first site's start, end = the last site's start + 1, count, min_m,
 *             max_m, sum_m, sum_m2 (the sum of m * m: at most count * 10^6).  Two runs merge by adding count, sum_m and sum_m2, taking
 *             the smaller min_m, the larger max_m, the earlier start and the later end.
 *   PARAMS    bsc_bw_params {items_per_section S: 1 .. 65535, default 1024;  reduction: >= 1, default 1024}.
 *   STREAM    of a block: section k holds the block's sites of rank [k S, (k + 1) S); sections lie back to back, uncompressed.  A section:
 *               chromId u32, chromStart u32 = its first site's start, chromEnd u32 = its last site's start + 1, itemStep u32 = 0,
 *               itemSpan u32 = 1, type u8 = 2 (varStep), reserved u8 = 0, itemCount u16          (24 bytes)
 *               itemCount x {start u32, value f32}
 *             little-endian.  Section k starts at byte k (24 + 8 S); only the last is short; n_bytes = 24 n_sections + 8 n_sites.
 *             A section never spans two blocks (a tiny block gives a tiny section).
 *   PER BLOCK sections[n_sections]: the summary of each section;  zoom0[n_windows]: the summaries of the windows w = start / reduction
 *             that hold at least one site, ascending.
 *   PYRAMID   (host, integers) level 0 is the blocks' zoom0 one behind the other; where a block's last window and the next block's
 *             first window lie on one contig and have the same w they merge.  Level l has windows of reduction * 4^l (64 bits): it is
 *             made by merging consecutive records of level l - 1 with equal start / (reduction * 4^l) on one contig.  Level 0 always
 *             exists; level l exists iff level l - 1 has more than 256 records; at most 8 levels.
 *   FILE      bbiFile version 4 as its published description states it, little-endian; readers follow offsets, the order is ours:
 *               0        header, 64 bytes: magic u32 = 0x888FFC26, version u16 = 4, zoomLevels u16, chromosomeTreeOffset u64,
 *                        fullDataOffset u64, fullIndexOffset u64, fieldCount u16 = 0, definedFieldCount u16 = 0, autoSqlOffset u64 = 0,
 *                        totalSummaryOffset u64, uncompressBufSize u32 = 0 (nothing is compressed; COMPRESSED FILE below), extensionOffset u64 = 0
 *               64       8 zoom headers of 24 bytes {reductionLevel u32 = min(reduction * 4^l, 2^32 - 1), reserved u32 = 0,
 *                        dataOffset u64, indexOffset u64}; unused ones zero
 *               256      total summary, 40 bytes {basesCovered u64 = the sites, minVal, maxVal, sumData, sumSquares f64} =
 *                        min_m / 10.0, max_m / 10.0, sum_m / 10.0, sum_m2 / 100.0 over everything; all zero with no site
 *               296      chromosome B+ tree: header 32 bytes {0x78CA8C91 u32, blockSize u32 = 256, keySize u32 = the longest name's
 *                        length, valSize u32 = 8, itemCount u64 = n_refs, reserved u64 = 0}; a node is {isLeaf u8, reserved u8 = 0,
 *                        count u16} and exactly count items (no padding); a leaf item key[keySize] (zero padded), chromId u32,
 *                        chromSize u32; a non-leaf item key[keySize], childOffset u64.  Every contig of the BAM header is listed, keys in
 *                        ascending memcmp order (readers search the tree); chromId = the contig's index in the BAM header, the order
 *                        the data are written in (what the R-tree needs).  Built bottom-up, up to 256 items a node, until one node is
 *                        left; written root first, level by level; a non-leaf key is its child's first key.  No contig: an empty leaf.
 *               fullDataOffset    u64 sectionCount, then the blocks' streams
 *               fullIndexOffset   R-tree over the sections: header 48 bytes {0x2468ACE0 u32, blockSize u32 = 256, itemCount u64,
 *                        startChromIx, startBase, endChromIx, endBase u32 (of everything; zero with no item), endFileOffset u64 = where
 *                        the indexed data end, itemsPerSlot u32 = 1, reserved u32 = 0}; a node {isLeaf u8, reserved u8, count u16} and
 *                        count items; a leaf item, 32 bytes: startChromIx, startBase, endChromIx, endBase u32, dataOffset u64, dataSize
 *                        u64; a non-leaf item, 24 bytes: the four bounds, childOffset u64.  Bottom-up with 256 a node until one node is
 *                        left, written root first, level by level; a node's start is the lexicographic minimum of its items' (chrom,
 *                        base) starts, its end the maximum of their ends.  No item: the root is an empty leaf.
 *               per level         u32 recordCount; its zoom blocks — up to 512 records of 32 bytes {chromId, chromStart, chromEnd,
 *                        validCount u32, minVal, maxVal, sumData, sumSquares f32} = (float)(min_m / 10.0), (float)(max_m / 10.0),
 *                        (float)(sum_m / 10.0), (float)(sum_m2 / 100.0); a block never spans two contigs —; then an R-tree with one leaf
 *                        item per block.  The level's dataOffset names the recordCount, its indexOffset the R-tree.
 *               end      u32 0x888FFC26
 *             The bytes are UCSC-unpinned, as the BCF bytes are htslib-unpinned: no UCSC or pyBigWig reader has seen them here;
 *             bs_call_amd/bigwig.py reads them back by the offsets alone.
 * Host (csrc/bigwig.c):
 *   bsc_bw_params_default      {1024, 1024}
 *   bsc_bigwig_sections_recs   the host form over packed records recs[0 .. n): the stream -> out[cap], the summaries -> sections[] and
 *                              zoom0[].  *n_sections and *n_zoom0 hold the ROOM of the two arrays on entry and the counts on return.  Where
 *                              any of the three rooms is too small: BSC_ERR_ARG, the three needs reported and nothing written.
 *   bsc_bigwig_open            a writer on a descriptor it may pwrite to (not closed here); names / lens: the BAM header's contigs
 *   bsc_bigwig_add             a block's stream appended (pwrite) and its entries kept.  BSC_ERR_ARG — nothing written — for a tid lower
 *                              than the last or not in the header, a start below the previous end on the same tid, or entries that do
 *                              not describe n_bytes (every section but the last of S sites, 24 n_sections + 8 n_sites = n_bytes)
 *   bsc_bigwig_finish          section count, R-tree, zoom levels, total summary, header, the closing magic; every write checked
 *                              (BSC_ERR_ARG with errno's text).  Once.
 *   bsc_bigwig_close           frees the writer (an unfinished file stays without a header: not a bigWig)
 * Device:
 *   bsc_bigwig_sites_device    from d_core[n] / d_aux[n], entry i = position x0 + i (x0 >= 1, x0 + n - 1 < 2^32; as
 *                              bsc_meth_regions_sites_device): the stream -> d_out[out_cap] (8-byte aligned), the summaries ->
 *                              d_sections[sec_cap], d_zoom[zoom_cap], and d_totals = six device u64 {n_bytes, n_sites, n_sections,
 *                              n_windows, sum of m, sum of m * m}.  An array whose room is too small is not written at all — the needs are
 *                              in d_totals, and nothing partial is to be trusted.  Asynchronous on `stream`; workspaces of the context
 *                              (one call in flight per context).
 *   bsc_block_bigwig_kept      the follow-up of the _keep block calls: preconditions and refusals of bsc_block_meth_kept; from the
 *                              arrays that block left in HBM, by the chain's emit byte per position, with the block's own x, into buffers
 *                              of its own.  *sections / *zoom0: the context's host copies, good until the next call.  The kept stream,
 *                              its tile offsets, the methylation tables, bsc_block_csi_kept and the region accumulators are untouched;
 *                              before or after them.  BSC_ERR_ARG with the sizes should a room be too small.  Waits.
 *   bsc_bigwig_stream_read     bytes [off, off + n) of that block's stream -> dst, queued on the context's stream
 * Compressed sections (csrc/zlibdev.hip: the bsc_zlib_*_kernel family; what UCSC's tools write and readers meet in practice):
 *   ZSTREAM   of a piece of bytes: the zlib header 78 9C, ONE final DEFLATE block — dynamic Huffman codes, or stored where that would not be
 *             smaller than the piece —, the piece's Adler-32 big-endian (RFC 1950, RFC 1951): at most the piece + 11 bytes.  A function of
 *             the piece's bytes alone.
 *   COMPRESSED FILE   the FILE above with every section replaced by its ZSTREAM and every zoom block by zlib's compress2 of it at the
 *             default level (host, libz: a pyramid is a few MB once per file); a leaf item's dataOffset / dataSize are the compressed
 *             ones; a level's leading u32 recordCount stays raw; uncompressBufSize = the largest raw size of any section or zoom block
 *             of the file (0 with none: then nothing is compressed either).  A writer is compressed or plain from its first non-empty add.
 *   bsc_zlib_pieces_device     piece k = bytes [k piece, min((k + 1) piece, n_bytes)) of d_src (any alignment), 1 <= piece <= 0xFF00: the
 *                              ZSTREAMs back to back in piece order -> d_out[out_cap], their lengths -> d_sizes[sizes_cap] (u32), and
 *                              d_totals = two device u64 {bytes out, pieces}.  The most needed: n_bytes + 11 pieces.  An array whose room
 *                              is too small is not written at all — the needs are in d_totals.  n_bytes = 0: {0, 0}.  Asynchronous on
 *                              `stream`; workspaces of the context (one call in flight per context).
 *   bsc_block_bigwig_deflate   the follow-up of bsc_block_bigwig_kept of the same block: that block's stream at stride 24 + 8 S into a buffer
 *                              of its own; *z_sizes: the context's host copy of the n_sections lengths, good until the next call.
 *                              BSC_ERR_ARG without a bsc_block_bigwig_kept before it, or with S > 8157 (24 + 8 S > 0xFF00).  A block with
 *                              no site: 0 / 0.  The uncompressed stream, the kept stream, the methylation tables, the CSI scan and the
 *                              region accumulators are untouched.  Waits.
 *   bsc_bigwig_zstream_read    bytes [off, off + n) of those streams -> dst, queued on the context's stream
 *   bsc_bigwig_add_z           bsc_bigwig_add for a block's ZSTREAMs: every check of bsc_bigwig_add on the summaries; in place of the byte
 *                              count, z_sizes[k] is 1 .. 24 + 8 count + 11 and their sum z_bytes.  After a non-empty bsc_bigwig_add_z a
 *                              non-empty bsc_bigwig_add is BSC_ERR_ARG with nothing written, and the reverse.
 * The coverage track (csrc/bwcovdev.hip: bsc_bwcov_write_kernel / bsc_bwcov_reduce_kernel over the mask of tracks, beside the tile, heads
 * and windows kernels of bigwigdev.hip; csrc/bigwig.c holds the host form and the writer): the depth a + b a level is read with, as a second
 * bigWig of the same sites.  The rule, from which the kernels, the host form and the Python forms are each written:
 *   TRACK     BSC_BW_LEVEL (bit 0): the track above, unchanged.  BSC_BW_COVERAGE (bit 1).  A track mask is 1, 2 or 3.
 *   SITE      exactly the SITE above: the same bsc_meth_params, the same a and b, the same emit-byte gate; a + b >= max(1, min_cov) is tested
 *             on the 64-bit sum, before any saturation.  Both tracks of one call therefore have the same sites, section boundaries, start /
 *             end / count, window set and n_bytes.
 *   COVERAGE VALUE   c = min(a + b, 2^32 - 1), a + b in 64 bits (counts already saturate at 2^32 - 1).  The float written is the conversion
 *             of the unsigned integer c to binary32, rounded once, to nearest, ties to even: C's (float)(uint32_t)c in the default rounding
 *             mode.  The device uses the hardware's u32 -> f32 conversion and does no other floating-point arithmetic here.
 *   SUMMARY   bsc_bw_sum, the same 40 bytes.  In a coverage summary min_m = min c, max_m = max c, sum_m = the sum of c (< 2^64 for
 *             count < 2^32: exact), sum_m2 = bits 0 .. 63 of the sum of c * c and _pad = its bits 64 .. 95 (the sum is < 2^96: exact).  In a
 *             level summary _pad stays 0.  Two coverage summaries merge as level summaries do, the 96-bit add carrying from sum_m2 into _pad.
 *   STREAM    the level STREAM with the coverage float in each item's value word: varStep type 2, 24 + 8 S bytes a section.
 *   PYRAMID   the level PYRAMID; on the host the merged sums are held in unsigned __int128, so nothing wraps.
 *   FILE / COMPRESSED FILE   the same layout and magic.  Every number is rounded ONCE from the exact integer, to nearest, ties to even
 *             (integer arithmetic on the host: no intermediate type).  Total summary: basesCovered = the sites; minVal, maxVal, sumData,
 *             sumSquares = min c, max c, the sum of c, the sum of c * c, each converted to f64.  A zoom record's minVal, maxVal, sumData,
 *             sumSquares are each converted to f32 directly from the integer, not through a double.  The level file's / 10.0 and / 100.0
 *             forms stay exactly as they are.
 *   bsc_bigwig_cov_sections_recs   the host form of the coverage track over packed records: the signature and the room rule of
 *                              bsc_bigwig_sections_recs; the kernels' checker.
 *   bsc_bigwig_open_track      bsc_bigwig_open with the writer's track, BSC_BW_LEVEL or BSC_BW_COVERAGE (anything else: BSC_ERR_ARG);
 *                              bsc_bigwig_open is this with BSC_BW_LEVEL.  A coverage writer's bsc_bigwig_add, _add_z, _finish and _close
 *                              apply the same checks and refusals; it keeps its entries' _pad (a level writer sets it to 0) and writes the
 *                              values and sums of the coverage FILE rule.  The level writer's bytes do not change.
 *   bsc_bigwig_tracks_device   bsc_bigwig_sites_device for a mask of tracks, in one sweep: its preconditions, alignment rules and refusals;
 *                              level_out / cov_out: a bsc_bw_track_out {d_out, out_cap, d_sections, sec_cap, d_zoom, zoom_cap} per requested
 *                              track, NULL for one not in `tracks` (a track asked for with NULL, or a mask other than 1, 2, 3: BSC_ERR_ARG).
 *                              d_totals = six device u64 {n_bytes, n_sites, n_sections, n_windows, sum of m, sum of m * m}, the last two 0
 *                              without bit 0 (a coverage track's totals are the sums of its section summaries: the host adds them).  An
 *                              array whose room is too small is not written at all and every other array is complete.  n = 0: six zeros.
 *   bsc_block_bigwig_tracks_kept   the twin of bsc_block_bigwig_kept for a mask of tracks: its preconditions, refusals and wait; the counts
 *                              once, the host copies of the sections and of zoom0 per requested track (NULL for the other; the pointer
 *                              arguments of a track not asked for may be NULL).  With bit 0 it fills the level buffers bsc_block_bigwig_kept
 *                              fills: bsc_bigwig_stream_read, bsc_block_bigwig_deflate and bsc_bigwig_zstream_read follow as they follow
 *                              that call; without bit 0 those are refused until the next level call.  The coverage stream lives in buffers
 *                              of its own (bsc_block_bigwig_kept leaves none: the three calls below are refused behind it).  The kept
 *                              stream, its tile offsets, the methylation tables, bsc_block_csi_kept, the region accumulators, the bigBed
 *                              data and the tabix scan are untouched.
 *   bsc_bigwig_cov_stream_read / bsc_block_bigwig_cov_deflate / bsc_bigwig_cov_zstream_read   bsc_bigwig_stream_read,
 *                              bsc_block_bigwig_deflate and bsc_bigwig_zstream_read for the coverage stream of the last
 *                              bsc_block_bigwig_tracks_kept with bit 1: bsc_zlib_pieces_device at stride 24 + 8 S, S <= 8157.
 * Not built: sharded runs, a device encoder for the zoom blocks, the batched and host-buffer block entries, a track of the combined-strand
 * CpGs, a per-base depth over every position (the kept arrays hold records only where the chain emitted one).
 */
typedef struct {
  uint32_t items_per_section; /* 1 .. 65535 */
  uint32_t reduction;         /* >= 1: the width of a level-0 zoom window */
} bsc_bw_params;
typedef struct {
  uint32_t start, end, count, min_m, max_m, _pad; /* _pad: 0 in a level summary; bits 64 .. 95 of the sum of c * c in a coverage summary */
  uint64_t sum_m, sum_m2;
} bsc_bw_sum;
#define BSC_BW_LEVEL 1u    /* track bits */
#define BSC_BW_COVERAGE 2u
typedef struct { /* where one track of bsc_bigwig_tracks_device goes: the rooms of bsc_bigwig_sites_device */
  void *d_out;
  uint64_t out_cap;
  void *d_sections;
  uint64_t sec_cap;
  void *d_zoom;
  uint64_t zoom_cap;
} bsc_bw_track_out;
typedef struct bsc_bigwig bsc_bigwig;
void bsc_bw_params_default(bsc_bw_params *p);
int bsc_bigwig_sections_recs(const bsc_vcf_rec *recs, size_t n, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bw_params *bw_params,
                             void *out, uint64_t cap, uint64_t *n_bytes, bsc_bw_sum *sections, uint64_t *n_sections, bsc_bw_sum *zoom0,
                             uint64_t *n_zoom0);
int bsc_bigwig_open(int fd, uint32_t n_refs, const char *const *names, const uint32_t *lens, const bsc_bw_params *bw_params, bsc_bigwig **bw);
int bsc_bigwig_add(bsc_bigwig *bw, uint32_t tid, const void *data, uint64_t n_bytes, const bsc_bw_sum *sections, uint64_t n_sections,
                   const bsc_bw_sum *zoom0, uint64_t n_zoom0);
int bsc_bigwig_finish(bsc_bigwig *bw);
void bsc_bigwig_close(bsc_bigwig *bw);
int bsc_bigwig_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, uint32_t x0, uint32_t chrom_id,
                            const bsc_meth_params *params, const bsc_bw_params *bw_params, void *d_out, uint64_t out_cap, void *d_sections,
                            uint64_t sec_cap, void *d_zoom, uint64_t zoom_cap, void *d_totals, void *stream);
int bsc_block_bigwig_kept(bsc_context *ctx, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bw_params *bw_params, uint64_t *n_bytes,
                          uint64_t *n_sites, const bsc_bw_sum **sections, uint64_t *n_sections, const bsc_bw_sum **zoom0, uint64_t *n_zoom0);
int bsc_bigwig_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_zlib_pieces_device(bsc_context *ctx, const void *d_src, uint64_t n_bytes, uint32_t piece, void *d_out, uint64_t out_cap, void *d_sizes,
                           uint64_t sizes_cap, void *d_totals, void *stream);
int bsc_block_bigwig_deflate(bsc_context *ctx, uint64_t *z_bytes, const uint32_t **z_sizes, uint64_t *n_sections);
int bsc_bigwig_zstream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_bigwig_add_z(bsc_bigwig *bw, uint32_t tid, const void *zdata, uint64_t z_bytes, const uint32_t *z_sizes, const bsc_bw_sum *sections,
                     uint64_t n_sections, const bsc_bw_sum *zoom0, uint64_t n_zoom0);
int bsc_bigwig_cov_sections_recs(const bsc_vcf_rec *recs, size_t n, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bw_params *bw_params,
                                 void *out, uint64_t cap, uint64_t *n_bytes, bsc_bw_sum *sections, uint64_t *n_sections, bsc_bw_sum *zoom0,
                                 uint64_t *n_zoom0);
int bsc_bigwig_open_track(int fd, uint32_t n_refs, const char *const *names, const uint32_t *lens, const bsc_bw_params *bw_params, uint32_t track,
                          bsc_bigwig **bw);
int bsc_bigwig_tracks_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, uint32_t x0, uint32_t chrom_id,
                             const bsc_meth_params *params, const bsc_bw_params *bw_params, uint32_t tracks, const bsc_bw_track_out *level_out,
                             const bsc_bw_track_out *cov_out, void *d_totals, void *stream);
int bsc_block_bigwig_tracks_kept(bsc_context *ctx, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bw_params *bw_params, uint32_t tracks,
                                 uint64_t *n_bytes, uint64_t *n_sites, uint64_t *n_sections, uint64_t *n_zoom0, const bsc_bw_sum **level_sections,
                                 const bsc_bw_sum **level_zoom0, const bsc_bw_sum **cov_sections, const bsc_bw_sum **cov_zoom0);
int bsc_bigwig_cov_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_block_bigwig_cov_deflate(bsc_context *ctx, uint64_t *z_bytes, const uint32_t **z_sizes, uint64_t *n_sections);
int bsc_bigwig_cov_zstream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
/*
 * The bedMethyl table as bigBed items (csrc/bigbeddev.hip: the bsc_bigbed_*_kernel family; csrc/bigbed.c holds the host form, which is their
 * checker): what a genome browser fetches by region — counts, GQ and FILTER per site — in place of the text table, made from the
 * per-position arrays a block call left in HBM.  Integers only, no atomics, no result that depends on an order.  The rule, from which the
 * host form, the tests' Python form and the kernels are each written:
 *   SITE      a record that gives a line under the per-cytosine rule of bsc_meth_format_rec with the given bsc_meth_params (contexts —
 *             BSC_METH_ALL included —, min_cov, min_phred, pass_only: exactly as written there).  Sites come in record order, their
 *             starts strictly increasing.
 *   ITEM      the site's bedMethyl line without its first three columns:
 *               chromId u32, chromStart u32 = pos - 1, chromEnd u32 = pos, little-endian                  (12 bytes)
 *               the line's bytes from the first byte of column 4 (the name) to the last byte of column 15, tabs included
 *               one NUL in the place of the '\n'
 *             so contig "\t" start "\t" end "\t" + the text + "\n" is the table's line, byte for byte.
 *             BSC_BB_ITEM_MAX = 100: 12 + name 3 + score 4 + strand 1 + thickStart 10 + thickEnd 10 + itemRgb 9 + coverage 10 + pct 2 + a 10 +
 *             b 10 + GQ 3 + FILTER 4 + 11 tabs + NUL — the table's longest line (the contig's name + 111) less the name, less "\t" 10 "\t"
 *             10 "\t", plus 12; pct 100 has a shorter itemRgb and b.  Attained by pos = 2^32 - 1, a CHG / CHH / CHN site, a = b = 4 * 10^9,
 *             phred >= 100 (under BSC_METH_CPG the longest is 99).  BSC_BB_ITEM_MIN = 46: 12 + "CG" + nine one-byte columns
 *             (score, strand, thickStart, thickEnd, coverage, pct, a, b, GQ) + itemRgb "0,255,0" 7 + FILTER 4 + 11 tabs + NUL.  Attained
 *             by pos <= 9, a = 0, b = 1 .. 9, phred <= 9.
 *   PARAMS    bsc_bb_params {items_per_block B: 1 .. 65535, default 512;  reduction: >= 1, default 1024}.
 *   STREAM    of a block call: the items of the call's sites back to back, in order; bigBed blocks carry no header.  Block k holds the
 *             sites of rank [k B, (k + 1) B); only the last block is short.  A block never spans two block calls or two contigs.
 *   PER CALL  one 24-byte struct, bsc_bb_sum {start u32, end u32, count u32, _pad u32 = 0, off u64}, for two arrays:
 *             blocks[n_blocks]: start = the block's first site's start, end = its last site's start + 1, count, off = the block's byte
 *             offset in the stream;  zoom0[n_windows]: the same {start, end, count} for the windows w = start / reduction that hold a
 *             site, ascending, off = 0.  d_totals = four u64 {n_bytes, n_sites, n_blocks, n_windows}.
 *   FILE      bbiFile version 4 in the layout of the bigWig file above, with these
 *             differences: magic 0x8789F2EB in the header and at the end; fieldCount = 15, definedFieldCount = 9; autoSqlOffset names
 *             the NUL-terminated text below, placed behind the total summary; fullDataOffset names a u64 that is the number of ITEMS;
 *             the R-tree has itemsPerSlot = B and one leaf item per block, bounds {tid, start, tid, end}, dataOffset / dataSize the
 *             block's bytes.  Sites are one base wide and never overlap, so the depth is 1 wherever it is not 0: the total summary is
 *             {basesCovered = sites, minVal = 1, maxVal = 1, sumData = sites, sumSquares = sites} (all zero with no site), a zoom record
 *             {chromId, chromStart, chromEnd, validCount = count, 1.0f, 1.0f, (float)count, (float)count}.  The pyramid's levels follow
 *             the bigWig rule unchanged (windows of reduction * 4^l, counts add, level l iff level l - 1 has more than 256 records, at
 *             most 8 levels, 512 records a zoom block, a zoom block never spans contigs).  uncompressBufSize = 0 in a plain file, the
 *             largest raw size of any data or zoom block in a compressed one, where every data block is its ZSTREAM and every zoom
 *             block compress2's at the default level: a raw block must fit a piece, B * BSC_BB_ITEM_MAX <= 0xFF00
 *             (B <= BSC_BB_Z_ITEMS_MAX = 652).  The bytes are UCSC-unpinned, as the bigWig's are.  The autoSql text, lines ending "\n":
 *               table bedMethyl
 *               "Methylation level per cytosine"
 *               (
 *               string chrom; "Reference sequence"
 *               uint chromStart; "Start, 0-based"
 *               uint chromEnd; "End"
 *               string name; "Context: CG, CHG, CHH or CHN"
 *               uint score; "Coverage, capped at 1000"
 *               char[1] strand; "+ or -"
 *               uint thickStart; "Start"
 *               uint thickEnd; "End"
 *               uint reserved; "Colour by level (itemRgb)"
 *               bigint coverage; "Informative reads: non-converted + converted"
 *               uint percent; "Methylation level, percent, rounded half up"
 *               uint nonConverted; "Non-converted reads"
 *               uint converted; "Converted reads"
 *               uint gq; "Phred-scaled genotype quality"
 *               string filter; "FILTER of the call"
 *               )
 * Host (csrc/bigbed.c):
 *   bsc_bb_params_default      {512, 1024}
 *   bsc_bigbed_blocks_recs     the host form over packed records recs[0 .. n), plain C over bsc_meth_format_rec: the stream -> out[cap],
 *                              the summaries -> blocks[] and zoom0[].  *n_blocks and *n_zoom0 hold the ROOM of the two arrays on entry and
 *                              the counts on return.  Where any of the three rooms is too small: BSC_ERR_ARG, the three needs reported and
 *                              nothing written.
 *   bsc_bigbed_open            a writer on a descriptor it may pwrite to (not closed here); names / lens: the BAM header's contigs
 *   bsc_bigbed_add             a call's stream appended (pwrite) and its entries kept.  BSC_ERR_ARG — nothing written — for a tid lower than
 *                              the last or not in the header, a start below the previous end on the same tid, a block other than the last
 *                              whose count is not B, blocks[0].off not 0 or offsets that do not ascend, a block whose bytes (to the next
 *                              offset; the last block's to n_bytes) lie outside count * [BSC_BB_ITEM_MIN, BSC_BB_ITEM_MAX], windows that do
 *                              not hold the blocks' sites.  A window two adds share on one contig merges: the counts add.
 *   bsc_bigbed_add_z           bsc_bigbed_add for a call's ZSTREAMs: every check of bsc_bigbed_add, with raw_bytes — the plain stream's
 *                              length, which the twin bsc_bigwig_add_z can work out from the counts and this one cannot — in n_bytes'
 *                              place; z_sizes[k] is 1 .. the block's raw bytes + 11 and their sum z_bytes; B <= BSC_BB_Z_ITEMS_MAX.  After a
 *                              non-empty bsc_bigbed_add_z a non-empty bsc_bigbed_add is BSC_ERR_ARG with nothing written, and the reverse.
 *   bsc_bigbed_finish          item count, R-tree, zoom levels (deflated with compress2 in a compressed file), total summary, autoSql text,
 *                              header, the closing magic; every write checked (BSC_ERR_ARG with errno's text).  Once.
 *   bsc_bigbed_close           frees the writer (an unfinished file stays without a header: not a bigBed)
 *                              The chromosome tree, the R-tree and the byte buffer are csrc/bbi_trees.h, which csrc/bigwig.c includes too.
 * Device:
 *   bsc_bigbed_sites_device    from d_core[n] / d_aux[n], entry i = position x0 + i (x0 >= 1, x0 + n - 1 < 2^32; the contract of
 *                              bsc_bigwig_sites_device): the stream -> d_out[out_cap] (16-byte aligned), the summaries ->
 *                              d_blocks[blk_cap], d_zoom[zoom_cap] (8-byte aligned), and d_totals.  An array whose room is too small is
 *                              not written at all — the needs are in d_totals, and nothing partial is to be trusted.  Asynchronous on
 *                              `stream`; workspaces of the context (one call in flight per context).
 *   bsc_block_bigbed_kept      the follow-up of the _keep block calls: preconditions and refusals of bsc_block_bigwig_kept; from the
 *                              arrays that block left in HBM, by the chain's emit byte per position, with the block's own x, into buffers
 *                              of its own (room for the most the block can give: its BSC_ERR_ARG for a room too small is unreachable).
 *                              *blocks / *zoom0: the context's host copies, good until the next call.  The kept stream, its tile offsets,
 *                              the methylation tables, bsc_block_csi_kept, the region accumulators and the bigWig buffers are untouched;
 *                              before or after them.  Waits.
 *   bsc_bigbed_stream_read     bytes [off, off + n) of that block's stream -> dst, queued on the context's stream
 * Compressed blocks (csrc/zlibdev.hip):
 *   bsc_zlib_ranges_device     piece k = bytes [offs[k], offs[k + 1]) of d_src (any alignment), d_offs = n_pieces + 1 ascending device
 *                              u64, every length 1 .. max_piece <= 0xFF00: the ZSTREAMs back to back in piece order -> d_out[out_cap],
 *                              their lengths -> d_sizes[sizes_cap] (u32), d_totals = THREE device u64 {bytes out, pieces, ranges whose
 *                              length was 0 or above max_piece}.  A stream is a function of its bytes alone: equal-length ranges give
 *                              bsc_zlib_pieces_device's bytes.  A bad range is clamped in the kernel (its workgroup touches no memory
 *                              outside its buffers; what comes out is then not to be trusted) and counted; the entry waits for the
 *                              count and reports BSC_ERR_ARG when it is not 0.  The most needed: the ranges' bytes + 11 n_pieces.  An
 *                              array whose room is too small is not written at all.  Workspaces of the context.
 *   bsc_block_bigbed_deflate   the follow-up of bsc_block_bigbed_kept of the same block: that call's blocks, by its blocks[].off, one ZSTREAM each
 *                              into a buffer of its own; *z_sizes: the context's host copy of the n_blocks lengths, good until the next call.
 *                              BSC_ERR_ARG without a bsc_block_bigbed_kept before it, or with B > BSC_BB_Z_ITEMS_MAX.  A block with no site:
 *                              0 / 0.  The uncompressed stream and everything bsc_block_bigbed_kept leaves alone are untouched.  Waits.
 *   bsc_bigbed_zstream_read    bytes [off, off + n) of those streams -> dst, queued on the context's stream
 * bam2bcf --meth-bigbed out.bb [--meth-bigbed-items n] [--meth-bigbed-zoom n] [--meth-bigbed-compress] and pipeline.run(bigbed_path=) drive
 * all of it; bs_call_amd/bigbed.py reads the file back by its offsets alone.
 * Not built: the combined-strand (--meth-merge) lines as items, sharded runs, a device encoder for the zoom blocks, the batched and
 * host-buffer block entries.
 */
#define BSC_BB_ITEM_MAX 100u
#define BSC_BB_ITEM_MIN 46u
#define BSC_BB_Z_ITEMS_MAX (0xFF00u / BSC_BB_ITEM_MAX) /* the most items a block of a compressed file may hold */
typedef struct {
  uint32_t items_per_block; /* 1 .. 65535 */
  uint32_t reduction;       /* >= 1: the width of a level-0 zoom window */
} bsc_bb_params;
typedef struct {
  uint32_t start, end, count, _pad;
  uint64_t off;
} bsc_bb_sum;
typedef struct bsc_bigbed bsc_bigbed;
void bsc_bb_params_default(bsc_bb_params *p);
int bsc_bigbed_blocks_recs(const bsc_vcf_rec *recs, size_t n, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bb_params *bb_params,
                           void *out, uint64_t cap, uint64_t *n_bytes, bsc_bb_sum *blocks, uint64_t *n_blocks, bsc_bb_sum *zoom0, uint64_t *n_zoom0);
int bsc_bigbed_open(int fd, uint32_t n_refs, const char *const *names, const uint32_t *lens, const bsc_bb_params *bb_params, bsc_bigbed **bb);
int bsc_bigbed_add(bsc_bigbed *bb, uint32_t tid, const void *data, uint64_t n_bytes, const bsc_bb_sum *blocks, uint64_t n_blocks,
                   const bsc_bb_sum *zoom0, uint64_t n_zoom0);
int bsc_bigbed_add_z(bsc_bigbed *bb, uint32_t tid, const void *zdata, uint64_t z_bytes, const uint32_t *z_sizes, uint64_t raw_bytes,
                     const bsc_bb_sum *blocks, uint64_t n_blocks, const bsc_bb_sum *zoom0, uint64_t n_zoom0);
int bsc_bigbed_finish(bsc_bigbed *bb);
void bsc_bigbed_close(bsc_bigbed *bb);
int bsc_bigbed_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, uint32_t n, uint32_t x0, uint32_t chrom_id,
                            const bsc_meth_params *params, const bsc_bb_params *bb_params, void *d_out, uint64_t out_cap, void *d_blocks,
                            uint64_t blk_cap, void *d_zoom, uint64_t zoom_cap, void *d_totals, void *stream);
int bsc_block_bigbed_kept(bsc_context *ctx, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bb_params *bb_params, uint64_t *n_bytes,
                          uint64_t *n_sites, const bsc_bb_sum **blocks, uint64_t *n_blocks, const bsc_bb_sum **zoom0, uint64_t *n_zoom0);
int bsc_bigbed_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_zlib_ranges_device(bsc_context *ctx, const void *d_src, const void *d_offs, uint32_t n_pieces, uint32_t max_piece, void *d_out,
                           uint64_t out_cap, void *d_sizes, uint64_t sizes_cap, void *d_totals, void *stream);
int bsc_block_bigbed_deflate(bsc_context *ctx, uint64_t *z_bytes, const uint32_t **z_sizes, uint64_t *n_blocks);
int bsc_bigbed_zstream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
/* with bsc_set_profiling: device time (HIP events on the context's stream) of the most recent raw block — bsc_block_records_raw[dev],
 * bsc_block_bcf_raw[dev][_keep] — from its first pre-processing launch to the last launch it queued, the host's wait for the prepared size included */
int bsc_last_raw_block_ms(bsc_context *ctx, float *ms);

/*
 * The variant-only call set (csrc/variantsdev.hip: bsc_var_select_kernel, the context's scan, bsc_var_pack_kernel; csrc/variants.c holds the
 * host form, which is their checker): the records with an ALT allele — about one in a thousand of a WGBS run's records, where every called
 * cytosine is one — as a second stream of the block, encoded by the encoder that made its kept stream.  The reference's users get it from
 * `bcftools view` or gemBS's snpxtr over the whole file; its own `snps` counter counts every record (csrc/sitestats.hip:11-15).  The cost is
 * the selection: a byte per position and a 16-byte head per emitted record; the block's main stream is not read again.
 *
 * VARIANT   A record is a variant when core.emit != 0 — and, in the per-position form where an emit-byte array is given, that position's
 *           byte is != 0 too — and core.alt[0] != 0: the record whose ALT column is not '.'.
 * PARAMS    bsc_var_params {min_phred, pass_only, known_only, reserved}; reserved must be 0 (BSC_ERR_ARG otherwise).  A variant is SELECTED
 *           iff core.phred >= min_phred, and !pass_only || core.flt == 0, and !known_only || rs_found != 0.  rs_found is byte 49 of the aux
 *           half: the dbSNP flag the block was given (snpxtr's mode).  The default is {0, 0, 0, 0}: every variant.
 * SELECTED  The selected records in position order, as packed bsc_vcf_rec (core + aux, 128 bytes), byte for byte as they lie.  Records at
 *           or beyond the count do not exist, whatever their bytes hold.
 * TOTALS    Ten u64 over the selected records: [0] records, [1] snp (alt[1] == 0), [2] multi (alt[1] != 0), [3] het (gt one of 1, 2, 3, 5,
 *           6, 8), [4] passed (flt == 0), [5] known (rs_found != 0), [6] known and passed, [7] transitions, [8] transversions, [9] the sum
 *           of core.phred.  Transitions and transversions are counted for records with alt[1] == 0, ref_code in 1..4 (A, C, G, T) and
 *           alt[0] one of "ACGT" only: the pair {REF, ALT} being {A, G} or {C, T} is a transition, anything else (REF == ALT included) a
 *           transversion; a record with REF N or another ALT byte counts as neither.  Integer sums: no result depends on an order.
 * STREAM    The selected records as encoded by the encoder of the block's kept stream — BCF2 records behind bsc_block_bcf_rawdev_keep, VCF
 *           lines behind bsc_block_vcf_rawdev_keep — with that call's rid or contig, its ids and its names: the concatenation of the
 *           selected records' byte ranges (lines) of the block's full stream.
 *
 *   bsc_var_params_default        {0, 0, 0, 0}
 *   bsc_variants_select_recs      the host form, over packed records (the per-position gate is core.emit alone): out[<= cap] the selected
 *                                 records, *n_out their number, totals (may be NULL).  cap too small: BSC_ERR_ARG, *n_out = the need, the
 *                                 totals filled, nothing written to out.
 *   bsc_variants_sites_device     over the dense per-position arrays d_core[n] / d_aux[n] (16-byte aligned) and d_emit[n], the chain's byte per
 *                                 position, or NULL (core.emit alone gates): d_recs[min(count, max_recs)] packed records (16-byte
 *                                 aligned; records beyond the room are counted, not stored, and nothing is written behind it), *d_n_recs a
 *                                 device u64 = the count — what bsc_bcf_block_device and bsc_vcf_text_block_device take —, d_totals ten
 *                                 device u64.  n = 0 gives zeros.  Asynchronous on `stream`; workspaces of the context's: one call in
 *                                 flight per context.
 *   bsc_block_variants_kept       the follow-up of bsc_block_bcf_rawdev_keep / bsc_block_vcf_rawdev_keep (and of bsc_block_bcf_again behind
 *                                 them): preconditions and refusals of bsc_block_meth_kept.  Select, scan and pack over the arrays that
 *                                 block left in HBM (by the chain's emit byte where the block has one), then the block's own encoder over
 *                                 the packed records into a buffer of the context's own (room: dev_cap bytes), with tile workspaces of its
 *                                 own.  dev_cap too small: BSC_ERR_ARG with *n_bytes = the room needed (*n_records and the totals are
 *                                 filled), and the call may be repeated.  A block with no variant: 0 / 0 and BSC_OK.  The kept stream,
 *                                 its tile offsets and bsc_block_csi_kept, the methylation tables and their index scan, the region
 *                                 accumulators, the bigWig and bigBed data are untouched, before or after; site statistics, bsc_get_stats
 *                                 and the read profile are not counted again.  Waits.
 *   bsc_variants_stream_read      bytes [off, off + n) of that stream -> dst, queued on the context's stream (bsc_meth_stream_read's twin)
 *   bsc_variants_stream_detach    the stream handed over as bsc_meth_stream_detach hands a table over: bsc_detached_read / _wait / _free and
 *                                 bsc_bgzf_write_device serve it; it counts against the four pooled buffers
 *   bsc_block_variants_csi_kept   bsc_block_csi_kept's twin for that stream, BEFORE it is detached: bsc_csi_scan_device with the variant
 *                                 encoder's own 64-record tile offsets as d_sync; the entries go to bsc_csi_add of the variant file's index.
 *                                 The entries stay valid until the next call of this entry on the context.
 * Not built: sharded runs, the batched and host-buffer block entries, a format for the variant stream other than the kept stream's, indels
 * (the caller makes none).
 */
typedef struct {
  uint32_t min_phred; /* selected: core.phred >= min_phred */
  int32_t pass_only;  /* != 0: core.flt == 0 only */
  int32_t known_only; /* != 0: rs_found != 0 only */
  uint32_t reserved;  /* 0 */
} bsc_var_params;
#define BSC_VAR_N_TOTALS 10
void bsc_var_params_default(bsc_var_params *p);
int bsc_variants_select_recs(const bsc_vcf_rec *recs, size_t n, const bsc_var_params *p, bsc_vcf_rec *out, uint64_t cap, uint64_t *n_out,
                             uint64_t totals[10]);
int bsc_variants_sites_device(bsc_context *ctx, const void *d_core, const void *d_aux, const void *d_emit, uint32_t n, const bsc_var_params *p,
                              void *d_recs, uint64_t max_recs, void *d_n_recs, void *d_totals, void *stream);
int bsc_block_variants_kept(bsc_context *ctx, const bsc_var_params *p, uint64_t dev_cap, uint64_t *n_bytes, uint64_t *n_records,
                            uint64_t totals[10]);
int bsc_variants_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_variants_stream_detach(bsc_context *ctx, void **d_stream, uint64_t *n_bytes);
int bsc_block_variants_csi_kept(bsc_context *ctx, int min_shift, const bsc_csi_entry **entries, uint64_t *n_entries, uint64_t *n_records);

/*
 * The read-level CpG concordance table (csrc/cpgreadsdev.hip: the site pass, the context's scan, the walk, the text encoder; csrc/cpgreads.c
 * holds the host form, which is their checker; bs_call_amd/cpgreads.py the Python rule).  Every other output is a function of the
 * per-position records; the pile-up has forgotten which bases came from one molecule.  This table is made from the prepared templates, their
 * read bytes and the block's reference codes while a block call still has them in HBM: per reference CpG how many templates read it methylated
 * and unmethylated, how many of those come from templates that cover enough CpGs to be judged and how many of these are discordant (PDR =
 * d / e), and the 2x2 table of the site with its reference-next CpG (methylation-haplotype blocks, allelic-methylation tests).  The reference
 * has no such output: the rule is this project's own.
 *
 * Inputs    those of bsc_reads_chain_device: prepared templates tpl[nr] (bsc_template), their read bytes seq (seq_bytes of them; a byte is
 *           base | qual << 2, base 0 A, 1 C, 2 G, 3 T), the block x .. y, ref = the reference codes (0 N, 1 .. 4 ACGT) of positions x .. y + 2,
 *           min_qual of the context's bsc_params.  A read k with off[k] + len[k] > seq_bytes is absent (as len[k] == 0).
 * COUNTS    A read byte counts iff min_qual <= byte >> 2 < 63: the pile-up's rule (src/call_genotypes.c:217; accdev.h applies it as a window
 *           test on the byte).
 * SITE      A position p with x <= p <= y, ref(p) == 2 and ref(p + 1) == 3 is a site.  The sites of a block in ascending order are s_0 < s_1
 *           < ...; NEXT(s_i) = s_{i+1}, and the last site has none.  Sites are a property of the reference alone: a site no read covers is
 *           still a site.
 * BYTE(t, q)  For k = 0, then k = 1: if len[k] > 0, pos[k] <= q, q - pos[k] < len[k] (compared in 64 bits) and seq[off[k] + q - pos[k]]
 *           COUNTS, that byte is BYTE(t, q) and the search stops.  A position q < x or q > y has no byte.  If neither read gives one, there is
 *           none.  The first counting byte decides whatever its base.
 * STATE(t, s) for a site at p: bs_strand == 1 (C2T): from BYTE(t, p); base 1 -> M, base 3 -> U, anything else or no byte -> none.
 *           bs_strand == 2 (G2A): from BYTE(t, p + 1); base 2 -> M, base 0 -> U, else none.  Any other bs_strand: none.  So a site at
 *           p == y never has a G2A state.
 * Per template  k_t is the number of sites with a state.  ELIGIBLE iff k_t >= min_sites.  DISCORDANT iff eligible and it has at least one M
 *           and at least one U.
 * Per site, all u32: m, u: templates with state M / U.  e: eligible templates with a state here.  d: discordant templates with a state here.
 *           With n = NEXT(s): dist = n - s, and mm, mu, um, uu count templates whose (STATE(t, s), STATE(t, n)) is (M,M), (M,U), (U,M),
 *           (U,U).  With no next site, dist and the four pair counts are 0.  A site between the two mates of a pair has no state, and the
 *           pair across it is not counted: pairs are reference-neighbours only.
 * RECORD    bsc_cpg_reads_site {pos, dist, m, u, e, d, mm, mu, um, uu}, 40 bytes.  There is one record per SITE of the block in position
 *           order, zero-count sites included.
 * TOTALS    Eight u64: [0] sites, [1] sum of m, [2] sum of u, [3] sum of mm + mu + um + uu, [4] templates with k_t >= 1, [5] eligible
 *           templates, [6] discordant templates, [7] 0 — over every site of the block, stored or not.
 * LINE      A line is written iff m + u >= max(1, min_cov).  Twelve tab-separated plain decimals and '\n':
 *             chrom  start = pos - 1  end = pos + 1  m  u  e  d  dist  mm  mu  um  uu
 *           start and end are those of a --meth-merge line of the same CpG (bsc_meth_cpg_*), so the two tables join on them.  No float is
 *           written anywhere: PDR is d / e, and the reader divides.  contig: 1 .. 255 bytes without tab or newline.  Text totals: {bytes,
 *           lines}.
 * Params    bsc_cpg_reads_params {min_sites, min_cov}, default {4, 1}.  min_sites == 0 is refused with BSC_ERR_ARG.
 * Not gated by the called genotype: a C->T SNP at a reference CpG reads as U; the join with the --meth-merge table (whose lines are
 * genotype-gated) is the user's filter.
 *
 *   bsc_cpg_reads_params_default  {4, 1}
 *   bsc_cpg_reads_sites_host      the host form: sites[<= cap] the records, *n_sites their number (records beyond cap are counted, not stored:
 *                                 BSC_OK all the same), totals (eight u64; may be NULL)
 *   bsc_cpg_reads_format          the lines of sites[n] -> buf.  Returns the length; the length needed, with nothing written, when cap is too
 *                                 small; < 0 for a bad argument.  totals2 (may be NULL): {bytes, lines}
 *   bsc_cpg_reads_device          the same records from device-resident inputs (d_tpl 8-byte aligned, d_ref y - x + 3 codes): d_sites[min(count,
 *                                 sites_cap)] (8-byte aligned; nothing is written behind the room), *d_n_sites a device u64 = the count, d_totals
 *                                 eight device u64.  Integer atomic adds alone: the bytes are a function of the input.  Asynchronous on
 *                                 `stream`; workspaces of the context's, grow-only: one call in flight per context.  A refusal writes nothing.
 *   bsc_cpg_reads_text_device     the lines of d_sites[min(*d_n_sites, max_sites)] -> d_out[<= out_cap] (16-byte aligned).  d_totals2: two device
 *                                 u64 {bytes, lines}.  A stream longer than out_cap is cut at a 64-record boundary and its full length is
 *                                 still reported, as the other text encoders do.
 *   bsc_block_cpg_reads_kept      the follow-up of bsc_block_bcf_rawdev_keep / bsc_block_vcf_rawdev_keep (and of bsc_block_bcf_again behind
 *                                 them): preconditions and refusals of bsc_block_meth_kept.  Reads the prepared templates, reads and
 *                                 reference codes that block left in HBM — nothing queued behind the pre-processing writes to them — and
 *                                 writes the table into a buffer of the context's own (room: dev_cap bytes).  dev_cap too small: BSC_ERR_ARG
 *                                 with *n_bytes = the room needed (the totals are filled), and the call may be repeated.  A block with no
 *                                 template gives its zero-count sites: no line.  The kept stream, its tile offsets and bsc_block_csi_kept,
 *                                 the methylation tables, the region accumulators, the bigWig and bigBed data and the variant selection are
 *                                 untouched, before or after.  Waits.
 *   bsc_cpg_reads_stream_read     bytes [off, off + n) of that table -> dst, queued on the context's stream (bsc_meth_stream_read's twin)
 *   bsc_cpg_reads_stream_detach   the table handed over as bsc_meth_stream_detach hands one over: bsc_detached_read / _wait / _free and
 *                                 bsc_bgzf_write_device serve it; it counts against the four pooled buffers
 * Not built: a tabix index of the table, sharded runs, the batched and host-buffer block entries, non-CpG contexts, pairs beyond the
 * reference-next site (the epiallele table below has the patterns of four consecutive sites), any float statistic of the 2x2 table.
 */
typedef struct {
  uint32_t pos, dist, m, u, e, d, mm, mu, um, uu;
} bsc_cpg_reads_site;
typedef struct {
  uint32_t min_sites; /* ELIGIBLE: k_t >= min_sites; 0 is refused */
  uint32_t min_cov;   /* LINE: m + u >= max(1, min_cov) */
} bsc_cpg_reads_params;
#define BSC_CPG_READS_N_TOTALS 8
void bsc_cpg_reads_params_default(bsc_cpg_reads_params *p);
int bsc_cpg_reads_sites_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                             int32_t min_qual, const bsc_cpg_reads_params *p, bsc_cpg_reads_site *sites, uint64_t cap, uint64_t *n_sites,
                             uint64_t totals[8]);
long bsc_cpg_reads_format(const char *contig, const bsc_cpg_reads_site *sites, size_t n, const bsc_cpg_reads_params *p, char *buf, size_t cap,
                          uint64_t totals2[2]);
int bsc_cpg_reads_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x, uint32_t y,
                         const void *d_ref, const bsc_cpg_reads_params *p, void *d_sites, uint64_t sites_cap, void *d_n_sites, void *d_totals,
                         void *stream);
int bsc_cpg_reads_text_device(bsc_context *ctx, const void *d_sites, const void *d_n_sites, uint64_t max_sites, const char *contig,
                              const bsc_cpg_reads_params *p, void *d_out, uint64_t out_cap, void *d_totals2, void *stream);
int bsc_block_cpg_reads_kept(bsc_context *ctx, const char *contig, const bsc_cpg_reads_params *p, uint64_t dev_cap, uint64_t *n_bytes,
                             uint64_t *n_lines, uint64_t totals[8]);
int bsc_cpg_reads_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_cpg_reads_stream_detach(bsc_context *ctx, void **d_stream, uint64_t *n_bytes);

/*
 * The allele-specific methylation table (csrc/asmdev.hip: the SNP pass, the windows, the records' heads, the walk, Fisher's test, the text
 * encoder; csrc/asm.c holds the host form, which is their checker; bs_call_amd/asm.py the Python rule).  The caller decides genotype and
 * methylation from the same reads; this is the output that uses both: for a heterozygous SNP the caller wrote and a reference CpG near it, do the
 * templates that carry allele 1 read the CpG differently from those that carry allele 2 (imprinting, cis-acting variants)?  It is made while a
 * block call still has the dense per-position records, the prepared templates, their read bytes and the reference codes in HBM.  The
 * reference has no such output: the rule is this project's own.
 *
 * Inputs    those of the read-level CpG table (tpl[nr], seq, x .. y, ref = the codes of x .. y + 2, min_qual), and core = the y - x + 1
 *           bsc_vcf_core records of the block with, optionally, emit = a byte per position (the chain's emit bytes: bsc_variants_sites_device
 *           has the same pair).  COUNTS, SITE, BYTE(t, q) and STATE(t, s) are those of the read-level CpG table, verbatim.
 * SNP       A position h in x .. y is a SNP when core[h - x].emit != 0 and, where the emit bytes are given, emit[h - x] != 0; gt is one of 1, 2,
 *           3, 5, 6, 8 (AC, AG, AT, CG, CT, GT: allele 1 is the first letter, allele 2 the second); phred >= min_phred; and !pass_only or
 *           flt == 0.
 * ALLELE(t, h)  0 (none), 1 or 2.  bs_strand other than 1 or 2: 0.  bs_strand == 1 and gt == 6 (CT): 0 — on a C2T template a C/T SNP cannot be
 *           told from conversion, and counting its unconverted Cs alone would bias the table.  bs_strand == 2 and gt == 2 (AG): 0, for the same
 *           reason.  Otherwise with b the base of BYTE(t, h) (no byte: 0), the genome bases b may stand for are, on a C2T template, {C, T} for a
 *           read T and {b} for any other base; on a G2A template {G, A} for a read A and {b} for any other.  If exactly one of the two alleles
 *           is in that set, ALLELE is its number; otherwise 0.
 * WINDOW    With W = max_dist the sites of h are the sites s with max(x, h - W) <= s <= min(y, h + W), computed in 64 bits (h - W below 0 is
 *           0), in ascending order, the sites no read covers included.  A site with h == s or h == s + 1 is in the window but OVERLAPPED: the
 *           SNP makes or unmakes the CpG on one allele, and the site never has a state for this SNP.
 * RECORD    bsc_asm_pair {snp_pos, cpg_pos, m1, u1, m2, u2, aq, info}, eight u32, 32 bytes: one per (SNP, window site), ordered by SNP position,
 *           then by site position.  m1: templates with ALLELE(t, h) == 1 and STATE(t, s) == M; u1, m2, u2 alike.  info = gt | flags << 8: flag 1
 *           OVERLAPPED (the counts stay 0), flag 2 DEEP: m1 + u1 + m2 + u2 > 46340 — beyond that the `int` products of the reference's Fisher
 *           test (src/stats_utils.c:25-91) leave 31 bits.
 * AQ        0 for an OVERLAPPED or DEEP record.  Otherwise z = Fisher's two-sided p of the table {c0, c1, c2, c3} = {m1, u1, m2, u2} by the
 *           statements of fisher_dev (csrc/callmath.h), with one addition: a point term exp(arg) is 0.0 when arg < -700.0 (such a term is below
 *           1e-304 and cannot change a z >= 1e-100 in the last bit, so no result depends on how exp underflows or on flushed subnormals), and
 *           aq = z >= 1e-100 ? (uint32_t)(int)(-(log(z) / ln 10) * 10.0 + 0.5) : 1000 — the form FS has.  No float is written anywhere.
 * TOTALS    Eight u64: [0] SNPs, [1] records, [2] (template, SNP) observations with ALLELE != 0, [3] of them those with allele 1, [4] the sum
 *           of m1 + u1 + m2 + u2, [5] DEEP records, [6], [7] 0.  [0] .. [4] run over every record, stored or not; DEEP is a property of a
 *           record's counts, which exist only where the record is stored: [5] runs over the stored records.
 * LINE      A line is written iff the record is neither OVERLAPPED nor DEEP and m1 + u1 >= c and m2 + u2 >= c, c = max(1, min_cov).  Eleven
 *           tab-separated fields and '\n':
 *             chrom  start = cpg_pos - 1  end = cpg_pos + 1  snp_pos  gt  m1  u1  m2  u2  aq  dist
 *           gt is the genotype's two letters (a gt byte above 9: NN), dist = cpg_pos - snp_pos as a signed decimal.  start and end are those of
 *           the --meth-merge and --meth-reads lines of the same CpG: the three tables join on them.  Lines are ordered by SNP, then by site —
 *           NOT by start: windows of neighbouring SNPs overlap.  No index is built.  Text totals: {bytes, lines}.
 * Params    bsc_asm_params {min_phred, pass_only, max_dist, min_cov}, default {20, 0, 500, 2}.  max_dist outside 1 .. 65535 is refused with
 *           BSC_ERR_ARG; more than 2^32 - 1 records in a block with BSC_ERR_RANGE.
 * No template spans two blocks (a block ends at a coverage gap): nothing is lost at block borders.
 *
 *   bsc_asm_params_default     {20, 0, 500, 2}
 *   bsc_asm_pairs_host         the host form: pairs[<= cap] the records, *n_pairs their number (records beyond cap are counted, not stored:
 *                              BSC_OK all the same), totals (eight u64; may be NULL).  emit may be NULL.  lfact_256: ln k! for k = 0 .. 255
 *                              (bsc_get_tables)
 *   bsc_asm_format             the lines of pairs[n] -> buf.  Returns the length; the length needed, with nothing written, when cap is too small;
 *                              < 0 for a bad argument.  totals2 (may be NULL): {bytes, lines}
 *   bsc_asm_fisher_p           z of AQ for one table {c0, c1, c2, c3} (each >= 0, their sum <= 46340), the clamp included: the host form's
 *                              Fisher test on its own, which the tests compare with the reference's.  -1.0 for a table outside that range
 *   bsc_asm_device             the same records from device-resident inputs (d_tpl 8-byte, d_core 16-byte aligned, d_ref y - x + 3 codes, d_emit
 *                              y - x + 1 bytes or NULL): d_pairs[min(count, pairs_cap)] (8-byte aligned; nothing is written behind the room),
 *                              *d_n_pairs a device u64 = the count, d_totals eight device u64.  Integer atomic adds alone: the bytes are a function
 *                              of the input.  Queued on `stream`, on which it waits twice for a count (the SNPs, the records) before the records
 *                              are made; workspaces of the context's, grow-only: one call in flight per context.  A refusal writes nothing.
 *   bsc_asm_text_device        the lines of d_pairs[min(*d_n_pairs, max_pairs)] -> d_out[<= out_cap] (16-byte aligned).  d_totals2: two device
 *                              u64 {bytes, lines}.  A stream longer than out_cap is cut at a 64-record boundary and its full length is still
 *                              reported, as the other text encoders do.
 *   bsc_block_asm_kept         the follow-up of bsc_block_bcf_rawdev_keep / bsc_block_vcf_rawdev_keep (and of bsc_block_bcf_again behind them):
 *                              the preconditions of bsc_block_cpg_reads_kept and bsc_block_variants_kept together.  Reads the dense records and
 *                              emit bytes, the prepared templates, reads and reference codes that block left in HBM and writes the table into a
 *                              buffer of the context's own (room: dev_cap bytes).  dev_cap too small: BSC_ERR_ARG with *n_bytes = the room
 *                              needed (the totals are filled), and the call may be repeated.  The kept stream, its tile offsets and
 *                              bsc_block_csi_kept, the methylation tables, the region accumulators, the bigWig and bigBed data, the variant
 *                              selection and the read-level CpG table are untouched, before or after.  Waits.
 *   bsc_asm_stream_read        bytes [off, off + n) of that table -> dst, queued on the context's stream (bsc_meth_stream_read's twin)
 *   bsc_asm_stream_detach      the table handed over as bsc_meth_stream_detach hands one over: bsc_detached_read / _wait / _free and
 *                              bsc_bgzf_write_device serve it; it counts against the four pooled buffers
 * Not built: sharded runs, the batched and host-buffer block entries, non-CpG contexts, a per-SNP aggregate, multiple-testing correction,
 * phasing across SNPs.
 */
typedef struct {
  uint32_t snp_pos, cpg_pos, m1, u1, m2, u2, aq, info;
} bsc_asm_pair;
typedef struct {
  uint32_t min_phred; /* SNP: phred >= min_phred */
  int32_t pass_only;  /* SNP: flt == 0 */
  uint32_t max_dist;  /* WINDOW: W, 1 .. 65535 */
  uint32_t min_cov;   /* LINE: m1 + u1 and m2 + u2 >= max(1, min_cov) */
} bsc_asm_params;
#define BSC_ASM_N_TOTALS 8
#define BSC_ASM_OVERLAPPED 1u
#define BSC_ASM_DEEP 2u
void bsc_asm_params_default(bsc_asm_params *p);
int bsc_asm_pairs_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                       int32_t min_qual, const bsc_vcf_core *core, const uint8_t *emit, const double *lfact_256, const bsc_asm_params *p,
                       bsc_asm_pair *pairs, uint64_t cap, uint64_t *n_pairs, uint64_t totals[8]);
long bsc_asm_format(const char *contig, const bsc_asm_pair *pairs, size_t n, const bsc_asm_params *p, char *buf, size_t cap, uint64_t totals2[2]);
double bsc_asm_fisher_p(const int32_t c[4], const double *lfact_256);
int bsc_asm_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const void *d_ref,
                   const void *d_core, const void *d_emit, const bsc_asm_params *p, void *d_pairs, uint64_t pairs_cap, void *d_n_pairs,
                   void *d_totals, void *stream);
int bsc_asm_text_device(bsc_context *ctx, const void *d_pairs, const void *d_n_pairs, uint64_t max_pairs, const char *contig, const bsc_asm_params *p,
                        void *d_out, uint64_t out_cap, void *d_totals2, void *stream);
int bsc_block_asm_kept(bsc_context *ctx, const char *contig, const bsc_asm_params *p, uint64_t dev_cap, uint64_t *n_bytes, uint64_t *n_lines,
                       uint64_t totals[8]);
int bsc_asm_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_asm_stream_detach(bsc_context *ctx, void **d_stream, uint64_t *n_bytes);

/*
 * The M-bias table (csrc/mbiasdev.hip: one walk over the RAW templates; csrc/mbias.c holds the host form, which is its checker;
 * bs_call_amd/mbias.py the Python rule): methylated and unmethylated calls per sequencing cycle, split by read 1 / read 2, by bisulfite
 * strand and by CpG / CHG / CHH — the curve from which the fixed trims (bsc_prep_params.left_trim / right_trim) and the under-conversion
 * rate (the CHH level) are chosen.  It is the one output made from the templates as the reader leaves them, before the pre-processing.
 * The reference has no such output: the rule is this project's own.
 *
 * Inputs    raw[nr] (bsc_raw_template), their read bytes seq (seq_bytes; a byte is base | qual << 2, base 0..3 = ACGT) and their mismatch
 *           lists misms[n_misms] (bsc_misms); the block x .. y; ref = the reference codes (0 N, 1..4 ACGT) of positions x .. y + 2, as
 *           bsc_block_*_rawdev take them; min_qual of the context's bsc_params; bsc_mbias_params {n_cycles}, default {512}, values outside
 *           1 .. BSC_MBIAS_MAX_CYCLES (1024) refused with BSC_ERR_ARG.  bsc_prep_params is NOT an input: the table shows the reads as
 *           sequenced, so that the trims can be chosen from it.
 * READ      Read k of template t is walked iff len[k] > 0, off[k] + len[k] <= seq_bytes, misms_off[k] + n_misms[k] <= n_misms (both sums
 *           in 64 bits, without wrapping), bs_strand is 1 or 2, orientation <= 1 and its list is not malformed (G below).  Otherwise it is
 *           skipped and counted in totals[6] — except that a read of a template with bs_strand == 0, and a read with len[k] == 0, are
 *           skipped without being counted anywhere.
 * END       e = k ^ orientation: 0 = read 1, 1 = read 2 (the mapping csrc/prep.c uses for the fixed trims: read[0] is R1 on a FORWARD
 *           template).
 * CYCLE     Read[0] is the forward-aligned read; read[1] is stored in reference orientation, as BAM stores it.  Byte j has the 0-based
 *           cycle c = j for k == 0 and c = len[k] - 1 - j for k == 1.  Soft-clipped bytes keep their cycles.  Hard-clipped bases are not
 *           in seq: they are ignored, and the cycles of a hard-clipped read start behind them.
 * G(j)      The genome position of byte j, from the list, in the convention of csrc/prep.c (its naming: CIGAR D -> BSC_MISMS_INS, CIGAR I
 *           -> BSC_MISMS_DEL; `position` is an offset in the read as stored, soft clip included).  pos[k] is the position of the first
 *           byte that is not soft-clipped.  The entries z = 0 .. n_misms[k] - 1 are walked in order with a read cursor that starts at 0:
 *             BSC_MISMS_MISMS   ignored altogether.
 *             SOFT, DEL         take the `size` bytes position .. position + size - 1 out of the mapping: they have no G.  The cursor becomes
 *                               position + size.
 *             INS               adds `size` to the genome offset of every byte at or behind `position`.  The cursor becomes position.
 *           The list is malformed if an entry's position is below the cursor; if a DEL or SOFT entry has position + size > len[k]; if a
 *           SOFT entry is neither entry 0 nor entry n_misms[k] - 1; or if an entry's type is none of the four.  A malformed list skips
 *           the whole read (totals[6]).  For a byte j that is not taken out,
 *             G(j) = pos[k] + (bytes i < j that are not taken out) + (the sizes of the INS entries with position <= j), in 64 bits.
 *           A byte with G < x or G > y has no G.  The device never indexes outside seq, misms or ref, whatever the list holds.
 * COUNTS    A byte counts iff min_qual <= byte >> 2 < 63: the pile-up's rule, the same as the read-level CpG table's.
 * CONTEXT   r(p) = the reference code of p, and N for p outside x .. y + 2.  For a counting byte with a G:
 *           bs_strand == 1 (C2T): a bin exists iff r(G) == C.  With n1 = r(G + 1), n2 = r(G + 2): CpG iff n1 == G; CHG iff n1 is A, C or T
 *           and n2 == G; CHH iff n1 and n2 are each A, C or T; an N that is needed gives no bin.  State: base C -> meth, base T -> unmeth,
 *           anything else -> none.
 *           bs_strand == 2 (G2A): a bin exists iff r(G) == G.  With p1 = r(G - 1), p2 = r(G - 2): CpG iff p1 == C; CHG iff p1 is A, G or T
 *           and p2 == C; CHH iff p1 and p2 are each A, G or T.  State: base G -> meth, base A -> unmeth.
 *           The table depends on the block cut only through r() being N outside the block.
 * TABLE     counts[e][s][ctx][c][state], u64: s = bs_strand - 1, ctx 0 CpG / 1 CHG / 2 CHH, c < n_cycles, state 0 meth / 1 unmeth —
 *           BSC_MBIAS_N_BINS (12) x n_cycles x 2 cells.  A counting byte with a bin and a state and c >= n_cycles goes to totals[3] and to
 *           no cell.  Mate overlap is NOT removed: both mates count where they overlap.
 * TOTALS    Eight u64: [0] reads walked, [1] bytes with a G, [2] bytes added to a cell, [3] overflow (above), [4] sum of meth over the CpG
 *           cells, [5] sum of unmeth over the CpG cells, [6] reads skipped, [7] 0.
 * LINE      The first line is "#read\tstrand\tcontext\tcycle\tmeth\tunmeth\n".  Then for e in 0, 1, s in 0, 1, ctx in 0, 1, 2 the cycles
 *           0 .. L(e), L(e) = the highest cycle at which any cell of end e is non-zero; an end with no count writes no line.  Columns: 1|2,
 *           C2T|G2A, CpG|CHG|CHH, cycle + 1, and the two counts as plain decimals, tab separated, '\n'.  Lines inside the range with two
 *           zeros are written (the reader plots them).  No float is written anywhere.
 *
 *   bsc_mbias_params_default   {512}
 *   bsc_mbias_host             the host form, a plain loop: ADDS into counts[12 * n_cycles * 2] and totals[8] (neither is zeroed here, as
 *                              bsc_meth_regions_sum_recs adds; totals may be NULL)
 *   bsc_mbias_format           the table's text -> buf.  Returns the length; the length needed, with nothing written, when cap is too small;
 *                              < 0 for a bad argument
 *   bsc_mbias_device           the same walk over device-resident inputs (d_raw 8-byte, d_misms 4-byte aligned; d_ref y - x + 3 codes): ADDS
 *                              into the caller's device table d_counts (12 * n_cycles * 2 u64) and d_totals (eight u64), both 8-byte aligned.
 *                              Integer atomic adds alone: the bytes are a function of the input.  Asynchronous on `stream`; no workspace.  A
 *                              refusal writes nothing.
 *   bsc_block_mbias_rawdev     the follow-up of bsc_block_bcf_rawdev_keep / bsc_block_vcf_rawdev_keep on the SAME raw pointers, called before
 *                              the reader's next block: x, y and the reference codes are those the block call left in HBM, and the
 *                              refusals are bsc_block_cpg_reads_kept's when they are gone.  Adds into an accumulator of the context's own,
 *                              made at the first call; a different n_cycles before bsc_mbias_reset is BSC_ERR_ARG.  totals (may be NULL):
 *                              the accumulator's totals so far.  Everything else the context keeps is untouched, before or after.  Waits.
 *   bsc_mbias_read             the accumulator -> counts_host[12 * n_cycles * 2] (may be NULL) and totals[8] (may be NULL), n_cycles that of
 *                              the calls that made it.  BSC_ERR_ARG, with nothing written, while there is none.  Waits.
 *   bsc_mbias_reset            drops the accumulator
 * NOT built: suggested trim bounds, a plot, the table in the JSON report (whose layout follows the reference), sharded runs, removal of the
 * mate overlap, a tabix index.
 */
typedef struct {
  uint32_t n_cycles; /* 1 .. BSC_MBIAS_MAX_CYCLES */
} bsc_mbias_params;
#define BSC_MBIAS_MAX_CYCLES 1024u
#define BSC_MBIAS_N_BINS 12u
#define BSC_MBIAS_N_TOTALS 8
void bsc_mbias_params_default(bsc_mbias_params *p);
int bsc_mbias_host(const bsc_raw_template *raw, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, const bsc_misms *misms, uint64_t n_misms,
                   uint32_t x, uint32_t y, const uint8_t *ref, int32_t min_qual, const bsc_mbias_params *p, uint64_t *counts, uint64_t totals[8]);
long bsc_mbias_format(const uint64_t *counts, const bsc_mbias_params *p, char *buf, size_t cap);
int bsc_mbias_device(bsc_context *ctx, const void *d_raw, uint32_t nr, const void *d_seq, uint64_t seq_bytes, const void *d_misms, uint64_t n_misms,
                     uint32_t x, uint32_t y, const void *d_ref, const bsc_mbias_params *p, void *d_counts, void *d_totals, void *stream);
int bsc_block_mbias_rawdev(bsc_context *ctx, const void *d_raw, uint32_t nr, const void *d_seq, uint64_t seq_bytes, const void *d_misms,
                           uint64_t n_misms, const bsc_mbias_params *p, uint64_t totals[8]);
int bsc_mbias_read(bsc_context *ctx, uint64_t *counts_host, uint64_t totals[8]);
int bsc_mbias_reset(bsc_context *ctx);

/*
 * The epiallele table (csrc/epidev.hip: the records' heads, the walk, the text encoder, behind the site pass and the scan of
 * csrc/cpgreadsdev.hip; csrc/epi.c holds the host form, which is their checker; bs_call_amd/epialleles.py the Python rule).  Per window of
 * four consecutive reference CpGs, how many templates show each of the 16 methylation patterns: what methclone, epipolymorphism,
 * methylation entropy and the methylation-haplotype load start from.  The read-level CpG table stops at pairs, and a 2x2 table of neighbours
 * cannot be turned into 4-site patterns afterwards; this one is made from the same prepared templates while they are in HBM.  The reference
 * has no such output: the rule is this project's own.
 *
 * COUNTS, SITE, BYTE(t, q) and STATE(t, s) are those of the read-level CpG table above, word for word, and the inputs are those of
 * bsc_cpg_reads_device.
 * WINDOW    With the block's sites s_0 < s_1 < ... < s_{S-1}, window i (0 <= i <= S - 4) is (s_i, s_{i+1}, s_{i+2}, s_{i+3}).  K = 4 is a
 *           constant of this table (BSC_EPI_K), not a parameter.  A block with S < 4 has no window.  Windows are a property of the reference
 *           alone: a window no template reads is still a window.  Windows never cross a block, as NEXT does not.
 * PATTERN(t, i)  is defined iff STATE(t, s_{i+j}) != none for all j = 0 .. 3.  Its code is the sum over j of [STATE(t, s_{i+j}) == M] << j:
 *           code 0 = UUUU, 15 = MMMM, and bit 0 is the leftmost site.  A template gives at most one pattern per window, mates included:
 *           BYTE already lets the first read win in an overlap.  A site in the gap between mates has no state, so no window containing
 *           that site gets a pattern from that template.
 * RECORD    bsc_epi_window {pos, span, c[16]}, 72 bytes, 8-byte aligned.  pos = s_i and span = s_{i+3} - s_i.  c[code] is the number of
 *           templates with that pattern.  There is one record per window in position order, zero-count windows included.
 * TOTALS    Eight u64, over every window whether stored or not: [0] windows, [1] the sum over all windows and codes of c, [2] templates
 *           that gave at least one pattern, [3] the sum over observations of popcount(code), [4] templates with k_t >= 4 (k_t: the number
 *           of sites with a state, as in the read-level table), [5 .. 7] 0.
 * LINE      With n = the sum of c (64 bits) and k = the number of codes with c > 0, a line is written iff n >= max(1, min_cov).  Twenty
 *           tab-separated plain decimals and '\n':
 *             chrom  start = pos - 1  end = pos + span + 1  n  k  c0 ... c15
 *           start is the start of the --meth-merge and --meth-reads lines of the window's first CpG, so the tables join.  No float is
 *           written: epipolymorphism is 1 - sum c^2 / n^2 and entropy is - sum (c / n) log2 (c / n); the reader computes them.  contig:
 *           1 .. 255 bytes without tab or newline.  Text totals: {bytes, lines}.
 * Params    bsc_epi_params {min_cov, reserved}, default {10, 0}.  reserved != 0 is refused with BSC_ERR_ARG.
 * Not gated by the called genotype, as the read-level table is not.
 *
 *   bsc_epi_params_default   {10, 0}
 *   bsc_epi_windows_host     the host form: win[<= cap] the records, *n_win their number (records beyond cap are counted, not stored: BSC_OK
 *                            all the same), totals (eight u64; may be NULL)
 *   bsc_epi_format           the lines of win[n] -> buf.  Returns the length; the length needed, with nothing written, when cap is too
 *                            small; < 0 for a bad argument.  totals2 (may be NULL): {bytes, lines}
 *   bsc_epi_device           the same records from device-resident inputs (d_tpl 8-byte aligned, d_ref y - x + 3 codes): d_win[min(count,
 *                            win_cap)] (8-byte aligned; nothing is written behind the room), *d_n_win a device u64 = the count, d_totals
 *                            eight device u64.  Integer atomic adds alone: the bytes are a function of the input.  Asynchronous on
 *                            `stream`; workspaces of the context's (the site masks are the read-level table's), grow-only: one call in
 *                            flight per context.  A refusal writes nothing.
 *   bsc_epi_text_device      the lines of d_win[min(*d_n_win, max_win)] -> d_out[<= out_cap] (16-byte aligned).  d_totals2: two device u64
 *                            {bytes, lines}.  A stream longer than out_cap is cut at a 64-record boundary and its full length is still
 *                            reported, as the other text encoders do.
 *   bsc_block_epi_kept       the twin of bsc_block_cpg_reads_kept, with its preconditions and refusals: walks the prepared templates, reads
 *                            and reference codes the last *_keep call left in HBM and writes the table into a buffer of the context's own
 *                            (room: dev_cap bytes).  dev_cap too small: BSC_ERR_ARG with *n_bytes = the room needed (the totals are
 *                            filled), and the call may be repeated.  Every other kept output — the kept stream, its index entries, the
 *                            methylation, read-level and allele-specific tables — is untouched, before or after.  Waits.
 *   bsc_epi_stream_read      bytes [off, off + n) of that table -> dst, queued on the context's stream
 *   bsc_epi_stream_detach    the table handed over as bsc_cpg_reads_stream_detach hands one over: bsc_detached_read / _wait / _free and
 *                            bsc_bgzf_write_device serve it; it counts against the four pooled buffers
 * Not built: K != 4 (the pattern table below has every template's whole string), non-CpG contexts, sharded runs, the batched and host-buffer
 * block entries, a tabix index of the table, float columns.
 */
#define BSC_EPI_K 4
typedef struct {
  uint32_t pos;   /* s_i */
  uint32_t span;  /* s_{i+3} - s_i */
  uint32_t c[16]; /* templates per pattern code */
} bsc_epi_window;
typedef struct {
  uint32_t min_cov;  /* LINE: n >= max(1, min_cov) */
  uint32_t reserved; /* 0; anything else is refused */
} bsc_epi_params;
#define BSC_EPI_N_TOTALS 8
void bsc_epi_params_default(bsc_epi_params *p);
int bsc_epi_windows_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                         int32_t min_qual, const bsc_epi_params *p, bsc_epi_window *win, uint64_t cap, uint64_t *n_win, uint64_t totals[8]);
long bsc_epi_format(const char *contig, const bsc_epi_window *win, size_t n, const bsc_epi_params *p, char *buf, size_t cap, uint64_t totals2[2]);
int bsc_epi_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const void *d_ref,
                   const bsc_epi_params *p, void *d_win, uint64_t win_cap, void *d_n_win, void *d_totals, void *stream);
int bsc_epi_text_device(bsc_context *ctx, const void *d_win, const void *d_n_win, uint64_t max_win, const char *contig, const bsc_epi_params *p,
                        void *d_out, uint64_t out_cap, void *d_totals2, void *stream);
int bsc_block_epi_kept(bsc_context *ctx, const char *contig, const bsc_epi_params *p, uint64_t dev_cap, uint64_t *n_bytes, uint64_t *n_lines,
                       uint64_t totals[8]);
int bsc_epi_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_epi_stream_detach(bsc_context *ctx, void **d_stream, uint64_t *n_bytes);

/*
 * The per-read CpG pattern table, PAT (csrc/patdev.hip: the slot pass, the walk, the heads and the text encoder, behind the site pass and the
 * scan of csrc/cpgreadsdev.hip, with the radix sort of csrc/sort.hip between walk and heads; csrc/pat.c holds the host form, which is their
 * checker; bs_call_amd/pat.py the Python rule).  For every template the string of methylated / unmethylated calls over the reference CpGs it
 * covers, identical strings collapsed and counted: `chrom  CpG-index  pattern  count`, patterns in C / T / ., lines sorted by index, then
 * pattern — the interchange format of the read-level methylation tools (wgbstools and what is built on it).  It is the general form of the
 * read-level table's pairs and of the epiallele table's K = 4.  The bytes are WGBSTOOLS-UNPINNED: no copy of that tool is at hand, the format
 * is written from its description.  wgbstools counts CpGs genome-wide; this table's index is the CpG's 1-based ordinal within its CONTIG
 * (bs_call_amd/pat.py has contig_offsets(fasta) and shift(lines, offset) to convert).  The reference has no such output: the rule is this
 * project's own.
 *
 * COUNTS, SITE, BYTE(t, q) and STATE(t, s) are those of the read-level CpG table above, word for word, and the inputs are those of
 * bsc_cpg_reads_device.
 * ORDINAL   The block's sites in ascending order are s_0 < ... < s_{S-1}; the ordinal of s_i is i.
 * PATTERN(t)  Let f and l be the first and last ordinals at which template t has a state and k_t the number of sites with a state.  No line
 *           unless k_t >= max(1, min_sites).  The template's string has l - f + 1 characters: character j is 'C' where STATE(t, s_{f+j}) is
 *           M, 'T' where it is U and '.' where there is none (a site in a mate gap, a low quality, another base, an overlap: BYTE's rule).
 * PIECES    A line holds at most BSC_PAT_MAX_SITES = 64 sites, so that a record has a fixed size: the string is cut after every 64th
 *           character counted from f, each piece is trimmed to its own first and last non-'.' character, a piece with no state gives
 *           nothing, and a piece's index is the ordinal of its first remaining site.  min_sites is judged on the template, not on a piece.
 *           A template of at most 64 spanned sites is one piece.  The cut is a limit of this table: a longer molecule's string is spread
 *           over several lines.
 * RECORD    bsc_pat_rec {idx, count, hi, lo}, 24 bytes, 8-byte aligned.  Site j of the piece sits in bits 127 - 2j and 126 - 2j of hi:lo,
 *           codes 1 '.', 2 'C', 3 'T' and 0 behind the last site: the integer order of (idx, hi, lo) is the order of
 *           `LC_ALL=C sort -k2,2n -k3,3` on the lines.  One record per distinct (idx, hi, lo) of the block, in that order; count = the
 *           pieces that share the key.  A block whose pieces (on the device: whose slots, one per started 64 sites of a template's span)
 *           exceed 2^32 - 1 is refused with BSC_ERR_RANGE.
 * TOTALS    Eight u64, over every record whether stored or not: [0] records, [1] the sum of count (= pieces), [2] templates that gave a
 *           line, [3] / [4] / [5] the sum of 'C' / 'T' / '.' over pieces, [6] templates cut into more than one piece (l - f + 1 > 64), [7] S.
 * LINE      chrom \t index_base + idx + 1 \t pattern \t count \n.  index_base (u64; above 2^63 is refused) is the number of sites of the
 *           contig in front of the block's first position, so that the index is the CpG's 1-based ordinal within its contig.  contig: 1 ..
 *           255 bytes without tab or newline.  Text totals: {bytes, lines}.
 * Params    bsc_pat_params {min_sites, reserved}, default {1, 0}.  reserved != 0 is refused with BSC_ERR_ARG.
 * Not gated by the called genotype, as the read-level table is not.
 *
 *   bsc_pat_params_default   {1, 0}
 *   bsc_pat_count_sites      host: *n = the sites p with from <= p < to (positions, 1 first; from >= 1) over a contig's codes as
 *                            bsc_fasta_contig gives them.  A C at the contig's last position is no site.  The running index_base of a file.
 *   bsc_pat_recs_host        the host form (qsort): rec[<= cap] the records, *n_rec their number (records beyond cap are counted, not
 *                            stored: BSC_OK all the same), totals (eight u64; may be NULL)
 *   bsc_pat_format           the lines of rec[n] -> buf.  Returns the length; the length needed, with nothing written, when cap is too
 *                            small; < 0 for a bad argument.  totals2 (may be NULL): {bytes, lines}.  p is checked; no field of it changes a line
 *   bsc_pat_device           the same records from device-resident inputs (d_tpl 8-byte aligned, d_ref y - x + 3 codes): d_rec[min(count,
 *                            rec_cap)] (8-byte aligned; nothing is written behind the room), *d_n_rec a device u64 = the count, d_totals
 *                            eight device u64.  Integer atomic adds alone, and equal keys are indistinguishable: the bytes are a function
 *                            of the input.  Everything is queued on `stream`; the call waits once, for the slot count that sizes the sort
 *                            (as bsc_asm_device waits for its counts), and returns with the rest in flight.  Workspaces of the context's
 *                            (the site masks are the read-level table's), grow-only: one call in flight per context.  A refusal writes
 *                            nothing.
 *   bsc_pat_text_device      the lines of d_rec[min(*d_n_rec, max_rec)] -> d_out[<= out_cap] (16-byte aligned).  d_totals2: two device u64
 *                            {bytes, lines}.  A stream longer than out_cap is cut at a 64-record boundary and its full length is still
 *                            reported, as the other text encoders do.
 *   bsc_block_pat_kept       the twin of bsc_block_epi_kept, with its preconditions and refusals: walks the prepared templates, reads and
 *                            reference codes the last *_keep call left in HBM and writes the table into a buffer of the context's own
 *                            (room: dev_cap bytes).  dev_cap too small: BSC_ERR_ARG with *n_bytes = the room needed (the totals are
 *                            filled), and the call may be repeated.  Every other kept output is untouched, before or after.  Waits.
 *   bsc_pat_stream_read      bytes [off, off + n) of that table -> dst, queued on the context's stream
 *   bsc_pat_stream_detach    the table handed over as bsc_epi_stream_detach hands one over
 * Not built: sharded runs, the batched and host-buffer block entries, non-CpG contexts, an index of the table, genome-wide indices in the
 * run, lines longer than 64 sites.
 */
#define BSC_PAT_MAX_SITES 64
typedef struct {
  uint32_t idx;   /* the ordinal of the piece's first site */
  uint32_t count; /* pieces with this (idx, hi, lo) */
  uint64_t hi;    /* sites 0 .. 31: site j in bits 63 - 2j, 62 - 2j */
  uint64_t lo;    /* sites 32 .. 63 */
} bsc_pat_rec;
typedef struct {
  uint32_t min_sites; /* PATTERN: k_t >= max(1, min_sites) */
  uint32_t reserved;  /* 0; anything else is refused */
} bsc_pat_params;
#define BSC_PAT_N_TOTALS 8
void bsc_pat_params_default(bsc_pat_params *p);
int bsc_pat_count_sites(const uint8_t *codes, uint64_t contig_len, uint64_t from, uint64_t to, uint64_t *n);
int bsc_pat_recs_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                      int32_t min_qual, const bsc_pat_params *p, bsc_pat_rec *rec, uint64_t cap, uint64_t *n_rec, uint64_t totals[8]);
long bsc_pat_format(const char *contig, uint64_t index_base, const bsc_pat_rec *rec, size_t n, const bsc_pat_params *p, char *buf, size_t cap,
                    uint64_t totals2[2]);
int bsc_pat_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const void *d_ref,
                   const bsc_pat_params *p, void *d_rec, uint64_t rec_cap, void *d_n_rec, void *d_totals, void *stream);
int bsc_pat_text_device(bsc_context *ctx, const void *d_rec, const void *d_n_rec, uint64_t max_rec, const char *contig, uint64_t index_base,
                        const bsc_pat_params *p, void *d_out, uint64_t out_cap, void *d_totals2, void *stream);
int bsc_block_pat_kept(bsc_context *ctx, const char *contig, const bsc_pat_params *p, uint64_t index_base, uint64_t dev_cap, uint64_t *n_bytes,
                       uint64_t *n_lines, uint64_t totals[8]);
int bsc_pat_stream_read(bsc_context *ctx, uint64_t off, uint64_t n, void *dst);
int bsc_pat_stream_detach(bsc_context *ctx, void **d_stream, uint64_t *n_bytes);

/*
 * The per-region fragment methylation summary (csrc/fragdev.hip: one walk behind the site pass and the scan of csrc/cpgreadsdev.hip;
 * csrc/frag.c holds the host form, which is its checker; bs_call_amd/frag.py the Python rule).  Per region of a BED file — a marker, a CpG
 * island, a DMR, a fixed tile — the number of templates (fragments) that are mostly unmethylated, mixed and mostly methylated within it: the
 * U / X / M counts of fragment-level deconvolution and of `wgbstools homog`, with the region's discordant fragments and the sums from which
 * the mean per-read level follows.  It is the product of the region summary above (which has forgotten the molecules) and the read-level
 * tables (which know no regions): the walk adds straight into per-region accumulators and writes no table.  The reference has no such
 * output: the rule is this project's own.
 *
 * COUNTS, SITE, BYTE(t, q) and STATE(t, s) are those of the read-level CpG table above, word for word; REGION is the region summary's; the
 * inputs are those of bsc_cpg_reads_device.
 * IN(s, R)  A site whose C is at the 1-based position p lies in the region R = {start, end} iff start < p <= end: REGION's containment,
 *           applied to the C.  A CpG whose C is inside and whose G is outside belongs to R — for a G2A template too, whose byte is read
 *           at p + 1; a CpG whose C is outside does not belong, wherever its G lies.
 * Per (template t, region R)  k = the number of sites s with IN(s, R) and STATE(t, s) != none; m = the number of those with state M.
 *           1 <= k < min_sites: t is SHORT in R.  k >= min_sites: t is a FRAGMENT of R, of exactly one class, tested in this order:
 *             U iff 100 m <= u_max_pct k;  M iff 100 m >= m_min_pct k;  X otherwise
 *           — in 64-bit integers.  A fragment is DISCORDANT iff 0 < m < k.  k == 0: t gives R nothing.
 * SUMS      Eight u64 per region: {frags, U, X, M, K = sum of k, Mm = sum of m, disc, short}; K and Mm run over fragments only.  Regions may
 *           overlap, nest, repeat and be empty: each is summed alone, and a template counts in every region where it qualifies.  Integer
 *           adds alone: the result is a function of the input, whatever the order.
 * Per block Only sites within x .. y count, as in the other read-level tables; the accumulators add over the block calls of a contig.
 * TOTALS    of one call, eight u64: [0] templates with k_t >= 1 over the whole block (k_t as in the read-level table), [1 .. 7] the sums of
 *           the seven columns frags .. disc over all attached regions.  short is per region only.
 * LINE      Twelve tab-separated columns and '\n', plain decimals, no header, no float:
 *             chrom  start  end  name  frags  U  X  M  K  Mm  disc  short
 *           name: as bsc_meth_regions_format writes it (the BED's fourth column, or ".").  The lines come in the attached order and join
 *           the region summary's lines on the first four columns.  The U / X / M shares, disc / frags and the mean level Mm / K are the
 *           reader's (bs_call_amd/frag.py: fractions).
 * Params    bsc_frag_params {min_sites, u_max_pct, m_min_pct, reserved}, default {3, 25, 75, 0}.  Refused with BSC_ERR_ARG: min_sites == 0, a
 *           percentage above 100, u_max_pct >= m_min_pct, reserved != 0.
 * LIMITS    No template spans two blocks: the reader ends a block only where the next forward-facing read begins more than one base behind
 *           everything the block holds (csrc/bamio.c, csrc/bamdev.hip), and a mate joins its template in the block that holds it.  So a
 *           fragment is counted once, in one block, and a region across a block border gets each template whole.  The one exception is the
 *           reader's keep_unmatched: a mate that arrives after its partner's block has closed is a template of its own in the later block,
 *           and the table then counts the molecule as two fragments (as every read-level table does).
 *           A template's candidates are the attached regions of index [lo, hi): hi from the sorted starts, lo from the running maximum of
 *           the ends.  A region longer than 65 536 bases is kept out of that running maximum and goes into a separate short list that every
 *           template tests whole, 64 entries a round: a chromosome-long region listed first costs one round a template, not the whole
 *           list.  A set of very many such regions costs (their number / 64) rounds a template.
 *           A template whose span touches more than 64 tiles (4 096 positions: a long read) does not fit the walk's strip of masks: the
 *           strip is then made again, read bytes and all, for every round of 64 candidates, the long list's rounds included, so such a
 *           template costs (rounds x tiles) where a shorter one costs (rounds + tiles).
 * Not gated by the called genotype, as the read-level table is not.
 *
 *   bsc_frag_params_default  {3, 25, 75, 0}
 *   bsc_frag_regions_host    the host form: adds the block into acc[n_regions][8] (NOT zeroed here) and, where totals is not NULL, writes the
 *                            call's eight totals.  regions need not be sorted.  A plain loop
 *   bsc_frag_format          the lines of regions[0 .. n) of one contig -> buf, with bsc_meth_regions_format's return conventions and
 *                            refusals: the length written; the length needed — and nothing written — when cap is too small; < 0 for a bad
 *                            argument
 *   bsc_frag_attach          regions[0 .. n) of ONE contig, sorted by (start, end), uploaded with the search's arrays; their accumulators
 *                            zeroed.  n == 0 detaches.  bsc_meth_regions_attach's refusals, and the previous attachment stays.  The
 *                            accumulators are this table's own: bsc_meth_regions_* neither see nor touch them.  Waits.
 *   bsc_frag_device          adds one block from device-resident inputs (d_tpl 8-byte aligned, d_ref y - x + 3 codes) into the attached
 *                            regions' accumulators; d_totals: eight device u64 (8-byte aligned), written.  Asynchronous on `stream`; calls
 *                            may follow one another on any streams the caller orders (the adds are atomic).  Every workspace is reserved
 *                            before anything is written; a refusal writes nothing.  BSC_ERR_ARG with nothing attached.  nr == 0 is legal
 *                            and adds nothing (the totals are zeroed).
 *   bsc_block_frag_kept      the twin of bsc_block_epi_kept, with its preconditions and refusals: walks the prepared templates, reads and
 *                            reference codes the last *_keep call left in HBM.  totals (may be NULL): the call's eight.  Every other kept
 *                            output is untouched, before or after.  Waits.
 *   bsc_frag_read            the accumulators -> acc_host[n][8], n = the attached count; waits for the context's stream and the stream of
 *                            the last accumulating call
 *   bsc_frag_reset           zeroes them (waits likewise)
 * Not built: sharded runs, the batched and host-buffer block entries, non-CpG contexts, classes other than the three, float columns.
 */
typedef struct {
  uint32_t min_sites; /* FRAGMENT: k >= min_sites; 0 is refused */
  uint32_t u_max_pct; /* U iff 100 m <= u_max_pct k */
  uint32_t m_min_pct; /* M iff 100 m >= m_min_pct k; must exceed u_max_pct */
  uint32_t reserved;  /* 0; anything else is refused */
} bsc_frag_params;
#define BSC_FRAG_N_SUMS 8
#define BSC_FRAG_N_TOTALS 8
void bsc_frag_params_default(bsc_frag_params *p);
int bsc_frag_regions_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                          int32_t min_qual, const bsc_frag_params *p, const bsc_meth_region *regions, size_t n_regions, uint64_t *acc,
                          uint64_t totals[8]);
long bsc_frag_format(const char *contig, const bsc_meth_region *regions, const char *const *names, const uint64_t *acc, size_t n, char *buf,
                     size_t cap);
int bsc_frag_attach(bsc_context *ctx, const bsc_meth_region *regions, uint64_t n);
int bsc_frag_device(bsc_context *ctx, const void *d_tpl, uint32_t nr, const void *d_seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const void *d_ref,
                    const bsc_frag_params *p, void *d_totals, void *stream);
int bsc_block_frag_kept(bsc_context *ctx, const bsc_frag_params *p, uint64_t totals[8]);
int bsc_frag_read(bsc_context *ctx, uint64_t *acc_host, uint64_t n);
int bsc_frag_reset(bsc_context *ctx);

/*
 * dbSNP index (host C + zlib; csrc/dbsnp.c): the reader of the compressed index bin/dbSNP_idx writes.  In the reference
 * the index never touches the likelihoods: an entry names the record (VCF ID), forces the AA / TT homozygous-reference
 * record of a site flagged in its `fq_mask` to be written (rs_found & 2, src/print_vcf.c:139) and feeds the dbSNP
 * counters of the statistics (:426-441).
 *   bsc_dbsnp_open          load_dbSNP_header   src/dbSNP.c:27-141
 *   bsc_dbsnp_load_contig   load_dbSNP_ctg      src/dbSNP.c:157-304 (the previous contig is dropped, as print_vcf_entry
 *                                               does at a contig change, src/print_vcf.c:553-562); a contig the index
 *                                               does not list loads as "nothing flagged"; *n_snps = entries loaded
 *   bsc_dbsnp_flags         rs_found (0 / 1 / 3) of positions x0 .. x0 + n - 1 (1-based) of the loaded contig: the
 *                           `dbsnp` array of bsc_chain_device / bsc_block_records / bsc_vcf_records
 *   bsc_dbsnp_name          dbSNP_lookup_name   src/dbSNP.c:306-350: returns rs_found, the name in rs (NUL-terminated) and
 *                           in *rs_len the length the reference hands to htslib (an odd number of digits counts its
 *                           filler byte); negative on error
 */
typedef struct bsc_dbsnp bsc_dbsnp;
int bsc_dbsnp_open(const char *path, bsc_dbsnp **out);
void bsc_dbsnp_close(bsc_dbsnp *db);
int bsc_dbsnp_n_contigs(const bsc_dbsnp *db);
const char *bsc_dbsnp_contig_name(const bsc_dbsnp *db, int i);
const char *bsc_dbsnp_header(const bsc_dbsnp *db);
int bsc_dbsnp_load_contig(bsc_dbsnp *db, const char *name, uint64_t *n_snps);
int bsc_dbsnp_flags(const bsc_dbsnp *db, uint32_t x0, uint32_t n, uint8_t *out);
int bsc_dbsnp_name(const bsc_dbsnp *db, uint32_t x, char *rs, size_t cap, size_t *rs_len);

/*
 * The loaded contig kept on the device (csrc/dbsnpdev_core.h, csrc/dbsnpdev.hip): the per-block products of the index — the flags the
 * chain reads, the names table the stream encoders search — are made in HBM instead of on a host thread and uploaded.
 *   bsc_dbsnp_attach         snapshots the contig currently loaded in db into the context (flat arrays, one upload); later
 *                            bsc_dbsnp_load_contig / bsc_dbsnp_close calls on db do not affect it.  No contig loaded, or one the index
 *                            does not list: an EMPTY contig is attached (flags 0, no names).  Replaces a previous attachment; *n_snps =
 *                            entries attached.  BSC_ERR_ARG, naming the position, for an entry whose prefix the index does not have.
 *                            The previous attachment is dropped before anything can fail: after a refused attach NOTHING is attached.
 *   bsc_dbsnp_detach         drops the attachment (bsc_destroy does too).  Both wait for the context's own stream first: a submitted
 *                            block may still be reading the arrays.
 *   bsc_dbsnp_count          names and name bytes of positions x0 .. x0 + n - 1: host arithmetic, no device round trip — the sizes of
 *                            bsc_dbsnp_names_device's outputs
 *   bsc_dbsnp_flags_device   d_out[n] = what bsc_dbsnp_flags writes, any alignment; asynchronous on `stream`
 *   bsc_dbsnp_names_device   d_pos[n_names] | d_off[n_names + 1] | d_bytes[n_bytes] = what bsc_dbsnp_names fills; asynchronous on
 *                            `stream`; room for fewer than bsc_dbsnp_count's figures is BSC_ERR_ARG before anything is launched
 * x0 >= 1, x0 + n - 1 <= 2^32 - 1; n = 0 does nothing; the three queries without an attachment are BSC_ERR_ARG.
 *
 * While a contig is attached, bsc_block_records_rawdev, bsc_block_bcf_rawdev, bsc_block_bcf_rawdev_keep and bsc_block_vcf_rawdev_keep
 * read dbsnp == NULL as "the attachment's flags" and names == NULL as "the attachment's names": both are made on the context's stream
 * ahead of the chain and the encoder (bsc_block_bcf_again encodes with the same table).  Arrays that are passed are used as before, and
 * every other entry — and these four with nothing attached — is unchanged.
 */
int bsc_dbsnp_attach(bsc_context *ctx, const bsc_dbsnp *db, uint64_t *n_snps);
int bsc_dbsnp_detach(bsc_context *ctx);
int bsc_dbsnp_count(const bsc_context *ctx, uint32_t x0, uint32_t n, uint32_t *n_names, uint64_t *n_bytes);
int bsc_dbsnp_flags_device(bsc_context *ctx, uint32_t x0, uint32_t n, void *d_out, void *stream);
int bsc_dbsnp_names_device(bsc_context *ctx, uint32_t x0, uint32_t n, void *d_pos, void *d_off, void *d_bytes, uint32_t cap_names,
                           uint64_t cap_bytes, void *stream);

/* Host-side text rendering of one record as a VCF data line ("CHROM POS ID REF ALT QUAL FILTER INFO FORMAT SAMPLE",
 * tab separated, no newline): the field layout of the record the reference hands to htslib (src/print_vcf.c:160-380).
 * Returns the length written, 0 when c->emit == 0, -1 when buf is too small.  `id` NULL/"" prints ".". */
int bsc_vcf_format(const bsc_vcf_core *c, const bsc_gt_meth *g, const char *contig, const char *id, char *buf,
                   size_t cap);

/* Per-launch kernel timing with HIP events recorded on the launch stream (measurement support):
 * after bsc_set_profiling(ctx, 1), bsc_last_kernel_ms() returns the device time of the most recent
 * calling kernel and of its Fisher pass (it waits for that launch to finish).  With n > 2^31 sites per
 * call only the last sub-launch is reported. */
int bsc_set_profiling(bsc_context *ctx, int enable);
int bsc_last_kernel_ms(bsc_context *ctx, float *call_ms, float *fisher_ms);
/* The same for the launch `age` launches back (0 = the most recent; the last 32 are kept), so that a timed loop can run
 * without waiting on events and read its launches' device times afterwards. */
int bsc_kernel_ms_history(bsc_context *ctx, uint32_t age, float *call_ms, float *fisher_ms);

/* Measurement support: the time (ms, HIP events on `stream`, average of `reps` launches queued back to back behind three untimed ones) of a kernel that moves exactly
 * the bytes of bsc_call_sites_device(ctx, d_cts, d_ref, n, d_out, 200, d_skip) — 104 + 1 in, 200 + 1 out per position,
 * same tile shape, no arithmetic: the practical memory ceiling for that call.  OVERWRITES d_out / d_skip with junk;
 * n is rounded down to a multiple of 64. */
int bsc_stream_probe_ms(bsc_context *ctx, const void *d_cts, const void *d_ref, uint64_t n, void *d_out, void *d_skip,
                        int reps, void *stream, float *ms);

/* Blocks until everything queued on the context's own stream (the host-buffer entries) has finished. */
int bsc_synchronize(bsc_context *ctx);

/* Counters (device -> host; synchronises the context's stream). */
int bsc_get_stats(bsc_context *ctx, bsc_stats *out);
int bsc_reset_stats(bsc_context *ctx);

/*
 * Synthetic 'L-pileup' generator: fills d_cts[n] and d_ref[n] on
 * the device for absolute site indices first_site .. first_site+n-1 of a synthetic contig.  Deterministic
 * in (seed, site index) only, so any window can be regenerated independently.  Bench/test support.
 */
#define BSC_SYNTH_NRUNS 1u /* flags: 1 % of 10-kb runs are N (reference code 0) with no reads */
int bsc_synth_pileup_device(bsc_context *ctx, uint64_t seed, uint64_t first_site, uint64_t n, uint32_t coverage,
                            uint32_t flags, void *d_cts, void *d_ref, void *stream);
/* Host generator of synthetic read pairs over positions x .. x+n_sites-1 ('L-reads'; see
 * bs_call_amd/csrc/synth_reads.c): fills tpl[] (in the order of the pairs' start positions — a template that lost its
 * forward read is therefore out of leftmost-position order, as in real align_lists) and seq[]; returns the number
 * of templates, or -1 if a buffer is too small.  Reference bases come from the same synthetic genome as the
 * L-pileup generator (site index = position). */
int64_t bsc_synth_reads_host(uint64_t seed, uint32_t x, uint32_t n_sites, uint32_t coverage, uint32_t flags,
                             bsc_template *tpl, uint64_t max_templates, uint8_t *seq, uint64_t seq_cap,
                             uint64_t *seq_used);
/* Host twin of the generator (same bits), for feeding the same inputs to a CPU checker. */
int bsc_synth_pileup_host(uint64_t seed, uint64_t first_site, uint64_t n, uint32_t coverage, uint32_t flags,
                          bsc_pileup *cts, uint8_t *ref);

#ifdef __cplusplus
}
#endif
#endif /* BSCALL_AMD_H */
