/*
 * ref_driver.c — a flat C ABI over the REFERENCE's own functions (heathsc/bs_call v2.1.7).
 *
 * *** TEST INFRASTRUCTURE, NOT PRODUCT. ***  This file is ours; it is linked (oracle/Makefile, target `ref`) with object
 * files compiled from the reference's unchanged sources into oracle/_ref/libbscall_ref.so, which is never committed.
 * Nothing here restates the reference: every number that comes out was computed by the reference's functions
 *   calc_gt_prob, fill_base_prob_table        src/genotype_model.c
 *   fisher, lfact_store_init                  src/stats_utils.c
 *   init_param                                src/init_param.c
 *   call_genotypes_ML, init/join_calc_threads src/call_genotypes.c   (HOT LOOP A, the calc-thread pool, HOT LOOP B)
 *   process_template_vector                   src/process_template.c (with trim_read, trim_soft_clips, handle_overlap)
 *   meth_profile                              src/meth_profile.c
 *   get_next_align_details                    src/input_sam.c        (with get_bam_misms, get_seq_and_qual, get_bs_strand)
 * The driver only builds their inputs (gt_vector / align_details / work_t) from flat arrays laid out as
 * bs_call_amd/abi.py lays them out, plays the threads the reference's main program would have run around them, and copies
 * the results out.  The reference's asserts are live: hand over only inputs it accepts (see oracle/ref_loader.py).
 *
 * Three levels:
 *   1  refdrv_calc_gt_prob_array, refdrv_fisher_array, refdrv_tables      site arithmetic
 *   2  refdrv_open / refdrv_block / refdrv_close                           one call_genotypes_ML block
 *   3  refdrv_prep_block (between refdrv_open and refdrv_close)            process_template_vector: the per-template stage,
 *                                                                          the read profile, then the same block as level 2
 *   R  refdrv_align_details                                                the record parser, one BAM record at a time
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "gem_tools.h"
#include "bs_call.h"

_Static_assert(sizeof(pileup) == 104, "pileup layout");
_Static_assert(sizeof(gt_meth) == 200, "gt_meth layout");
_Static_assert(sizeof(gt_vcf) == 208, "gt_vcf layout");

/* abi.py: TEMPLATE (40 B), RAW_TEMPLATE (72 B), MISMS (12 B) */
typedef struct {
  uint32_t pos[2];
  uint32_t len[2];
  uint64_t off[2];
  uint8_t mapq[2];
  uint8_t orientation;
  uint8_t bs_strand;
  uint32_t flags;
} drv_template;

typedef struct {
  uint32_t pos[2];
  uint32_t span[2]; /* reference_span */
  uint32_t len[2];
  uint32_t n_misms[2];
  uint64_t off[2];
  uint64_t misms_off[2];
  uint8_t mapq[2];
  uint8_t orientation;
  uint8_t bs_strand;
  uint32_t pad;
} drv_raw_template;

typedef struct {
  uint32_t type, position, size;
} drv_misms;

_Static_assert(sizeof(drv_template) == 40, "TEMPLATE layout");
_Static_assert(sizeof(drv_raw_template) == 72, "RAW_TEMPLATE layout");
_Static_assert(sizeof(drv_misms) == 12, "MISMS layout");

int refdrv_sizeof_pileup(void) { return (int)sizeof(pileup); }
int refdrv_sizeof_gt_meth(void) { return (int)sizeof(gt_meth); }
int refdrv_sizeof_gt_vcf(void) { return (int)sizeof(gt_vcf); }

static void drop_flt_names(sr_param *par) {
  for (int i = 0; i < 4; i++) {
    free(par->defs.flt_name[i]);
    par->defs.flt_name[i] = NULL;
  }
}

/* ---- level 1 ------------------------------------------------------------------------------------------------------- */
static sr_param site_par; /* level 1 keeps its own parameter block: a level-2 session may be open */

void refdrv_calc_gt_prob_array(gt_meth *gt, const char *rf, uint64_t n, double under_conv, double over_conv, double ref_bias) {
  init_param(&site_par), fill_base_prob_table();
  site_par.under_conv = under_conv;
  site_par.over_conv = over_conv;
  site_par.ref_bias = ref_bias;
  for (uint64_t i = 0; i < n; i++) calc_gt_prob(gt + i, &site_par, rf[i]);
  drop_flt_names(&site_par);
}

void refdrv_fisher_array(const int *c4, uint64_t n, double *out) {
  static double lfs[LFACT_STORE_SIZE];
  lfact_store_init(lfs);
  for (uint64_t i = 0; i < n; i++) {
    int c[4]; /* fisher() changes its table */
    memcpy(c, c4 + 4 * i, sizeof c);
    out[i] = fisher(c, lfs);
  }
}

void refdrv_tables(double *lfact_store, uint8_t *gt_het) {
  init_param(&site_par);
  memcpy(lfact_store, site_par.defs.lfact_store, sizeof site_par.defs.lfact_store);
  for (int i = 0; i < 10; i++) gt_het[i] = site_par.defs.gt_het[i];
  drop_flt_names(&site_par);
}

/* ---- levels 2 and 3: one session = one parameter set ------------------------------------------------------------------ */
static sr_param par;
static int session_open;
static ctg_t drv_ctg;
static pthread_t profile_thr;
static int profile_thr_running;

/* the block's reference codes (0 N, 1 A, 2 C, 3 G, 4 T), handed over by the caller of refdrv_prep_block */
static const char *ref_codes;
static uint32_t ref_codes_x0, ref_codes_n;

/* process_template_vector asks for the block's reference through this function; the reference's own one reads a FASTA
 * index through htslib.  Positions outside what the caller handed over read as N, like positions outside the contig. */
bool get_sequence_string(ctg_t *const ctg, const uint32_t x, const uint32_t sz, ctg_t *const prev_ctg, gt_string *const ref,
                         sr_param *const p) {
  (void)ctg, (void)prev_ctg, (void)p;
  if (sz == 0 || ref_codes == NULL) return true;
  gt_string_resize(ref, (uint64_t)sz + 1);
  for (uint32_t i = 0; i < sz; i++) {
    uint64_t at = (uint64_t)x + i;
    ref->buffer[i] = (at >= ref_codes_x0 && at - ref_codes_x0 < ref_codes_n) ? ref_codes[at - ref_codes_x0] : 0;
  }
  ref->buffer[sz] = 0;
  ref->length = (uint64_t)sz + 1;
  return false;
}

/* the consumer the reference's main program runs next to the process thread: one meth_profile() per handed-over template */
static void *profile_consumer(void *arg) {
  work_t *const w = &((sr_param *)arg)->work;
  for (;;) {
    pthread_mutex_lock(&w->mprof_mutex);
    while (w->mprof_read_idx == w->mprof_write_idx && !w->mprof_end) pthread_cond_wait(&w->mprof_cond1, &w->mprof_mutex);
    const int slot = w->mprof_read_idx;
    const int drained = slot == w->mprof_write_idx;
    pthread_mutex_unlock(&w->mprof_mutex);
    if (drained) return NULL;
    mprof_thread_t *const job = &w->mprof_thread[slot];
    meth_profile(job->al, job->x, job->orig_pos, (int)job->max_pos, arg);
    pthread_mutex_lock(&w->mprof_mutex);
    w->mprof_read_idx = (slot + 1) % N_MPROF_BUFFERS;
    pthread_cond_broadcast(&w->mprof_cond2);
    pthread_mutex_unlock(&w->mprof_mutex);
  }
}

/* trims: {left_trim[0], left_trim[1], right_trim[0], right_trim[1]} or NULL; with_stats: allocate bs_stats and run the
 * profile consumer (level 3).  n_calc_threads: 1..3. */
int refdrv_open(double under_conv, double over_conv, double ref_bias, int min_qual, int n_calc_threads, const int *trims, int with_stats) {
  if (session_open || n_calc_threads < 1 || n_calc_threads > 3 || min_qual < 1 || min_qual > MAX_QUAL) return -1;
  init_param(&par), fill_base_prob_table();
  par.under_conv = under_conv;
  par.over_conv = over_conv;
  par.ref_bias = ref_bias;
  par.min_qual = (uint8_t)min_qual;
  if (trims) {
    par.left_trim[0] = (uint32_t)trims[0];
    par.left_trim[1] = (uint32_t)trims[1];
    par.right_trim[0] = (uint32_t)trims[2];
    par.right_trim[1] = (uint32_t)trims[3];
  }
  par.num_threads[CALC_THREADS] = n_calc_threads - 1; /* init_calc_threads starts 1 + this many */
  work_t *const w = &par.work;
  w->ref = gt_string_new(16384);
  w->ref1 = gt_string_new(16384);
  for (int i = 0; i < N_MPROF_BUFFERS; i++)
    for (int k = 0; k < 2; k++) w->mprof_thread[i].orig_pos[k] = gt_vector_new(256, sizeof(int));
  if (with_stats) {
    w->stats = calloc(1, sizeof(bs_stats));
    w->stats->meth_profile = gt_vector_new(256, sizeof(meth_cts));
    memset(w->stats->meth_profile->memory, 0, sizeof(meth_cts) * w->stats->meth_profile->elements_allocated);
  }
  memset(&drv_ctg, 0, sizeof drv_ctg);
  drv_ctg.name = "ref_driver";
  init_calc_threads(&par);
  profile_thr_running = 0;
  if (with_stats) {
    if (pthread_create(&profile_thr, NULL, profile_consumer, &par)) return -2;
    profile_thr_running = 1;
  }
  session_open = 1;
  return 0;
}

void refdrv_close(void) {
  if (!session_open) return;
  work_t *const w = &par.work;
  join_calc_threads(&par);
  if (profile_thr_running) {
    pthread_mutex_lock(&w->mprof_mutex);
    w->mprof_end = true;
    pthread_cond_broadcast(&w->mprof_cond1);
    pthread_mutex_unlock(&w->mprof_mutex);
    pthread_join(profile_thr, NULL);
    profile_thr_running = 0;
  }
  for (int i = 0; i < N_MPROF_BUFFERS; i++)
    for (int k = 0; k < 2; k++) gt_vector_delete(w->mprof_thread[i].orig_pos[k]);
  if (w->stats) {
    gt_vector_delete(w->stats->meth_profile);
    free(w->stats);
    w->stats = NULL;
  }
  gt_string_delete(w->ref);
  gt_string_delete(w->ref1);
  free(w->vcf);
  w->vcf = NULL;
  w->vcf_size = 0;
  drop_flt_names(&par);
  session_open = 0;
}

static gt_vector *bytes_vector(const uint8_t *src, uint32_t n) {
  gt_vector *v = gt_vector_new(n ? n : 1, 1);
  memcpy(gt_vector_get_mem(v, uint8_t), src, n);
  gt_vector_set_used(v, n);
  return v;
}

static void free_align_list(gt_vector *list) {
  align_details **al_p = gt_vector_get_mem(list, align_details *);
  for (uint64_t i = 0; i < gt_vector_get_used(list); i++) {
    for (int k = 0; k < 2; ++k) {
      if (al_p[i]->read[k]) gt_vector_delete(al_p[i]->read[k]);
      gt_vector_delete(al_p[i]->mismatches[k]);
    }
    free(al_p[i]);
  }
  gt_vector_delete(list);
}

/* after call_genotypes_ML returned: wait for its calc threads, then copy the pile-up, the calls and the skip flags out */
static void collect_block(uint32_t sz, pileup *out_pile, gt_meth *out_gtm, uint8_t *out_skip) {
  work_t *const w = &par.work;
  pthread_mutex_lock(&w->calc_mutex);
  while (w->calc_threads_complete < w->n_calc_threads) {
    struct timespec until;
    clock_gettime(CLOCK_REALTIME, &until), until.tv_sec += 1;
    pthread_cond_timedwait(&w->calc_cond2, &w->calc_mutex, &until);
  }
  pthread_mutex_unlock(&w->calc_mutex);
  memcpy(out_pile, w->calc_threads[0].cts, sizeof(pileup) * (size_t)sz); /* thread 0 was handed the start of the array */
  for (uint32_t i = 0; i < sz; i++) {
    out_skip[i] = w->vcf[i].skip ? 1 : 0;
    if (w->vcf[i].skip) memset(out_gtm + i, 0, sizeof(gt_meth)); /* the entry of a skipped position is never written */
    else memcpy(out_gtm + i, &w->vcf[i].gtm, sizeof(gt_meth));
  }
  w->vcf_n = 0; /* what the print thread does once it has written the block */
}

/* Level 2.  tpl: nr templates whose read k is len[k] bytes at seq + off[k] (len 0: no read); ref: the codes of x .. y. */
int refdrv_block(const drv_template *tpl, uint32_t nr, const uint8_t *seq, uint32_t x, uint32_t y, const char *ref,
                 pileup *out_pile, gt_meth *out_gtm, uint8_t *out_skip) {
  if (!session_open || y < x) return -1;
  work_t *const w = &par.work;
  const uint32_t sz = y - x + 1;
  gt_vector *list = gt_vector_new(nr ? nr : 1, sizeof(align_details *));
  for (uint32_t i = 0; i < nr; i++) {
    align_details *al = calloc(1, sizeof *al);
    al->forward_position = tpl[i].pos[0];
    al->reverse_position = tpl[i].pos[1];
    al->orientation = (gt_strand)tpl[i].orientation;
    al->bs_strand = (gt_bs_strand)tpl[i].bs_strand;
    for (int k = 0; k < 2; ++k) {
      al->mapq[k] = tpl[i].mapq[k];
      al->reference_span[k] = tpl[i].len[k];
      al->read[k] = tpl[i].len[k] ? bytes_vector(seq + tpl[i].off[k], tpl[i].len[k]) : NULL;
      al->mismatches[k] = gt_vector_new(8, sizeof(gt_misms));
    }
    gt_vector_insert(list, al, align_details *);
  }
  /* call_genotypes_ML swaps ref1 into ref before it wakes the calc threads: the block's codes go into ref1 */
  gt_string_resize(w->ref1, (uint64_t)sz + 3);
  memcpy(w->ref1->buffer, ref, sz);
  memset(w->ref1->buffer + sz, 0, 3);
  w->ref1->length = (uint64_t)sz + 3;
  call_genotypes_ML(&drv_ctg, list, x, y, &par);
  collect_block(sz, out_pile, out_gtm, out_skip);
  free_align_list(list);
  return 0;
}

/* Level 3.  raw / seq / misms: nr raw templates (RAW_TEMPLATE, MISMS).  ref: n_ref codes, the first one of position ref_x0.
 * x must be what process_template_vector derives from the first template (its start - 2, at least 1): the caller sized
 * out_pile / out_gtm / out_skip for x .. y.  out_tpl[nr] / out_seq (seq_cap bytes): the prepared templates, flattened;
 * out_stats[7]: base_filter[0..4], filter_cts[gt_flt_none], filter_bases[gt_flt_none]; out_prof: prof_cap x 4 counters of
 * bs_stats.meth_profile from its element 0 on, *out_prof_used its length.  Returns 0, or a negative number. */
int refdrv_prep_block(const drv_raw_template *raw, uint32_t nr, const uint8_t *seq, const drv_misms *misms, uint32_t x, uint32_t y,
                      const char *ref, uint32_t ref_x0, uint32_t n_ref, drv_template *out_tpl, uint8_t *out_seq, uint64_t seq_cap,
                      uint64_t *out_stats, uint64_t *out_prof, uint64_t prof_cap, uint64_t *out_prof_used, pileup *out_pile,
                      gt_meth *out_gtm, uint8_t *out_skip) {
  if (!session_open || !par.work.stats || nr == 0 || y < x) return -1;
  uint32_t first = raw[0].pos[0] ? raw[0].pos[0] : raw[0].pos[1];
  if (first == 0 || first > y || (first > 2 ? first - 2 : 1) != x) return -2;
  work_t *const w = &par.work;
  gt_vector *list = gt_vector_new(nr, sizeof(align_details *));
  for (uint32_t i = 0; i < nr; i++) {
    align_details *al = calloc(1, sizeof *al);
    al->forward_position = raw[i].pos[0];
    al->reverse_position = raw[i].pos[1];
    al->orientation = (gt_strand)raw[i].orientation;
    al->bs_strand = (gt_bs_strand)raw[i].bs_strand;
    for (int k = 0; k < 2; ++k) {
      al->mapq[k] = raw[i].mapq[k];
      al->reference_span[k] = raw[i].span[k];
      al->read[k] = raw[i].len[k] ? bytes_vector(seq + raw[i].off[k], raw[i].len[k]) : NULL;
      al->mismatches[k] = gt_vector_new(8, sizeof(gt_misms));
      for (uint32_t z = 0; z < raw[i].n_misms[k]; z++) {
        const drv_misms *m = misms + raw[i].misms_off[k] + z;
        gt_misms e;
        memset(&e, 0, sizeof e);
        e.misms_type = (gt_misms_t)m->type;
        e.position = m->position;
        e.size = m->size;
        gt_vector_insert(al->mismatches[k], e, gt_misms);
      }
    }
    gt_vector_insert(list, al, align_details *);
  }
  ref_codes = ref;
  ref_codes_x0 = ref_x0;
  ref_codes_n = n_ref;
  bs_stats *const st = w->stats;
  uint64_t before[7];
  for (int i = 0; i < 5; i++) before[i] = st->base_filter[i];
  before[5] = st->filter_cts[gt_flt_none];
  before[6] = st->filter_bases[gt_flt_none];
  gt_status rc = process_template_vector(list, &drv_ctg, y, &par);
  ref_codes = NULL;
  if (rc != GT_STATUS_OK) {
    free_align_list(list);
    return -3;
  }
  collect_block(y - x + 1, out_pile, out_gtm, out_skip);
  for (int i = 0; i < 5; i++) out_stats[i] = st->base_filter[i] - before[i];
  out_stats[5] = st->filter_cts[gt_flt_none] - before[5];
  out_stats[6] = st->filter_bases[gt_flt_none] - before[6];
  int ret = 0;
  uint64_t at = 0;
  align_details **al_p = gt_vector_get_mem(list, align_details *);
  for (uint32_t i = 0; i < nr && !ret; i++) {
    const align_details *al = al_p[i];
    memset(out_tpl + i, 0, sizeof(drv_template));
    out_tpl[i].pos[0] = al->forward_position;
    out_tpl[i].pos[1] = al->reverse_position;
    out_tpl[i].orientation = (uint8_t)al->orientation;
    out_tpl[i].bs_strand = (uint8_t)al->bs_strand;
    for (int k = 0; k < 2; ++k) {
      out_tpl[i].mapq[k] = al->mapq[k];
      const uint64_t n = al->read[k] ? gt_vector_get_used(al->read[k]) : 0;
      if (at + n > seq_cap) {
        ret = -4;
        break;
      }
      out_tpl[i].off[k] = at;
      out_tpl[i].len[k] = (uint32_t)n;
      if (n) memcpy(out_seq + at, gt_vector_get_mem(al->read[k], uint8_t), n);
      at += n;
    }
  }
  /* call_genotypes_ML returned only after the consumer had drained its queue: the profile is complete */
  const uint64_t used = gt_vector_get_used(st->meth_profile);
  *out_prof_used = used;
  if (used > prof_cap) ret = ret ? ret : -5;
  else memcpy(out_prof, st->meth_profile->memory, sizeof(meth_cts) * used);
  free_align_list(list);
  return ret;
}

/* ---- level R: the record parser ------------------------------------------------------------------------------------------------
 * get_next_align_details reads its record through htslib's sam_read1 (sam_itr_next with an iterator).  There is no htslib here:
 * these two are ours, and sam_read1 hands over the next record of the buffer refdrv_align_details was given — a BAM file's
 * alignment records as the file holds them, block_size first. */
static const uint8_t *rd_records;
static const uint64_t *rd_offsets;
static uint64_t rd_n, rd_next;
static uint8_t *rd_buf; /* the record in hand */
static uint64_t rd_buf_cap;

static uint32_t rd_le32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

int sam_read1(htsFile *fp, bam_hdr_t *h, bam1_t *b) {
  (void)fp, (void)h;
  if (rd_next >= rd_n) return -1;
  const uint8_t *p = rd_records + rd_offsets[rd_next++];
  const uint32_t block_size = rd_le32(p);
  p += 4;
  bam1_core_t *const c = &b->core;
  c->tid = (int32_t)rd_le32(p);
  c->pos = (int32_t)rd_le32(p + 4);
  c->l_qname = p[8];
  c->qual = p[9];
  c->bin = (uint16_t)(p[10] | p[11] << 8);
  c->n_cigar = (uint16_t)(p[12] | p[13] << 8);
  c->flag = (uint16_t)(p[14] | p[15] << 8);
  c->l_qseq = (int32_t)rd_le32(p + 16);
  c->mtid = (int32_t)rd_le32(p + 20);
  c->mpos = (int32_t)rd_le32(p + 24);
  c->isize = (int32_t)rd_le32(p + 28);
  /* data points at the name, in a copy placed so that the CIGAR behind the name is dword-aligned: bam_get_cigar reads it as uint32_t */
  const uint32_t l_data = block_size - 32, shift = (4u - (c->l_qname & 3u)) & 3u;
  if ((uint64_t)l_data + 8 > rd_buf_cap) {
    free(rd_buf);
    rd_buf_cap = 2 * ((uint64_t)l_data + 8);
    rd_buf = malloc(rd_buf_cap);
    if (!rd_buf) return -2;
  }
  memcpy(rd_buf + shift, p + 32, l_data);
  b->data = rd_buf + shift;
  b->l_data = (int)l_data;
  b->m_data = block_size - 32;
  return (int)block_size;
}

int sam_itr_next(htsFile *fp, hts_itr_t *itr, bam1_t *b) {
  (void)fp, (void)itr, (void)b;
  return -1;
}

typedef struct {
  int32_t ret;
  uint32_t filtered, reverse, alignment_flag, align_length, orientation, forward_position, reverse_position;
  uint32_t mapq, reference_span, bs_strand; /* mapq[ix], reference_span[ix]: ix = 1 for a reverse-strand record */
  uint32_t n_misms;
  uint64_t misms_off; /* into out_misms */
  uint32_t read_len, pad; /* the used length of read[ix] (l_qseq) */
  uint64_t read_off;  /* into out_seq */
} drv_align_out;
_Static_assert(sizeof(drv_align_out) == 72, "ALIGN_OUT layout");

/* records: n alignment records (block_size, the 32 fixed bytes, the data), record i at records + offsets[i]; records_len: the
 * buffer's size.  One get_next_align_details per record with a fresh align_details.  A record the reference does not use
 * (ret = 1) leaves its span, strand, list and read empty, as the reference leaves them.  Returns 0; -1: a record does not lie
 * in the buffer or its fixed fields do not fit its block_size; -2 / -3: ms_cap / seq_cap too small. */
int refdrv_align_details(const uint8_t *records, uint64_t records_len, const uint64_t *offsets, uint64_t n, uint64_t mapq_thresh,
                         uint64_t max_template_len, int keep_unmatched, int ignore_dup, drv_align_out *out, drv_misms *out_misms,
                         uint64_t ms_cap, uint8_t *out_seq, uint64_t seq_cap) {
  for (uint64_t i = 0; i < n; i++) {
    if (offsets[i] + 36 > records_len) return -1;
    const uint8_t *p = records + offsets[i];
    const uint64_t bs = rd_le32(p), l_name = p[12], n_cigar = p[16] | (uint32_t)p[17] << 8, l_seq = rd_le32(p + 20);
    if (bs < 32 || offsets[i] + 4 + bs > records_len || 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq > bs) return -1;
  }
  rd_records = records;
  rd_offsets = offsets;
  rd_n = n;
  rd_next = 0;
  uint64_t ms_at = 0, seq_at = 0;
  int rc = 0;
  for (uint64_t i = 0; i < n && !rc; i++) {
    align_details al;
    memset(&al, 0, sizeof al);
    for (int k = 0; k < 2; k++) al.mismatches[k] = gt_vector_new(8, sizeof(gt_misms));
    bam1_t b;
    memset(&b, 0, sizeof b);
    bool reverse = false;
    gt_filter_reason filtered = gt_flt_none;
    uint32_t align_length = 0, alignment_flag = 0;
    const int ret = get_next_align_details(NULL, NULL, NULL, &b, &al, mapq_thresh, max_template_len, keep_unmatched != 0, ignore_dup != 0,
                                           &reverse, &filtered, &align_length, &alignment_flag);
    const int ix = reverse ? 1 : 0;
    drv_align_out *o = out + i;
    memset(o, 0, sizeof *o);
    o->ret = ret;
    o->filtered = (uint32_t)filtered;
    o->reverse = reverse ? 1 : 0;
    o->alignment_flag = alignment_flag;
    o->align_length = align_length;
    o->orientation = (uint32_t)al.orientation;
    o->forward_position = al.forward_position;
    o->reverse_position = al.reverse_position;
    o->mapq = al.mapq[ix];
    o->reference_span = al.reference_span[ix];
    o->bs_strand = (uint32_t)al.bs_strand;
    o->misms_off = ms_at;
    o->read_off = seq_at;
    const uint64_t nm = gt_vector_get_used(al.mismatches[ix]);
    if (ms_at + nm > ms_cap) rc = -2;
    else {
      const gt_misms *m = gt_vector_get_mem(al.mismatches[ix], gt_misms);
      for (uint64_t z = 0; z < nm; z++) {
        out_misms[ms_at + z].type = (uint32_t)m[z].misms_type;
        out_misms[ms_at + z].position = m[z].position;
        out_misms[ms_at + z].size = m[z].size;
      }
      o->n_misms = (uint32_t)nm;
      ms_at += nm;
    }
    if (!rc && al.read[ix]) {
      const uint64_t len = gt_vector_get_used(al.read[ix]);
      if (seq_at + len > seq_cap) rc = -3;
      else {
        if (len) memcpy(out_seq + seq_at, gt_vector_get_mem(al.read[ix], uint8_t), len);
        o->read_len = (uint32_t)len;
        seq_at += len;
      }
    }
    for (int k = 0; k < 2; k++) {
      if (al.read[k]) gt_vector_delete(al.read[k]);
      gt_vector_delete(al.mismatches[k]);
    }
  }
  rd_records = NULL;
  rd_n = rd_next = 0;
  return rc;
}
