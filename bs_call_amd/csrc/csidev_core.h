/*
 * csidev_core.h — the record walk of the CSI index scan (csidev.hip): one interval of a block's output stream — whole BCF2 records, or
 * whole VCF data lines — read record by record, each record's window (its 0-based position >> min_shift), and the runs of consecutive
 * records that share a window.  The statements compile for the device and for a host compiler (tests/csidev/csi_walk_host.c runs them on
 * the CPU, under the sanitizers), like dbsnpdev_core.h's.
 *
 *   BCF    l_shared, l_indiv at bytes 0 and 4, POS (0-based) at byte 12; the next record begins 8 + l_shared + l_indiv further on
 *          (csrc/bcf.c: bsc_bcf_record's fixed fields).  rlen is 1 for every record this project writes: a record lies in one window.
 *   text   CHROM '\t' POS (1-based, decimal) '\t' ... '\n'
 *
 * Nothing outside [beg, end) is read.  A record that does not end inside its interval, a line without a position, or a position below
 * the one before it stops the walk with an error bit: the runs closed so far stand, the rest of the interval is not walked.
 */
#ifndef BSC_CSIDEV_CORE_H
#define BSC_CSIDEV_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define CSI_FN __host__ __device__ __forceinline__
#else
#define CSI_FN static inline
#endif

#define CSI_FMT_BCF 0
#define CSI_FMT_VCF 1
#define CSI_ERR_STEP 1u     /* a record that leaves its interval (or is shorter than its fixed fields) */
#define CSI_ERR_ORDER 2u    /* a position below the one before it */
#define CSI_ERR_POS 4u      /* a text line without a tab-separated decimal position of 1 .. 2^32 - 1 */
#define CSI_ERR_INTERVAL 8u /* interval offsets that descend or lie beyond the stream */

/* one run: the layout of bsc_csi_entry (include/bscall_amd.h) */
typedef struct {
  uint32_t window, n_records;
  uint64_t u_beg;
} csi_run;

CSI_FN uint32_t csi_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

/* the record at s[p], p < end: its length (0: malformed, *err says how) and its 0-based position */
CSI_FN uint64_t csi_record(int format, const uint8_t *s, uint64_t p, uint64_t end, uint32_t *pos0, uint32_t *err) {
  if (format == CSI_FMT_BCF) {
    if (end - p < 32u) {
      *err |= CSI_ERR_STEP;
      return 0;
    }
    const uint32_t l_shared = csi_u32(s + p), l_indiv = csi_u32(s + p + 4u);
    const uint64_t step = 8u + (uint64_t)l_shared + l_indiv;
    if (l_shared < 24u || step > end - p) {
      *err |= CSI_ERR_STEP;
      return 0;
    }
    *pos0 = csi_u32(s + p + 12u);
    return step;
  }
  uint64_t q = p;
  while (q < end && s[q] != '\t' && s[q] != '\n') q++;
  if (q >= end) {
    *err |= CSI_ERR_STEP;
    return 0;
  }
  if (s[q] != '\t') {
    *err |= CSI_ERR_POS;
    return 0;
  }
  q++;
  uint64_t v = 0;
  unsigned nd = 0;
  while (q < end && s[q] >= '0' && s[q] <= '9' && nd < 11u) {
    v = v * 10u + (uint64_t)(s[q] - '0');
    nd++;
    q++;
  }
  if (q >= end) {
    *err |= CSI_ERR_STEP;
    return 0;
  }
  if (!nd || s[q] != '\t' || v == 0 || v > 0xffffffffull) {
    *err |= CSI_ERR_POS;
    return 0;
  }
  while (q < end && s[q] != '\n') q++;
  if (q >= end) {
    *err |= CSI_ERR_STEP;
    return 0;
  }
  *pos0 = (uint32_t)(v - 1u);
  return q + 1u - p;
}

/*
 * The runs of s[beg, end): returns how many there are.  out != NULL: run k goes to out[at + k] where at + k < cap (u_beg counted from
 * s, as beg and end are).  *n_rec += the records walked, *err |= what stopped the walk.  The count does not depend on out, so a counting
 * pass and a writing pass over the same bytes agree.
 */
CSI_FN uint32_t csi_walk(int format, const uint8_t *s, uint64_t beg, uint64_t end, int min_shift, csi_run *out, uint64_t at, uint64_t cap, uint32_t *n_rec,
                         uint32_t *err) {
  uint32_t runs = 0, in_run = 0, win = 0, last = 0, recs = 0;
  uint64_t run_beg = beg;
  for (uint64_t p = beg; p < end;) {
    uint32_t pos0 = 0;
    const uint64_t step = csi_record(format, s, p, end, &pos0, err);
    if (!step) break;
    if (recs && pos0 < last) {
      *err |= CSI_ERR_ORDER;
      break;
    }
    const uint32_t w = pos0 >> min_shift;
    if (in_run && w != win) { /* the run before this record is closed */
      if (out && at + runs < cap) {
        csi_run r;
        r.window = win;
        r.n_records = in_run;
        r.u_beg = run_beg;
        out[at + runs] = r;
      }
      runs++;
      in_run = 0;
    }
    if (!in_run) {
      win = w;
      run_beg = p;
    }
    in_run++;
    recs++;
    last = pos0;
    p += step;
  }
  if (in_run) {
    if (out && at + runs < cap) {
      csi_run r;
      r.window = win;
      r.n_records = in_run;
      r.u_beg = run_beg;
      out[at + runs] = r;
    }
    runs++;
  }
  *n_rec += recs;
  return runs;
}

#endif
