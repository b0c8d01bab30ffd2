/*
 * bedidx_core.h — the line walk of the BED index scan (beddev.hip) and of its host form (tabix.c: bsc_bed_entries_host): one interval of a
 * block's methylation table — whole lines  chrom '\t' start '\t' end '\t' ... '\n' —, read line by line, each line's windows (wb = start >>
 * min_shift, wl = (end - 1) >> min_shift: a BED line is an interval and may lie in more than one window) and the runs of consecutive lines
 * that share (wb, wl).  The statements compile for the device and for a host compiler, like csidev_core.h's; include/bscall_amd.h has the rule.
 *
 * Nothing outside [beg, end) is read.  A line that does not end inside its interval, a line without its two numbers, or a start below the
 * one before it stops the walk with an error bit: the runs closed so far stand, the rest of the interval is not walked.
 */
#ifndef BSC_BEDIDX_CORE_H
#define BSC_BEDIDX_CORE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define BED_FN __host__ __device__ __forceinline__
#else
#define BED_FN static inline
#endif

#define BED_ERR_STEP 1u     /* a line that leaves its interval */
#define BED_ERR_ORDER 2u    /* a start below the one before it */
#define BED_ERR_LINE 4u     /* no two tab-separated decimal columns after the first, end <= start, end > 2^32, more than 10 digits */
#define BED_ERR_INTERVAL 8u /* interval offsets that descend or lie beyond the stream */

/* one run: the layout of bsc_bed_entry (include/bscall_amd.h) */
typedef struct {
  uint32_t win_beg, win_last, n_lines, zero;
  uint64_t u_beg;
} bed_run;

/* a decimal number of 1 .. 10 digits at s[*q], *q < end, closed by a tab (or, nl != 0, a newline): 0 and *q on the closing byte, or the
 * error bit */
BED_FN uint32_t bed_number(const uint8_t *s, uint64_t *q, uint64_t end, int nl, uint64_t *v) {
  uint64_t x = 0, p = *q;
  unsigned nd = 0;
  while (p < end && s[p] >= '0' && s[p] <= '9' && nd < 11u) {
    x = x * 10u + (uint64_t)(s[p] - '0');
    nd++;
    p++;
  }
  if (p >= end) return BED_ERR_STEP;
  if (!nd || nd > 10u || !(s[p] == '\t' || (nl && s[p] == '\n'))) return BED_ERR_LINE;
  *q = p;
  *v = x;
  return 0;
}

/* the line at s[p], p < end: its length (0: malformed, *err says how), its start and its last base (end - 1) */
BED_FN uint64_t bed_line(const uint8_t *s, uint64_t p, uint64_t end, uint32_t *start, uint32_t *last, uint32_t *err) {
  uint64_t q = p, a = 0, b = 0;
  while (q < end && s[q] != '\t' && s[q] != '\n') q++;
  if (q >= end) {
    *err |= BED_ERR_STEP;
    return 0;
  }
  if (s[q] != '\t') {
    *err |= BED_ERR_LINE;
    return 0;
  }
  q++;
  uint32_t e = bed_number(s, &q, end, 0, &a);
  if (!e) {
    q++;
    e = bed_number(s, &q, end, 1, &b);
  }
  if (e) {
    *err |= e;
    return 0;
  }
  if (b <= a || b > 0x100000000ull) {
    *err |= BED_ERR_LINE;
    return 0;
  }
  while (q < end && s[q] != '\n') q++;
  if (q >= end) {
    *err |= BED_ERR_STEP;
    return 0;
  }
  *start = (uint32_t)a;
  *last = (uint32_t)(b - 1u);
  return q + 1u - p;
}

BED_FN void bed_put(bed_run *out, uint64_t at, uint64_t cap, uint32_t wb, uint32_t wl, uint32_t n, uint64_t u) {
  if (out && at < cap) {
    bed_run r;
    r.win_beg = wb;
    r.win_last = wl;
    r.n_lines = n;
    r.zero = 0;
    r.u_beg = u;
    out[at] = r;
  }
}

/*
 * The runs of s[beg, end): returns how many there are.  out != NULL: run k goes to out[at + k] where at + k < cap (u_beg counted from s, as
 * beg and end are).  *n_lines += the lines walked, *err |= what stopped the walk.  The count does not depend on out, so a counting pass and
 * a writing pass over the same bytes agree.
 */
BED_FN uint32_t bed_walk(const uint8_t *s, uint64_t beg, uint64_t end, int min_shift, bed_run *out, uint64_t at, uint64_t cap, uint32_t *n_lines,
                         uint32_t *err) {
  uint32_t runs = 0, in_run = 0, wb = 0, wl = 0, prev = 0, lines = 0;
  uint64_t run_beg = beg;
  for (uint64_t p = beg; p < end;) {
    uint32_t start = 0, last = 0;
    const uint64_t step = bed_line(s, p, end, &start, &last, err);
    if (!step) break;
    if (lines && start < prev) {
      *err |= BED_ERR_ORDER;
      break;
    }
    const uint32_t b = start >> min_shift, l = last >> min_shift;
    if (in_run && (b != wb || l != wl)) { /* the run before this line is closed */
      bed_put(out, at + runs, cap, wb, wl, in_run, run_beg);
      runs++;
      in_run = 0;
    }
    if (!in_run) {
      wb = b;
      wl = l;
      run_beg = p;
    }
    in_run++;
    lines++;
    prev = start;
    p += step;
  }
  if (in_run) {
    bed_put(out, at + runs, cap, wb, wl, in_run, run_beg);
    runs++;
  }
  *n_lines += lines;
  return runs;
}

#endif
