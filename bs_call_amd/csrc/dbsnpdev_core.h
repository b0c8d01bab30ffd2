/*
 * dbsnpdev_core.h — the loaded contig of a dbSNP index as flat arrays, and the per-position / per-entry statements over them,
 * written once for the host and the device (the bamdev_core.h / fmtg_dev.h pattern): csrc/dbsnpdev.hip runs them one thread per
 * 16 positions (flags) and one thread per entry (names), bsc_dbsnp_count runs the counting on the host, and
 * tests/dbsnpdev/dbsnp_flat_host.c runs all of them on the CPU against bsc_dbsnp_flags / bsc_dbsnp_name / bsc_dbsnp_names.
 *
 * The flat form (bsc_dev_dbsnp_flatten, csrc/dbsnp.c) is ONE block of memory, so an attachment is one allocation and one upload:
 *   mask[n_bins], fq[n_bins]   the bins min_bin .. min_bin + n_bins - 1 (n_bins = the reader's bins_used: none behind it holds an entry)
 *   ent_first[n_bins + 1]      entries before the bin
 *   dig[n_entries + 1]         where the entry's bytes start in `pool`: the two bytes of an explicit prefix index, if any, then its digits
 *   txt[n_entries + 1]         where the entry's name starts in the contig's names written one behind the other — a range's table of
 *                              offsets is a subtraction, off[k] = txt[e0 + k] - txt[e0]: no scan, no atomics
 *   pre_off[n_prefixes + 1]    the prefixes' text in pre_txt
 *   ent[n_entries]             the reader's entry word: digit bytes << 8 | prefix field << 6 | bit in the bin
 *   pool, pre_txt
 * Every entry was checked when the block was made (its prefix exists, its bit is the mask's): nothing here checks again.
 */
#ifndef BSC_DBSNPDEV_CORE_H
#define BSC_DBSNPDEV_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BSC_DBF_FN static __host__ __device__ __forceinline__
#else
#define BSC_DBF_FN static inline __attribute__((unused))
#endif

typedef struct { /* what bsc_dev_dbsnp_flatten returns: the block (malloc'ed) and where its arrays start */
  void *blob;
  size_t bytes;
  uint32_t min_bin, n_bins, n_entries, n_prefixes;
  size_t o_mask, o_fq, o_ent_first, o_dig, o_txt, o_pre_off, o_ent, o_pool, o_pre_txt;
} bsc_dbsnp_flat_blob;

typedef struct { /* the arrays, in host or in device memory */
  uint32_t min_bin, n_bins, n_entries, n_prefixes;
  const uint64_t *mask, *fq;
  const uint32_t *ent_first, *dig, *txt, *pre_off;
  const uint16_t *ent;
  const uint8_t *pool;
  const char *pre_txt;
} bsc_dbsnp_flat;

#ifdef __cplusplus
extern "C" {
#endif
struct bsc_dbsnp;
/* csrc/dbsnp.c: the contig loaded in db (none, or one the index lacks: an empty block).  BSC_ERR_ARG with the position for an entry
 * whose prefix the index does not have. */
int bsc_dev_dbsnp_flatten(const struct bsc_dbsnp *db, bsc_dbsnp_flat_blob *out);
void bsc_dev_dbsnp_flat_free(bsc_dbsnp_flat_blob *b);
#ifdef __cplusplus
}
#endif

/* the arrays of a block that lies at `base` (the host block itself, or its copy in HBM) */
BSC_DBF_FN bsc_dbsnp_flat bsc_dbf_view(const bsc_dbsnp_flat_blob *b, const void *base) {
  const char *p = (const char *)base;
  bsc_dbsnp_flat v;
  v.min_bin = b->min_bin;
  v.n_bins = b->n_bins;
  v.n_entries = b->n_entries;
  v.n_prefixes = b->n_prefixes;
  v.mask = (const uint64_t *)(p + b->o_mask);
  v.fq = (const uint64_t *)(p + b->o_fq);
  v.ent_first = (const uint32_t *)(p + b->o_ent_first);
  v.dig = (const uint32_t *)(p + b->o_dig);
  v.txt = (const uint32_t *)(p + b->o_txt);
  v.pre_off = (const uint32_t *)(p + b->o_pre_off);
  v.ent = (const uint16_t *)(p + b->o_ent);
  v.pool = (const uint8_t *)(p + b->o_pool);
  v.pre_txt = p + b->o_pre_txt;
  return v;
}

/* rs_found of position x (64 bits: a range may end at 2^32 - 1 and ask for the position behind it): 0 / 1 / 3 */
BSC_DBF_FN unsigned bsc_dbf_flag(const bsc_dbsnp_flat *f, uint64_t x) {
  const uint64_t bn = x >> 6;
  if (bn < f->min_bin || bn - f->min_bin >= f->n_bins) return 0;
  const uint64_t mk = (uint64_t)1 << (x & 63u);
  const uint32_t b = (uint32_t)(bn - f->min_bin);
  if (!(f->mask[b] & mk)) return 0;
  return (f->fq[b] & mk) ? 3u : 1u;
}

/* mask and fq_mask of the 64 positions x .. x + 63, bit k = position x + k: the bin of x and the bin behind it */
BSC_DBF_FN void bsc_dbf_window(const bsc_dbsnp_flat *f, uint64_t x, uint64_t *m, uint64_t *q) {
  const uint64_t bn = x >> 6;
  const unsigned s = (unsigned)(x & 63u);
  uint64_t m0 = 0, q0 = 0, m1 = 0, q1 = 0;
  if (bn >= f->min_bin && bn - f->min_bin < f->n_bins) {
    m0 = f->mask[bn - f->min_bin];
    q0 = f->fq[bn - f->min_bin];
  }
  if (s && bn + 1 >= f->min_bin && bn + 1 - f->min_bin < f->n_bins) {
    m1 = f->mask[bn + 1 - f->min_bin];
    q1 = f->fq[bn + 1 - f->min_bin];
  }
  *m = s ? (m0 >> s) | (m1 << (64u - s)) : m0;
  *q = s ? (q0 >> s) | (q1 << (64u - s)) : q0;
}

/* four positions' bits -> their four flag bytes, the first position in the low byte */
BSC_DBF_FN uint32_t bsc_dbf_flags4(unsigned m, unsigned q) {
  const uint32_t a = (m & 1u) | ((m & 2u) << 7) | ((m & 4u) << 14) | ((m & 8u) << 21);
  const uint32_t b = (q & 1u) | ((q & 2u) << 7) | ((q & 4u) << 14) | ((q & 8u) << 21);
  return a | ((a & b) << 1);
}

/* entries at positions < x: the number of the first entry of a range that starts at x */
BSC_DBF_FN uint32_t bsc_dbf_rank(const bsc_dbsnp_flat *f, uint64_t x) {
  const uint64_t bn = x >> 6;
  if (bn < f->min_bin) return 0;
  if (bn - f->min_bin >= f->n_bins) return f->n_entries;
  const uint32_t b = (uint32_t)(bn - f->min_bin);
  const uint64_t below = ((uint64_t)1 << (x & 63u)) - 1u;
  return f->ent_first[b] + (uint32_t)__builtin_popcountll(f->mask[b] & below);
}

/* names and name bytes of x0 .. x0 + n - 1 (what bsc_dbsnp_names counts); *e0 = the first entry of the range */
BSC_DBF_FN void bsc_dbf_count(const bsc_dbsnp_flat *f, uint32_t x0, uint32_t n, uint32_t *e0, uint32_t *n_names, uint64_t *n_bytes) {
  const uint32_t a = n ? bsc_dbf_rank(f, x0) : 0u, b = n ? bsc_dbf_rank(f, (uint64_t)x0 + n) : 0u;
  *e0 = a;
  *n_names = b - a;
  *n_bytes = b > a ? (uint64_t)(f->txt[b] - f->txt[a]) : 0u;
}

/* the bin (counted from min_bin) that holds entry e < n_entries: the last one with ent_first <= e */
BSC_DBF_FN uint32_t bsc_dbf_entry_bin(const bsc_dbsnp_flat *f, uint32_t e) {
  uint32_t lo = 0, hi = f->n_bins; /* ent_first[lo] <= e < ent_first[hi] */
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (f->ent_first[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

/* the r-th (from 0) set bit of m; r < popcount(m) */
BSC_DBF_FN unsigned bsc_dbf_select(uint64_t m, unsigned r) {
  unsigned pos = 0;
  for (unsigned w = 32; w; w >>= 1) {
    const unsigned c = (unsigned)__builtin_popcountll(m & (((uint64_t)1 << w) - 1u));
    if (r >= c) {
      r -= c;
      m >>= w;
      pos += w;
    }
  }
  return pos;
}

/* the position of entry e: the select of its rank in its bin's mask */
BSC_DBF_FN uint32_t bsc_dbf_entry_pos(const bsc_dbsnp_flat *f, uint32_t e) {
  const uint32_t b = bsc_dbf_entry_bin(f, e);
  return (uint32_t)(((uint64_t)f->min_bin + b) << 6) + bsc_dbf_select(f->mask[b], e - f->ent_first[b]);
}

/* the prefix of entry e (fields 1 .. 3: the first three prefixes; field 0: a two-byte index in front of the digits, low byte first,
 * as csrc/dbsnp.c reads it) and where its digit bytes start */
BSC_DBF_FN uint32_t bsc_dbf_entry_prefix(const bsc_dbsnp_flat *f, uint32_t e, const uint8_t **digits) {
  const unsigned field = (f->ent[e] >> 6) & 3u;
  const uint8_t *p = f->pool + f->dig[e];
  if (field) {
    *digits = p;
    return field - 1u;
  }
  *digits = p + 2;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

/* the length bsc_dbsnp_name returns in *rs_len: the prefix and two characters per digit byte, the filler of an odd count included */
BSC_DBF_FN uint32_t bsc_dbf_entry_len(const bsc_dbsnp_flat *f, uint32_t e) {
  const uint8_t *d;
  const uint32_t p = bsc_dbf_entry_prefix(f, e, &d);
  return f->pre_off[p + 1] - f->pre_off[p] + 2u * (uint32_t)(f->ent[e] >> 8);
}

/* the name of entry e, bsc_dbf_entry_len(e) bytes */
BSC_DBF_FN void bsc_dbf_entry_name(const bsc_dbsnp_flat *f, uint32_t e, char *out) {
  const uint8_t *d;
  const uint32_t p = bsc_dbf_entry_prefix(f, e, &d);
  for (uint32_t i = f->pre_off[p]; i < f->pre_off[p + 1]; i++) *out++ = f->pre_txt[i];
  const unsigned nd = f->ent[e] >> 8;
  for (unsigned k = 0; k < nd; k++) { /* a BCD byte: two digits, or a digit and the filler 0xf -> NUL */
    const unsigned hi = d[k] >> 4, lo = d[k] & 15u;
    *out++ = hi < 10u ? (char)('0' + hi) : 0;
    *out++ = lo < 10u ? (char)('0' + lo) : 0;
  }
}

#endif
