/*
 * bigwig.c — the methylation bigWig track on the host: the host form of a block's data stream and summaries over packed records
 * (bsc_bigwig_sections_recs), and the writer of the file (bsc_bigwig_open / _add / _finish / _close).  include/bscall_amd.h has the rule
 * (site, value, summary, stream, pyramid, file layout); everything here is written from that text.
 *
 * bsc_bigwig_sections_recs is the CHECKER of the device's kernels (csrc/bigwigdev.hip): for any record bytes the device leaves the bytes
 * and the summaries this file leaves — tests/test_gpu_bigwig.py compares them.  Plain C, nothing shared with the device code but the table
 * of the 1001 floats, which the device copies entries of.  The writer never walks the data bytes: a section's place is arithmetic on the
 * counts, the two trees and the zoom levels are arithmetic on the summaries, all in integers until a float is stored.
 * integration/bigwig_san.c drives the writer under the address and undefined-behaviour sanitizers.
 *
 * A compressed writer (bsc_bigwig_add_z) takes a block's sections as zlib streams — the device made them (csrc/zlibdev.hip) — with their
 * sizes: a section's place is the running sum of the sizes.  It deflates the zoom blocks itself at bsc_bigwig_finish (libz, compress2 at the
 * default level) and states the largest raw block in the header; integration/bigwig_z_san.c drives it under the sanitizers.
 *
 * The coverage track (bsc_bigwig_cov_sections_recs, bsc_bigwig_open_track with BSC_BW_COVERAGE) shares all of it: the host form differs in
 * the site's integer (c = min(a + b, 2^32 - 1)) and its float ((float)c, one rounding), a summary's sum of squares is 96 bits (_pad holds
 * the top 32; sum_merge carries), the writer's merged sums are unsigned __int128, and a coverage file's floats come from the exact integers
 * by bw_round_bits — integer arithmetic, rounded once.  The level writer's bytes are what they were.  integration/bigwig_cov_san.c drives
 * the coverage code under the sanitizers; bsc_bigwig_cov_sections_recs is the checker of csrc/bwcovdev.hip.
 */
#include <errno.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

/* libz is wanted by a compressed writer's bsc_bigwig_finish alone: a weak reference, so that a program of the plain writer by itself
 * (integration/bigwig_san.c as tests/test_bigwig_host.py builds it) still links without libz; the library links it. */
extern int compress2(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen, int level) __attribute__((weak));

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

#include "bbi_trees.h" /* the byte buffer, the checked pwrite, the two trees: shared with bigbed.c */

#define BW_MAGIC 0x888FFC26u
#define BW_ZBLOCK 512u /* records a zoom block */
#define BW_LEVELS 8

void bsc_bw_params_default(bsc_bw_params *p) {
  if (!p) return;
  p->items_per_section = 1024;
  p->reduction = 1024;
}

/* (float)(m / 10.0), m = 0 .. 1000: the table the device copies entries of (bsc_bigwig_sites_device uploads it verbatim) */
static float bw_value_tab[1001];
static pthread_once_t bw_value_once = PTHREAD_ONCE_INIT;
static void bw_value_make(void) {
  for (int m = 0; m <= 1000; m++) bw_value_tab[m] = (float)((double)m / 10.0);
}
const float *bsc_bw_values(void) {
  pthread_once(&bw_value_once, bw_value_make);
  return bw_value_tab;
}

static int bw_params_ok(const bsc_bw_params *p) { return p && p->items_per_section >= 1 && p->items_per_section <= 65535 && p->reduction >= 1; }

/* the per-cytosine rule of bsc_meth_format_rec, restated: 1 and the site's a, b when the record gives a line */
static int bw_site(const bsc_vcf_rec *r, const bsc_meth_params *p, uint64_t *a, uint64_t *b) {
  const bsc_vcf_core *c = &r->core;
  if (!c->emit || (c->gt != 4 && c->gt != 7)) return 0;
  if (c->cg != 'C' && !(p->contexts == BSC_METH_ALL && c->cg == 'H')) return 0;
  const int minus = c->gt == 7;
  *a = minus ? r->counts[6] : r->counts[5];
  *b = minus ? r->counts[4] : r->counts[7];
  if (*a + *b < (p->min_cov > 1 ? p->min_cov : 1)) return 0;
  if (c->phred < p->min_phred) return 0;
  if (p->pass_only && c->flt) return 0;
  return 1;
}

static void sum_first(bsc_bw_sum *s, uint32_t start, uint32_t m) {
  s->start = start;
  s->end = start + 1u;
  s->count = 1;
  s->min_m = s->max_m = m;
  s->_pad = 0;
  s->sum_m = m;
  s->sum_m2 = (uint64_t)m * m;
}

static void sum_merge(bsc_bw_sum *s, const bsc_bw_sum *t) {
  s->count += t->count;
  s->sum_m += t->sum_m;
  s->sum_m2 += t->sum_m2;
  s->_pad += t->_pad + (s->sum_m2 < t->sum_m2); /* a coverage summary's 96-bit sum of squares: the carry (a level summary's never carries) */
  if (t->min_m < s->min_m) s->min_m = t->min_m;
  if (t->max_m > s->max_m) s->max_m = t->max_m;
  if (t->start < s->start) s->start = t->start;
  if (t->end > s->end) s->end = t->end;
}

/* the host form of one track (BSC_BW_LEVEL or BSC_BW_COVERAGE) */
static int bw_sections_recs(const char *who, uint32_t track, const bsc_vcf_rec *recs, size_t n, uint32_t chrom_id, const bsc_meth_params *params,
                            const bsc_bw_params *bw_params, void *out, uint64_t cap, uint64_t *n_bytes, bsc_bw_sum *sections, uint64_t *n_sections,
                            bsc_bw_sum *zoom0, uint64_t *n_zoom0) {
  if (!params || !bw_params || !n_bytes || !n_sections || !n_zoom0 || (n && !recs) || (cap && !out) || (*n_sections && !sections) ||
      (*n_zoom0 && !zoom0))
    return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (params->contexts != BSC_METH_CPG && params->contexts != BSC_METH_ALL)
    return bsc_set_error(BSC_ERR_ARG, "%s: contexts is %d, not BSC_METH_CPG or BSC_METH_ALL", who, (int)params->contexts);
  if (!bw_params_ok(bw_params)) return bsc_set_error(BSC_ERR_ARG, "%s: items_per_section is 1 .. 65535, reduction 1 or more", who);
  const uint64_t S = bw_params->items_per_section, red = bw_params->reduction;
  const uint64_t sec_room = *n_sections, zoom_room = *n_zoom0;
  const float *val = bsc_bw_values();
  uint64_t a, b;
  /* the counts first: nothing is written unless all of it fits */
  uint64_t sites = 0, windows = 0, last_w = 0;
  for (size_t i = 0; i < n; i++) {
    if (!bw_site(&recs[i], params, &a, &b)) continue;
    const uint64_t w = (uint32_t)(recs[i].core.pos - 1u) / red;
    if (!sites || w != last_w) windows++;
    last_w = w;
    sites++;
  }
  const uint64_t secs = (sites + S - 1) / S;
  *n_bytes = 24 * secs + 8 * sites;
  *n_sections = secs;
  *n_zoom0 = windows;
  if (*n_bytes > cap || secs > sec_room || windows > zoom_room)
    return bsc_set_error(BSC_ERR_ARG, "%s: %llu bytes, %llu sections and %llu windows do not fit the room given", who, (unsigned long long)*n_bytes,
                         (unsigned long long)secs, (unsigned long long)windows);
  uint64_t rank = 0, nw = 0;
  for (size_t i = 0; i < n; i++) {
    if (!bw_site(&recs[i], params, &a, &b)) continue;
    const uint32_t start = recs[i].core.pos - 1u;
    /* the site's integer: m, or c = min(a + b, 2^32 - 1); its float: entry m of the table, or the one conversion of c */
    const uint32_t m = track == BSC_BW_COVERAGE ? (a + b > 0xffffffffull ? 0xffffffffu : (uint32_t)(a + b)) : (uint32_t)((2000 * a + (a + b)) / (2 * (a + b)));
    const float value = track == BSC_BW_COVERAGE ? (float)m : val[m];
    const uint64_t k = rank / S, in = rank % S;
    uint8_t *sec = (uint8_t *)out + k * (24 + 8 * S);
    bsc_bw_sum one;
    sum_first(&one, start, m);
    if (!in) { /* the section's first site: its header */
      const uint64_t left = sites - k * S;
      put32(sec, chrom_id);
      put32(sec + 4, start);
      put32(sec + 12, 0);
      put32(sec + 16, 1);
      sec[20] = 2;
      sec[21] = 0;
      sec[22] = (uint8_t)(left < S ? left : S);
      sec[23] = (uint8_t)((left < S ? left : S) >> 8);
      sections[k] = one;
    } else {
      sum_merge(&sections[k], &one);
    }
    put32(sec + 8, start + 1u); /* (the last site's stays) */
    put32(sec + 24 + 8 * in, start);
    memcpy(sec + 24 + 8 * in + 4, &value, 4);
    const uint64_t w = start / red;
    if (!rank || w != last_w) zoom0[nw++] = one; else sum_merge(&zoom0[nw - 1], &one);
    last_w = w;
    rank++;
  }
  return BSC_OK;
}

int bsc_bigwig_sections_recs(const bsc_vcf_rec *recs, size_t n, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bw_params *bw_params,
                             void *out, uint64_t cap, uint64_t *n_bytes, bsc_bw_sum *sections, uint64_t *n_sections, bsc_bw_sum *zoom0,
                             uint64_t *n_zoom0) {
  return bw_sections_recs("bsc_bigwig_sections_recs", BSC_BW_LEVEL, recs, n, chrom_id, params, bw_params, out, cap, n_bytes, sections, n_sections, zoom0,
                          n_zoom0);
}

int bsc_bigwig_cov_sections_recs(const bsc_vcf_rec *recs, size_t n, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bw_params *bw_params,
                                 void *out, uint64_t cap, uint64_t *n_bytes, bsc_bw_sum *sections, uint64_t *n_sections, bsc_bw_sum *zoom0,
                                 uint64_t *n_zoom0) {
  return bw_sections_recs("bsc_bigwig_cov_sections_recs", BSC_BW_COVERAGE, recs, n, chrom_id, params, bw_params, out, cap, n_bytes, sections, n_sections,
                          zoom0, n_zoom0);
}

/* ---- an exact integer to a float, rounded once -----------------------------------------------------------------------------------------
 * v as the float of `mant` significand bits (24: binary32, 53: binary64) and exponent bias `bias`, to nearest, ties to even, in integer
 * arithmetic: no intermediate type, so a sum of 96 bits is rounded once (a conversion through a double rounds twice).  Returns the
 * float's bits; a value that rounds beyond the format's range gives infinity, as the conversion does. */
typedef unsigned __int128 u128;
static uint64_t bw_round_bits(u128 v, int mant, int bias, int exp_max) {
  if (!v) return 0;
  int top = 127;
  while (!(v >> top)) top--;
  uint64_t q;
  if (top < mant) {
    q = (uint64_t)v << (mant - 1 - top); /* exact */
  } else {
    const int sh = top - (mant - 1);
    const u128 rem = v & (((u128)1 << sh) - 1), half = (u128)1 << (sh - 1);
    q = (uint64_t)(v >> sh);
    if (rem > half || (rem == half && (q & 1))) q++;
    if (q >> mant) { /* rounded up to the next power of two */
      q >>= 1;
      top++;
    }
  }
  const uint64_t e = (uint64_t)(top + bias);
  if (e >= (uint64_t)exp_max) return (uint64_t)exp_max << (mant - 1); /* infinity */
  return (e << (mant - 1)) | (q & (((uint64_t)1 << (mant - 1)) - 1));
}
static float bw_f32_of(u128 v) {
  const uint32_t bits = (uint32_t)bw_round_bits(v, 24, 127, 255);
  float f;
  memcpy(&f, &bits, 4);
  return f;
}
static double bw_f64_of(u128 v) {
  const uint64_t bits = bw_round_bits(v, 53, 1023, 2047);
  double d;
  memcpy(&d, &bits, 8);
  return d;
}
static u128 bw_sum2_of(const bsc_bw_sum *s) { return ((u128)s->_pad << 64) | s->sum_m2; }

/* ---- the writer ------------------------------------------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t tid;
  bsc_bw_sum s;
  uint64_t off;  /* a section's place in the file (not used by a zoom record) */
  uint64_t size; /* and its bytes there */
  u128 wide_m, wide_m2; /* a coverage writer's zoom record: the sums of c and of c * c as merged, held wide enough that nothing wraps */
} bw_rec;

static void rec_wide_set(bw_rec *r) {
  r->wide_m = r->s.sum_m;
  r->wide_m2 = bw_sum2_of(&r->s);
}
static void rec_merge(bw_rec *r, const bw_rec *t) {
  sum_merge(&r->s, &t->s);
  r->wide_m += t->wide_m;
  r->wide_m2 += t->wide_m2;
}

struct bsc_bigwig {
  int fd;
  uint32_t n_refs, key_size;
  char **names;
  uint32_t *lens;
  bsc_bw_params par;
  uint64_t data_start; /* fullDataOffset: the section count, the streams behind it */
  uint64_t data_bytes;
  bw_rec *sec;
  uint64_t n_sec, cap_sec;
  bw_rec *z0;
  uint64_t n_z0, cap_z0;
  int have_last, finished;
  int mode; /* 0 until the first non-empty add; then BW_PLAIN or BW_Z */
  uint32_t track; /* BSC_BW_LEVEL or BSC_BW_COVERAGE: what the summaries' integers are, and how they become floats */
  uint32_t last_tid, last_end;
};
enum { BW_PLAIN = 1, BW_Z = 2 };

static int bw_open(const char *who, int fd, uint32_t n_refs, const char *const *names, const uint32_t *lens, const bsc_bw_params *bw_params, uint32_t track,
                   bsc_bigwig **out) {
  if (out) *out = NULL;
  if (!out || fd < 0 || (n_refs && (!names || !lens))) return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (track != BSC_BW_LEVEL && track != BSC_BW_COVERAGE) return bsc_set_error(BSC_ERR_ARG, "%s: track is %u, not BSC_BW_LEVEL or BSC_BW_COVERAGE", who, track);
  if (!bw_params_ok(bw_params)) return bsc_set_error(BSC_ERR_ARG, "%s: items_per_section is 1 .. 65535, reduction 1 or more", who);
  bsc_bigwig *bw = calloc(1, sizeof *bw);
  if (!bw) return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  bw->fd = fd;
  bw->track = track;
  bw->par = *bw_params;
  bw->names = calloc(n_refs ? n_refs : 1, sizeof *bw->names);
  bw->lens = calloc(n_refs ? n_refs : 1, sizeof *bw->lens);
  int bad = !bw->names || !bw->lens;
  for (uint32_t k = 0; k < n_refs && !bad; k++) {
    if (!names[k]) {
      bsc_bigwig_close(bw);
      return bsc_set_error(BSC_ERR_ARG, "%s: contig %u has no name", who, k);
    }
    const size_t len = strlen(names[k]);
    if (len > 65535) {
      bsc_bigwig_close(bw);
      return bsc_set_error(BSC_ERR_ARG, "%s: contig %u has a name of %zu bytes", who, k, len);
    }
    bw->names[k] = malloc(len + 1);
    if (!bw->names[k]) {
      bad = 1;
      break;
    }
    memcpy(bw->names[k], names[k], len + 1);
    bw->lens[k] = lens[k];
    bw->n_refs = k + 1;
    if (len > bw->key_size) bw->key_size = (uint32_t)len;
  }
  if (bad) {
    bsc_bigwig_close(bw);
    return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  }
  bw->data_start = 296 + chrom_tree_bytes(n_refs, bw->key_size);
  *out = bw;
  return BSC_OK;
}

int bsc_bigwig_open(int fd, uint32_t n_refs, const char *const *names, const uint32_t *lens, const bsc_bw_params *bw_params, bsc_bigwig **out) {
  return bw_open("bsc_bigwig_open", fd, n_refs, names, lens, bw_params, BSC_BW_LEVEL, out);
}

int bsc_bigwig_open_track(int fd, uint32_t n_refs, const char *const *names, const uint32_t *lens, const bsc_bw_params *bw_params, uint32_t track,
                          bsc_bigwig **out) {
  return bw_open("bsc_bigwig_open_track", fd, n_refs, names, lens, bw_params, track, out);
}

void bsc_bigwig_close(bsc_bigwig *bw) {
  if (!bw) return;
  for (uint32_t k = 0; bw->names && k < bw->n_refs; k++) free(bw->names[k]);
  free(bw->names);
  free(bw->lens);
  free(bw->sec);
  free(bw->z0);
  free(bw);
}

/* bsc_bigwig_add (z_sizes NULL: data is the plain stream) and bsc_bigwig_add_z (data is the sections' zlib streams, z_sizes their lengths) */
static int bw_add(bsc_bigwig *bw, const char *who, uint32_t tid, const void *data, uint64_t n_bytes, const uint32_t *z_sizes, int z,
                  const bsc_bw_sum *sections, uint64_t n_sections, const bsc_bw_sum *zoom0, uint64_t n_zoom0) {
  if (!bw || (n_bytes && !data) || (n_sections && !sections) || (n_zoom0 && !zoom0) || (z && n_sections && !z_sizes))
    return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (bw->finished) return bsc_set_error(BSC_ERR_ARG, "%s: the file is finished", who);
  if (tid >= bw->n_refs) return bsc_set_error(BSC_ERR_ARG, "%s: contig %u of %u", who, tid, bw->n_refs);
  if (bw->have_last && tid < bw->last_tid) return bsc_set_error(BSC_ERR_ARG, "%s: contig %u behind contig %u", who, tid, bw->last_tid);
  if (!n_sections) {
    if (n_bytes || n_zoom0) return bsc_set_error(BSC_ERR_ARG, "%s: bytes or windows without a section", who);
    return BSC_OK;
  }
  if (!n_zoom0) return bsc_set_error(BSC_ERR_ARG, "%s: sections without a window", who);
  if (bw->mode && bw->mode != (z ? BW_Z : BW_PLAIN))
    return bsc_set_error(BSC_ERR_ARG, "%s: the file's sections are %s", who, bw->mode == BW_Z ? "compressed: bsc_bigwig_add_z adds to it" : "plain: bsc_bigwig_add adds to it");
  const uint64_t S = bw->par.items_per_section, red = bw->par.reduction;
  uint64_t sites = 0, zsites = 0;
  uint32_t end = bw->have_last && tid == bw->last_tid ? bw->last_end : 0;
  if (sections[0].start < end)
    return bsc_set_error(BSC_ERR_ARG, "%s: contig %u: start %u lies below the previous end %u", who, tid, sections[0].start, end);
  for (uint64_t k = 0; k < n_sections; k++) {
    const bsc_bw_sum *s = &sections[k];
    if (!s->count || s->count > S || (k + 1 < n_sections && s->count != S) || s->start < end || s->end <= s->start || s->end - s->start < s->count)
      return bsc_set_error(BSC_ERR_ARG, "%s: section %llu is not one of %llu sites in order", who, (unsigned long long)k, (unsigned long long)S);
    end = s->end;
    sites += s->count;
  }
  if (!z && 24 * n_sections + 8 * sites != n_bytes)
    return bsc_set_error(BSC_ERR_ARG, "%s: %llu sections of %llu sites are not %llu bytes", who, (unsigned long long)n_sections,
                         (unsigned long long)sites, (unsigned long long)n_bytes);
  if (z) {
    uint64_t zsum = 0;
    for (uint64_t k = 0; k < n_sections; k++) {
      if (!z_sizes[k] || z_sizes[k] > 24 + 8 * (uint64_t)sections[k].count + 11)
        return bsc_set_error(BSC_ERR_ARG, "%s: section %llu of %u sites has a stream of %u bytes", who, (unsigned long long)k, sections[k].count, z_sizes[k]);
      zsum += z_sizes[k];
    }
    if (zsum != n_bytes)
      return bsc_set_error(BSC_ERR_ARG, "%s: the streams' sizes add up to %llu bytes, not %llu", who, (unsigned long long)zsum, (unsigned long long)n_bytes);
  }
  for (uint64_t k = 0; k < n_zoom0; k++) {
    const bsc_bw_sum *z = &zoom0[k];
    if (!z->count || z->end <= z->start || (z->end - 1u) / red != z->start / red || (k && z->start / red <= zoom0[k - 1].start / red))
      return bsc_set_error(BSC_ERR_ARG, "%s: window %llu is not one window of %llu bases in order", who, (unsigned long long)k, (unsigned long long)red);
    zsites += z->count;
  }
  if (zsites != sites || zoom0[0].start != sections[0].start || zoom0[n_zoom0 - 1].end != end)
    return bsc_set_error(BSC_ERR_ARG, "%s: the windows do not hold the sections' sites", who);
  if (grow((void **)&bw->sec, &bw->cap_sec, bw->n_sec + n_sections, sizeof *bw->sec)) return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  if (grow((void **)&bw->z0, &bw->cap_z0, bw->n_z0 + n_zoom0, sizeof *bw->z0)) return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  const uint64_t base = bw->data_start + 8 + bw->data_bytes;
  if (write_all(bw->fd, data, n_bytes, base)) return bsc_set_error(BSC_ERR_ARG, "%s: write failed: %s", who, strerror(errno));
  uint64_t at = base;
  for (uint64_t k = 0; k < n_sections; k++) {
    bw_rec *r = &bw->sec[bw->n_sec++];
    r->tid = tid;
    r->s = sections[k];
    if (bw->track == BSC_BW_LEVEL) r->s._pad = 0;
    rec_wide_set(r);
    r->off = at;
    r->size = z ? z_sizes[k] : 24 + 8 * (uint64_t)sections[k].count;
    at += z ? z_sizes[k] : 24 + 8 * S;
  }
  for (uint64_t k = 0; k < n_zoom0; k++) {
    bw_rec *prev = bw->n_z0 ? &bw->z0[bw->n_z0 - 1] : NULL;
    if (!k && prev && prev->tid == tid && prev->s.start / red == zoom0[0].start / red) { /* a window two blocks share */
      bw_rec first;
      first.s = zoom0[0];
      if (bw->track == BSC_BW_LEVEL) first.s._pad = 0;
      rec_wide_set(&first);
      rec_merge(prev, &first);
      if (bw->track == BSC_BW_LEVEL) prev->s._pad = 0;
      continue;
    }
    bw->z0[bw->n_z0].tid = tid;
    bw->z0[bw->n_z0].s = zoom0[k];
    bw->z0[bw->n_z0].off = 0;
    bw->z0[bw->n_z0].size = 0;
    if (bw->track == BSC_BW_LEVEL) bw->z0[bw->n_z0].s._pad = 0;
    rec_wide_set(&bw->z0[bw->n_z0]);
    bw->n_z0++;
  }
  bw->data_bytes += n_bytes;
  bw->have_last = 1;
  bw->mode = z ? BW_Z : BW_PLAIN;
  bw->last_tid = tid;
  bw->last_end = end;
  return BSC_OK;
}

int bsc_bigwig_add(bsc_bigwig *bw, uint32_t tid, const void *data, uint64_t n_bytes, const bsc_bw_sum *sections, uint64_t n_sections,
                   const bsc_bw_sum *zoom0, uint64_t n_zoom0) {
  return bw_add(bw, "bsc_bigwig_add", tid, data, n_bytes, NULL, 0, sections, n_sections, zoom0, n_zoom0);
}

int bsc_bigwig_add_z(bsc_bigwig *bw, uint32_t tid, const void *zdata, uint64_t z_bytes, const uint32_t *z_sizes, const bsc_bw_sum *sections,
                     uint64_t n_sections, const bsc_bw_sum *zoom0, uint64_t n_zoom0) {
  return bw_add(bw, "bsc_bigwig_add_z", tid, zdata, z_bytes, z_sizes, 1, sections, n_sections, zoom0, n_zoom0);
}

/* a zoom level's records at file offset `at`: the count, the blocks — each deflated (compress2, the default level) where z —, the R-tree
 * over the blocks; *index = the tree's offset; *max_raw: raised to the largest block's raw bytes */
static int zoom_level_put(bw_buf *b, const bw_rec *r, uint64_t n, uint64_t at, uint64_t *index, int z, uint64_t *max_raw, uint32_t track) {
  const uint64_t b0 = b->n;
  rt_item *it = malloc((size_t)(n ? n : 1) * sizeof *it); /* (at most one block per record) */
  if (!it) return -1;
  uint64_t n_it = 0;
  buf_u32(b, (uint32_t)n);
  for (uint64_t i = 0; i < n;) {
    uint64_t j = i;
    while (j < n && j - i < BW_ZBLOCK && r[j].tid == r[i].tid) j++;
    rt_item v = {r[i].tid, r[i].s.start, r[i].tid, r[j - 1].s.end, at + (b->n - b0), 32 * (j - i)};
    const size_t raw_at = b->n;
    if (v.size > *max_raw) *max_raw = v.size;
    for (; i < j; i++) {
      const bsc_bw_sum *s = &r[i].s;
      buf_u32(b, r[i].tid);
      buf_u32(b, s->start);
      buf_u32(b, s->end);
      buf_u32(b, s->count);
      if (track == BSC_BW_COVERAGE) { /* each from the exact integer, once */
        buf_f32(b, bw_f32_of(s->min_m));
        buf_f32(b, bw_f32_of(s->max_m));
        buf_f32(b, bw_f32_of(r[i].wide_m));
        buf_f32(b, bw_f32_of(r[i].wide_m2));
        continue;
      }
      buf_f32(b, (float)((double)s->min_m / 10.0));
      buf_f32(b, (float)((double)s->max_m / 10.0));
      buf_f32(b, (float)((double)s->sum_m / 10.0));
      buf_f32(b, (float)((double)s->sum_m2 / 100.0));
    }
    if (z && !b->oom) { /* the block's raw bytes, just written, give way to their stream */
      uLongf zn = (uLongf)(v.size + v.size / 512 + 64); /* (above compressBound: at most 16 KiB in) */
      Bytef *zb = malloc(zn);
      if (!zb || compress2(zb, &zn, b->p + raw_at, (uLong)v.size, Z_DEFAULT_COMPRESSION) != Z_OK) {
        free(zb);
        free(it);
        return -1;
      }
      b->n = raw_at;
      uint8_t *q = buf_room(b, zn);
      if (q) memcpy(q, zb, zn);
      free(zb);
      v.size = zn;
    }
    it[n_it++] = v;
  }
  *index = at + (b->n - b0);
  const int rc = rtree_put(b, it, n_it, *index, *index, 1);
  free(it);
  return rc;
}

int bsc_bigwig_finish(bsc_bigwig *bw) {
  static const char who[] = "bsc_bigwig_finish";
  if (!bw) return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (bw->finished) return bsc_set_error(BSC_ERR_ARG, "%s: the file is finished", who);
  if (bw->n_z0 > 0xffffffffull) return bsc_set_error(BSC_ERR_ARG, "%s: more than 2^32 - 1 zoom records", who);
  if (bw->mode == BW_Z && !compress2) return bsc_set_error(BSC_ERR_ARG, "%s: a compressed file needs libz, which this program does not link", who);
  bw_buf head = {0}, tail = {0};
  int rc = 0, levels = 0;
  uint64_t z_red[BW_LEVELS] = {0}, z_data[BW_LEVELS] = {0}, z_index[BW_LEVELS] = {0};
  const uint64_t index_at = bw->data_start + 8 + bw->data_bytes;
  /* the sections' index */
  rt_item *it = malloc((size_t)(bw->n_sec ? bw->n_sec : 1) * sizeof *it);
  uint64_t covered = 0, min_m = 0, max_m = 0, sum_m = 0, sum_m2 = 0, max_raw = 0;
  u128 wide_m = 0, wide_m2 = 0; /* a coverage file's totals: nothing wraps */
  const int z = bw->mode == BW_Z;
  if (!it) rc = -1;
  for (uint64_t k = 0; k < bw->n_sec && !rc; k++) {
    const bw_rec *s = &bw->sec[k];
    const rt_item v = {s->tid, s->s.start, s->tid, s->s.end, s->off, s->size};
    it[k] = v;
    if (z && 24 + 8 * (uint64_t)s->s.count > max_raw) max_raw = 24 + 8 * (uint64_t)s->s.count;
    if (!k || s->s.min_m < min_m) min_m = s->s.min_m;
    if (!k || s->s.max_m > max_m) max_m = s->s.max_m;
    covered += s->s.count;
    sum_m += s->s.sum_m;
    sum_m2 += s->s.sum_m2;
    wide_m += s->s.sum_m;
    wide_m2 += bw_sum2_of(&s->s);
  }
  if (!rc) rc = rtree_put(&tail, it, bw->n_sec, index_at, index_at, 1);
  free(it);
  /* the pyramid */
  bw_rec *cur = bw->z0, *own = NULL;
  uint64_t n_cur = bw->n_z0, width = bw->par.reduction;
  for (int l = 0; l < BW_LEVELS && !rc; l++) {
    if (l) {
      if (n_cur <= 256) break;
      width *= 4; /* (reduction < 2^32, 4^7 = 2^14: 64 bits hold it) */
      bw_rec *next = malloc((size_t)n_cur * sizeof *next);
      if (!next) {
        rc = -1;
        break;
      }
      uint64_t m = 0;
      for (uint64_t i = 0; i < n_cur; i++) {
        if (m && next[m - 1].tid == cur[i].tid && next[m - 1].s.start / width == cur[i].s.start / width) rec_merge(&next[m - 1], &cur[i]);
        else next[m++] = cur[i];
      }
      free(own);
      cur = own = next;
      n_cur = m;
    }
    z_red[l] = width < 0xffffffffull ? width : 0xffffffffull;
    z_data[l] = index_at + tail.n;
    rc = zoom_level_put(&tail, cur, n_cur, z_data[l], &z_index[l], z, &max_raw, bw->track);
    levels = l + 1;
  }
  free(own);
  buf_u32(&tail, BW_MAGIC);
  /* the header, the zoom headers, the total summary, the chromosome tree, the section count */
  buf_u32(&head, BW_MAGIC);
  buf_u16(&head, 4);
  buf_u16(&head, (uint16_t)levels);
  buf_u64(&head, 296);
  buf_u64(&head, bw->data_start);
  buf_u64(&head, index_at);
  buf_u16(&head, 0);
  buf_u16(&head, 0);
  buf_u64(&head, 0);
  buf_u64(&head, 256);
  buf_u32(&head, z ? (uint32_t)max_raw : 0); /* uncompressBufSize: at most 24 + 8 * 65535 or 32 * 512 */
  buf_u64(&head, 0);
  for (int l = 0; l < BW_LEVELS; l++) {
    buf_u32(&head, l < levels ? (uint32_t)z_red[l] : 0);
    buf_u32(&head, 0);
    buf_u64(&head, l < levels ? z_data[l] : 0);
    buf_u64(&head, l < levels ? z_index[l] : 0);
  }
  buf_u64(&head, covered);
  if (bw->track == BSC_BW_COVERAGE) {
    buf_f64(&head, bw_f64_of(min_m));
    buf_f64(&head, bw_f64_of(max_m));
    buf_f64(&head, bw_f64_of(wide_m));
    buf_f64(&head, bw_f64_of(wide_m2));
  } else {
    buf_f64(&head, (double)min_m / 10.0);
    buf_f64(&head, (double)max_m / 10.0);
    buf_f64(&head, (double)sum_m / 10.0);
    buf_f64(&head, (double)sum_m2 / 100.0);
  }
  if (!rc) rc = chrom_tree_put(&head, bw->n_refs, bw->key_size, bw->names, bw->lens, 296);
  buf_u64(&head, bw->n_sec);
  if (!rc && (head.oom || tail.oom)) rc = -1;
  if (rc) {
    free(head.p);
    free(tail.p);
    return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  }
  if (head.n != bw->data_start + 8) {
    free(head.p);
    free(tail.p);
    return bsc_set_error(BSC_ERR_ARG, "%s: the head is %zu bytes, not %llu", who, head.n, (unsigned long long)bw->data_start + 8);
  }
  if (write_all(bw->fd, tail.p, tail.n, index_at) || write_all(bw->fd, head.p, head.n, 0))
    rc = bsc_set_error(BSC_ERR_ARG, "%s: write failed: %s", who, strerror(errno));
  free(head.p);
  free(tail.p);
  if (!rc) bw->finished = 1;
  return rc;
}
