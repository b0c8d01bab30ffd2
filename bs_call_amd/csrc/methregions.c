/*
 * methregions.c — the per-region methylation summary on the host: the sums of a set of regions over packed records, the lines of the
 * summary, and the reader of the BED text that names the regions.  include/bscall_amd.h has the rule (site, region, sums, line).
 *
 * This is the CHECKER of the device's reduction (csrc/methregionsdev.hip): for any record bytes and any regions the device's accumulators
 * equal bsc_meth_regions_sum_recs' — tests/test_gpu_methregions.py compares them.  Plain C, a loop over regions per record (quadratic:
 * a checker), nothing shared with the device code.  The BED reader takes untrusted text: integration/methregions_san.c runs it and the
 * formatter under the address and undefined-behaviour sanitizers.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

/* the per-cytosine rule of bsc_meth_format_rec, restated: 1 and the site's a, b when the record gives a line */
static int region_site(const bsc_vcf_rec *r, const bsc_meth_params *p, uint64_t *a, uint64_t *b) {
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

int bsc_meth_regions_sum_recs(const bsc_vcf_rec *recs, size_t n, const bsc_meth_params *p, const bsc_meth_region *regions, size_t n_regions,
                              uint64_t *acc) {
  if (!p || (n && !recs) || (n_regions && (!regions || !acc))) return bsc_set_error(BSC_ERR_ARG, "bsc_meth_regions_sum_recs: NULL argument");
  if (p->contexts != BSC_METH_CPG && p->contexts != BSC_METH_ALL)
    return bsc_set_error(BSC_ERR_ARG, "bsc_meth_regions_sum_recs: contexts is %d, not BSC_METH_CPG or BSC_METH_ALL", (int)p->contexts);
  for (size_t k = 0; k < n_regions; k++)
    if (regions[k].start > regions[k].end)
      return bsc_set_error(BSC_ERR_ARG, "bsc_meth_regions_sum_recs: region %zu has start %u > end %u", k, regions[k].start, regions[k].end);
  for (size_t i = 0; i < n; i++) {
    uint64_t a, b;
    if (!region_site(&recs[i], p, &a, &b)) continue;
    const uint32_t pos = recs[i].core.pos;
    if (!pos) continue;
    const uint64_t cov = a + b, pct = (200 * a + cov) / (2 * cov);
    for (size_t k = 0; k < n_regions; k++)
      if (regions[k].start < pos && pos <= regions[k].end) {
        acc[4 * k] += 1;
        acc[4 * k + 1] += a;
        acc[4 * k + 2] += b;
        acc[4 * k + 3] += pct;
      }
  }
  return BSC_OK;
}

static int label_ok(const char *s) { /* 1 .. 255 bytes without a tab or a newline */
  const size_t l = strnlen(s, 256);
  return l >= 1 && l <= 255 && !memchr(s, '\t', l) && !memchr(s, '\n', l);
}

long bsc_meth_regions_format(const char *contig, const bsc_meth_region *regions, const char *const *names, const uint64_t *acc, size_t n, char *buf,
                             size_t cap) {
  if (!contig || (n && (!regions || !acc)) || (!buf && cap) || !label_ok(contig)) return -1;
  size_t at = 0;
  for (int pass = 0; pass < 2; pass++) { /* the length, then — if it fits — the bytes */
    at = 0;
    for (size_t k = 0; k < n; k++) {
      const char *name = names && names[k] ? names[k] : ".";
      if (!label_ok(name)) return -1;
      const uint64_t sites = acc[4 * k], A = acc[4 * k + 1], B = acc[4 * k + 2], P = acc[4 * k + 3], cov = A + B;
      char line[1024]; /* two labels of 255 bytes, eight numbers of 20 digits, ten separators */
      int m = snprintf(line, sizeof line, "%s\t%u\t%u\t%s\t%llu\t%llu\t%llu\t%llu\t", contig, regions[k].start, regions[k].end, name,
                       (unsigned long long)sites, (unsigned long long)cov, (unsigned long long)A, (unsigned long long)B);
      if (m < 0 || (size_t)m >= sizeof line) return -1;
      int t;
      if (sites && cov) {
        /* (A, B < 2^56 for any sums the device can form: 200 A + cov does not wrap) */
        t = snprintf(line + m, sizeof line - (size_t)m, "%llu\t%llu\n", (unsigned long long)((200 * A + cov) / (2 * cov)),
                     (unsigned long long)((2 * P + sites) / (2 * sites)));
      } else
        t = snprintf(line + m, sizeof line - (size_t)m, ".\t.\n");
      if (t < 0 || (size_t)(m + t) >= sizeof line) return -1;
      if (pass) memcpy(buf + at, line, (size_t)(m + t));
      at += (size_t)(m + t);
    }
    if (at > cap) break;
  }
  return (long)at;
}

/* ---- the BED reader ------------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  uint32_t contig, start, end;
  uint64_t order; /* the line's rank in the file: the sort is stable by it */
  char *name;
} bed_row;

static int bed_row_cmp(const void *pa, const void *pb) {
  const bed_row *a = pa, *b = pb;
  if (a->contig != b->contig) return a->contig < b->contig ? -1 : 1;
  if (a->start != b->start) return a->start < b->start ? -1 : 1;
  if (a->end != b->end) return a->end < b->end ? -1 : 1;
  return a->order < b->order ? -1 : (a->order > b->order);
}

void bsc_meth_bed_free(bsc_meth_bed *bed) {
  if (!bed) return;
  for (uint32_t c = 0; bed->contigs && c < bed->n_contigs; c++) free(bed->contigs[c]);
  for (uint64_t k = 0; bed->names && k < bed->n_regions; k++) free(bed->names[k]);
  free(bed->contigs);
  free(bed->first);
  free(bed->regions);
  free(bed->names);
  free(bed);
}

static char *bed_dup(const char *s, size_t n) {
  char *d = malloc(n + 1);
  if (d) {
    memcpy(d, s, n);
    d[n] = 0;
  }
  return d;
}

/* a coordinate: digits only, below 2^32 */
static int bed_coord(const char *s, size_t n, uint32_t *v) {
  if (!n || n > 10) return 0;
  uint64_t x = 0;
  for (size_t i = 0; i < n; i++) {
    if (s[i] < '0' || s[i] > '9') return 0;
    x = x * 10 + (uint64_t)(s[i] - '0');
  }
  if (x > 0xffffffffull) return 0;
  *v = (uint32_t)x;
  return 1;
}

static int bed_word(const char *s, size_t n, const char *w) { /* the line begins with the word w and a separator, or is it */
  const size_t l = strlen(w);
  return n >= l && !memcmp(s, w, l) && (n == l || s[l] == ' ' || s[l] == '\t');
}

int bsc_meth_regions_parse_bed(const char *text, size_t len, bsc_meth_bed **out) {
  if (!out || (len && !text)) return bsc_set_error(BSC_ERR_ARG, "bsc_meth_regions_parse_bed: NULL argument");
  *out = NULL;
  bed_row *rows = NULL;
  size_t n_rows = 0, cap_rows = 0;
  char **contigs = NULL;
  uint32_t n_contigs = 0, cap_contigs = 0;
  int rc = BSC_OK;
  uint64_t line_no = 0;
#define BED_FAIL(...)                              \
  do {                                             \
    rc = bsc_set_error(BSC_ERR_ARG, __VA_ARGS__);  \
    goto done;                                     \
  } while (0)
#define BED_NOMEM()                                                                           \
  do {                                                                                        \
    rc = bsc_set_error(BSC_ERR_NOMEM, "bsc_meth_regions_parse_bed: out of memory");          \
    goto done;                                                                                \
  } while (0)
  for (size_t at = 0; at < len;) {
    line_no++;
    const char *ln = text + at;
    const char *nl = memchr(ln, '\n', len - at);
    if (!nl) BED_FAIL("BED line %llu: the final line has no newline", (unsigned long long)line_no);
    size_t n = (size_t)(nl - ln);
    at += n + 1;
    if (n && ln[n - 1] == '\r') n--;
    if (!n || ln[0] == '#' || bed_word(ln, n, "track") || bed_word(ln, n, "browser")) continue;
    const char sep = memchr(ln, '\t', n) ? '\t' : ' ';
    const char *col[4];
    size_t col_n[4];
    int n_col = 0;
    for (size_t s = 0; n_col < 4;) {
      const char *e = memchr(ln + s, sep, n - s);
      col[n_col] = ln + s;
      col_n[n_col] = e ? (size_t)(e - (ln + s)) : n - s;
      n_col++;
      if (!e) break;
      s = (size_t)(e - ln) + 1;
    }
    if (n_col < 3) BED_FAIL("BED line %llu: %d columns, a region needs three (chrom, start, end)", (unsigned long long)line_no, n_col);
    if (!col_n[0]) BED_FAIL("BED line %llu: the contig's name is empty", (unsigned long long)line_no);
    if (col_n[0] > 255) BED_FAIL("BED line %llu: the contig's name is longer than 255 bytes", (unsigned long long)line_no);
    uint32_t start, end;
    if (!bed_coord(col[1], col_n[1], &start) || !bed_coord(col[2], col_n[2], &end))
      BED_FAIL("BED line %llu: a coordinate is not a decimal number below 2^32", (unsigned long long)line_no);
    if (start > end) BED_FAIL("BED line %llu: start %u > end %u", (unsigned long long)line_no, start, end);
    if (n_col == 4 && col_n[3] > 255) BED_FAIL("BED line %llu: the name is longer than 255 bytes", (unsigned long long)line_no);
    uint32_t c = 0;
    while (c < n_contigs && (strlen(contigs[c]) != col_n[0] || memcmp(contigs[c], col[0], col_n[0]))) c++;
    if (c == n_contigs) {
      if (n_contigs == cap_contigs) {
        char **g = realloc(contigs, (cap_contigs = cap_contigs ? cap_contigs * 2 : 16) * sizeof *g);
        if (!g) BED_NOMEM();
        contigs = g;
      }
      if (!(contigs[n_contigs] = bed_dup(col[0], col_n[0]))) BED_NOMEM();
      n_contigs++;
    }
    if (n_rows == cap_rows) {
      bed_row *g = realloc(rows, (cap_rows = cap_rows ? cap_rows * 2 : 256) * sizeof *g);
      if (!g) BED_NOMEM();
      rows = g;
    }
    char *name = n_col == 4 && col_n[3] ? bed_dup(col[3], col_n[3]) : bed_dup(".", 1);
    if (!name) BED_NOMEM();
    const bed_row row = {c, start, end, n_rows, name};
    rows[n_rows++] = row;
  }
  if (n_rows) qsort(rows, n_rows, sizeof *rows, bed_row_cmp);
  bsc_meth_bed *bed = calloc(1, sizeof *bed);
  if (!bed) BED_NOMEM();
  bed->first = calloc((size_t)n_contigs + 1, sizeof *bed->first);
  bed->regions = calloc(n_rows + 1, sizeof *bed->regions);
  bed->names = calloc(n_rows + 1, sizeof *bed->names);
  if (!bed->first || !bed->regions || !bed->names) {
    bsc_meth_bed_free(bed); /* (it owns nothing of rows / contigs yet) */
    BED_NOMEM();
  }
  for (size_t k = 0; k < n_rows; k++) {
    bed->regions[k].start = rows[k].start;
    bed->regions[k].end = rows[k].end;
    bed->names[k] = rows[k].name;
    bed->first[rows[k].contig + 1] = k + 1;
  }
  for (uint32_t c = 0; c < n_contigs; c++) /* (every listed contig has a row: first[c + 1] is set) */
    if (bed->first[c + 1] < bed->first[c]) bed->first[c + 1] = bed->first[c];
  bed->n_contigs = n_contigs;
  bed->contigs = contigs;
  bed->n_regions = n_rows;
  contigs = NULL;
  n_contigs = 0;
  n_rows = 0; /* the names belong to the result */
  *out = bed;
done:
  for (size_t k = 0; k < n_rows; k++) free(rows[k].name);
  free(rows);
  for (uint32_t c = 0; c < n_contigs; c++) free(contigs[c]);
  free(contigs);
  return rc;
#undef BED_FAIL
#undef BED_NOMEM
}
