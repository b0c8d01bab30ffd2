/*
 * frag.c — the host form of the per-region fragment methylation summary (include/bscall_amd.h: COUNTS, SITE, BYTE, STATE of the read-level
 * CpG table, REGION of the region summary; IN, the classes, SUMS, TOTALS, LINE): plain loops written from the rule and from nothing else,
 * the checker of the kernel of csrc/fragdev.hip.  Host C alone.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

void bsc_frag_params_default(bsc_frag_params *p) {
  if (!p) return;
  p->min_sites = 3;
  p->u_max_pct = 25;
  p->m_min_pct = 75;
  p->reserved = 0;
}

enum { FR_NONE = 0, FR_M = 1, FR_U = 2 };
enum { FR_FRAGS = 0, FR_CU = 1, FR_CX = 2, FR_CM = 3, FR_K = 4, FR_MM = 5, FR_DISC = 6, FR_SHORT = 7 };

/* BYTE(t, q): -1 = none */
static int fr_byte(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint64_t q) {
  if (q < x || q > y) return -1;
  for (int k = 0; k < 2; k++) {
    if (t->len[k] == 0 || t->off[k] > seq_bytes || (uint64_t)t->len[k] > seq_bytes - t->off[k]) continue;
    if ((uint64_t)t->pos[k] > q || q - t->pos[k] >= (uint64_t)t->len[k]) continue;
    const unsigned b = seq[t->off[k] + (q - t->pos[k])];
    const int qual = (int)(b >> 2);
    if (qual >= min_qual && qual < 63) return (int)b;
  }
  return -1;
}

/* STATE(t, s) for the site at p */
static int fr_state(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint32_t p) {
  if (t->bs_strand == 1) {
    const int b = fr_byte(t, seq, seq_bytes, x, y, min_qual, p);
    return b < 0 ? FR_NONE : ((b & 3) == 1 ? FR_M : ((b & 3) == 3 ? FR_U : FR_NONE));
  }
  if (t->bs_strand == 2) {
    const int b = fr_byte(t, seq, seq_bytes, x, y, min_qual, (uint64_t)p + 1);
    return b < 0 ? FR_NONE : ((b & 3) == 2 ? FR_M : ((b & 3) == 0 ? FR_U : FR_NONE));
  }
  return FR_NONE;
}

/* the one check of the parameters: the host form's and, through bscall_api.c, every context entry's (not in the header: p is not NULL) */
int bsc_frag_params_bad(const char *who, const bsc_frag_params *p) {
  if (p->min_sites == 0) return bsc_set_error(BSC_ERR_ARG, "%s: min_sites is 0", who);
  if (p->u_max_pct > 100 || p->m_min_pct > 100)
    return bsc_set_error(BSC_ERR_ARG, "%s: a percentage above 100 (u_max_pct %u, m_min_pct %u)", who, p->u_max_pct, p->m_min_pct);
  if (p->u_max_pct >= p->m_min_pct) return bsc_set_error(BSC_ERR_ARG, "%s: u_max_pct (%u) is not below m_min_pct (%u)", who, p->u_max_pct, p->m_min_pct);
  if (p->reserved) return bsc_set_error(BSC_ERR_ARG, "%s: reserved is %u, not 0", who, p->reserved);
  return BSC_OK;
}

int bsc_frag_regions_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                          int32_t min_qual, const bsc_frag_params *p, const bsc_meth_region *regions, size_t n_regions, uint64_t *acc,
                          uint64_t totals[8]) {
  static const char who[] = "bsc_frag_regions_host";
  int rc;
  if (!p || !ref || (nr && !tpl) || (n_regions && (!regions || !acc))) return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (y < x) return bsc_set_error(BSC_ERR_ARG, "%s: y (%u) < x (%u)", who, y, x);
  if ((rc = bsc_frag_params_bad(who, p))) return rc;
  for (size_t r = 0; r < n_regions; r++)
    if (regions[r].start > regions[r].end)
      return bsc_set_error(BSC_ERR_ARG, "%s: region %llu has start %u > end %u", who, (unsigned long long)r, regions[r].start, regions[r].end);
  uint64_t S = 0;
  for (uint64_t q = x; q <= y; q++) S += ref[q - x] == 2 && ref[q - x + 1] == 3;
  uint32_t *site = malloc((S ? S : 1) * sizeof *site);
  uint8_t *st = malloc(S ? S : 1);
  if (!site || !st) {
    free(site);
    free(st);
    return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  }
  uint64_t n = 0;
  for (uint64_t q = x; q <= y; q++)
    if (ref[q - x] == 2 && ref[q - x + 1] == 3) site[n++] = (uint32_t)q;
  uint64_t t[BSC_FRAG_N_TOTALS] = {0};
  for (uint32_t i = 0; i < nr; i++) {
    /* the sites outside [lo - 1, hi), the reads' span and the position in front of it, have no byte and so no state */
    uint64_t lo = UINT64_MAX, hi = 0;
    for (int m = 0; m < 2; m++)
      if (tpl[i].len[m]) {
        if (tpl[i].pos[m] < lo) lo = tpl[i].pos[m];
        if ((uint64_t)tpl[i].pos[m] + tpl[i].len[m] > hi) hi = (uint64_t)tpl[i].pos[m] + tpl[i].len[m];
      }
    if (lo == UINT64_MAX) continue;
    uint64_t k0 = 0, k1 = S;
    while (k0 < k1) { /* the first site at or behind lo - 1 */
      const uint64_t mid = (k0 + k1) >> 1;
      if ((uint64_t)site[mid] + 1 < lo) k0 = mid + 1; else k1 = mid;
    }
    for (k1 = k0; k1 < S && site[k1] < hi; k1++) {}
    uint64_t kt = 0;
    for (uint64_t s = k0; s < k1; s++) {
      st[s] = (uint8_t)fr_state(&tpl[i], seq, seq_bytes, x, y, min_qual, site[s]);
      kt += st[s] != FR_NONE;
    }
    if (!kt) continue;
    t[0]++;
    for (size_t r = 0; r < n_regions; r++) {
      uint64_t k = 0, m = 0;
      for (uint64_t s = k0; s < k1; s++)
        if (regions[r].start < site[s] && site[s] <= regions[r].end && st[s] != FR_NONE) {
          k++;
          m += st[s] == FR_M;
        }
      if (!k) continue;
      uint64_t *a = acc + (size_t)r * BSC_FRAG_N_SUMS;
      if (k < p->min_sites) {
        a[FR_SHORT]++;
        continue;
      }
      const int cls = 100u * m <= (uint64_t)p->u_max_pct * k ? FR_CU : (100u * m >= (uint64_t)p->m_min_pct * k ? FR_CM : FR_CX);
      const uint64_t disc = m > 0 && m < k;
      a[FR_FRAGS]++;
      a[cls]++;
      a[FR_K] += k;
      a[FR_MM] += m;
      a[FR_DISC] += disc;
      t[1 + FR_FRAGS]++;
      t[1 + cls]++;
      t[1 + FR_K] += k;
      t[1 + FR_MM] += m;
      t[1 + FR_DISC] += disc;
    }
  }
  if (totals) memcpy(totals, t, sizeof t);
  free(site);
  free(st);
  return BSC_OK;
}

/* a contig or a region's name: 1 .. 255 bytes without tab or newline, as bsc_meth_regions_format asks */
static int fr_label_ok(const char *s) {
  const size_t n = strlen(s);
  return n >= 1 && n <= 255 && !strchr(s, '\t') && !strchr(s, '\n');
}

long bsc_frag_format(const char *contig, const bsc_meth_region *regions, const char *const *names, const uint64_t *acc, size_t n, char *buf,
                     size_t cap) {
  if (!contig || (n && (!regions || !acc)) || (!buf && cap) || !fr_label_ok(contig)) return -1;
  size_t at = 0;
  for (int pass = 0; pass < 2; pass++) { /* the length, then — if it fits — the bytes */
    at = 0;
    for (size_t k = 0; k < n; k++) {
      const char *name = names && names[k] ? names[k] : ".";
      if (!fr_label_ok(name)) return -1;
      const uint64_t *a = acc + k * BSC_FRAG_N_SUMS;
      char line[1024]; /* two labels of 255 bytes, two numbers of 10 and eight of 20 digits, twelve separators */
      const int m = snprintf(line, sizeof line, "%s\t%u\t%u\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", contig, regions[k].start, regions[k].end,
                             name, (unsigned long long)a[0], (unsigned long long)a[1], (unsigned long long)a[2], (unsigned long long)a[3],
                             (unsigned long long)a[4], (unsigned long long)a[5], (unsigned long long)a[6], (unsigned long long)a[7]);
      if (m < 0 || (size_t)m >= sizeof line) return -1;
      if (pass) memcpy(buf + at, line, (size_t)m);
      at += (size_t)m;
    }
    if (at > cap) break;
  }
  return (long)at;
}
