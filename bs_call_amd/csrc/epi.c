/*
 * epi.c — the host form of the epiallele table (include/bscall_amd.h: COUNTS, SITE, BYTE, STATE of the read-level CpG table; WINDOW, PATTERN,
 * RECORD, TOTALS, LINE): plain loops written from the rule and from nothing else, the checker of the kernels of csrc/epidev.hip.  Host C alone.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

void bsc_epi_params_default(bsc_epi_params *p) {
  if (!p) return;
  p->min_cov = 10;
  p->reserved = 0;
}

enum { EP_NONE = 0, EP_M = 1, EP_U = 2 };

/* BYTE(t, q): -1 = none */
static int ep_byte(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint64_t q) {
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
static int ep_state(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint32_t p) {
  if (t->bs_strand == 1) {
    const int b = ep_byte(t, seq, seq_bytes, x, y, min_qual, p);
    return b < 0 ? EP_NONE : ((b & 3) == 1 ? EP_M : ((b & 3) == 3 ? EP_U : EP_NONE));
  }
  if (t->bs_strand == 2) {
    const int b = ep_byte(t, seq, seq_bytes, x, y, min_qual, (uint64_t)p + 1);
    return b < 0 ? EP_NONE : ((b & 3) == 2 ? EP_M : ((b & 3) == 0 ? EP_U : EP_NONE));
  }
  return EP_NONE;
}

int bsc_epi_windows_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                         int32_t min_qual, const bsc_epi_params *p, bsc_epi_window *win, uint64_t cap, uint64_t *n_win, uint64_t totals[8]) {
  if (!p || !n_win || !ref || (nr && !tpl) || (cap && !win)) return bsc_set_error(BSC_ERR_ARG, "bsc_epi_windows_host: NULL argument");
  *n_win = 0;
  if (y < x) return bsc_set_error(BSC_ERR_ARG, "bsc_epi_windows_host: y (%u) < x (%u)", y, x);
  if (p->reserved) return bsc_set_error(BSC_ERR_ARG, "bsc_epi_windows_host: reserved is %u, not 0", p->reserved);
  /* the sites, then every window's record, whatever the room: the counts are the totals' source */
  uint64_t S = 0;
  for (uint64_t q = x; q <= y; q++) S += ref[q - x] == 2 && ref[q - x + 1] == 3;
  const uint64_t nw = S >= BSC_EPI_K ? S - (BSC_EPI_K - 1) : 0;
  uint32_t *site = malloc((S ? S : 1) * sizeof *site);
  uint8_t *st = malloc(S ? S : 1);
  bsc_epi_window *all = calloc(nw ? nw : 1, sizeof *all);
  if (!site || !st || !all) {
    free(site);
    free(st);
    free(all);
    return bsc_set_error(BSC_ERR_NOMEM, "bsc_epi_windows_host: out of memory");
  }
  uint64_t k = 0;
  for (uint64_t q = x; q <= y; q++)
    if (ref[q - x] == 2 && ref[q - x + 1] == 3) site[k++] = (uint32_t)q;
  for (uint64_t i = 0; i < nw; i++) {
    all[i].pos = site[i];
    all[i].span = site[i + BSC_EPI_K - 1] - site[i];
  }
  uint64_t t[BSC_EPI_N_TOTALS] = {0};
  t[0] = nw;
  for (uint32_t r = 0; r < nr; r++) {
    /* the sites outside [lo - 1, hi), the reads' span and the position in front of it, have no byte and so no state */
    uint64_t lo = UINT64_MAX, hi = 0;
    for (int m = 0; m < 2; m++)
      if (tpl[r].len[m]) {
        if (tpl[r].pos[m] < lo) lo = tpl[r].pos[m];
        if ((uint64_t)tpl[r].pos[m] + tpl[r].len[m] > hi) hi = (uint64_t)tpl[r].pos[m] + tpl[r].len[m];
      }
    if (lo == UINT64_MAX) continue;
    uint64_t k0 = 0, k1 = S;
    while (k0 < k1) { /* the first site at or behind lo - 1 */
      const uint64_t mid = (k0 + k1) >> 1;
      if ((uint64_t)site[mid] + 1 < lo) k0 = mid + 1; else k1 = mid;
    }
    for (k1 = k0; k1 < S && site[k1] < hi; k1++) {}
    uint64_t kt = 0;
    for (k = k0; k < k1; k++) {
      st[k] = (uint8_t)ep_state(&tpl[r], seq, seq_bytes, x, y, min_qual, site[k]);
      kt += st[k] != EP_NONE;
    }
    t[4] += kt >= BSC_EPI_K;
    int gave = 0;
    for (uint64_t i = k0; i + BSC_EPI_K <= k1; i++) { /* window i lies within the visited sites; any other holds a site without a state */
      unsigned code = 0;
      int defined = 1;
      for (unsigned j = 0; j < BSC_EPI_K; j++) {
        if (st[i + j] == EP_NONE) defined = 0;
        code |= (unsigned)(st[i + j] == EP_M) << j;
      }
      if (!defined) continue;
      all[i].c[code]++;
      t[3] += (uint64_t)__builtin_popcount(code);
      gave = 1;
    }
    t[2] += (uint64_t)gave;
  }
  for (uint64_t i = 0; i < nw; i++)
    for (int c = 0; c < 16; c++) t[1] += all[i].c[c];
  if (cap) memcpy(win, all, (size_t)(nw < cap ? nw : cap) * sizeof *all);
  *n_win = nw;
  if (totals) memcpy(totals, t, sizeof t);
  free(site);
  free(st);
  free(all);
  return BSC_OK;
}

long bsc_epi_format(const char *contig, const bsc_epi_window *win, size_t n, const bsc_epi_params *p, char *buf, size_t cap, uint64_t totals2[2]) {
  if (!contig || !p || (n && !win) || (cap && !buf)) return bsc_set_error(BSC_ERR_ARG, "bsc_epi_format: NULL argument");
  if (p->reserved) return bsc_set_error(BSC_ERR_ARG, "bsc_epi_format: reserved is %u, not 0", p->reserved);
  const size_t cl = strlen(contig);
  if (cl < 1 || cl > 255 || strchr(contig, '\t') || strchr(contig, '\n'))
    return bsc_set_error(BSC_ERR_ARG, "bsc_epi_format: the contig's name must be 1 .. 255 bytes without tab or newline");
  const uint64_t need = p->min_cov > 1 ? p->min_cov : 1;
  char line[640]; /* the name + 214 at the most */
  uint64_t bytes = 0, lines = 0;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) {
      const bsc_epi_window *w = &win[i];
      uint64_t sum = 0;
      unsigned kinds = 0;
      for (int c = 0; c < 16; c++) {
        sum += w->c[c];
        kinds += w->c[c] != 0;
      }
      if (sum < need) continue;
      int l = snprintf(line, sizeof line, "%s\t%u\t%llu\t%llu\t%u", contig, w->pos - 1u, (unsigned long long)w->pos + w->span + 1ull,
                       (unsigned long long)sum, kinds);
      for (int c = 0; c < 16; c++) l += snprintf(line + l, sizeof line - (size_t)l, "\t%u", w->c[c]);
      line[l++] = '\n';
      if (pass) memcpy(buf + o, line, (size_t)l);
      else lines++;
      o += (uint64_t)l;
    }
    bytes = o;
    if (!pass && bytes > cap) break; /* too small: the need, nothing written */
  }
  if (totals2) {
    totals2[0] = bytes;
    totals2[1] = lines;
  }
  return (long)bytes;
}
