/*
 * cpgreads.c — the host form of the read-level CpG concordance table (include/bscall_amd.h: COUNTS, SITE, BYTE, STATE, RECORD, TOTALS, LINE):
 * plain loops written from the rule and from nothing else, the checker of the kernels of csrc/cpgreadsdev.hip.  Host C alone.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

void bsc_cpg_reads_params_default(bsc_cpg_reads_params *p) {
  if (!p) return;
  p->min_sites = 4;
  p->min_cov = 1;
}

enum { CR_NONE = 0, CR_M = 1, CR_U = 2 };

/* BYTE(t, q): -1 = none */
static int cr_byte(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint64_t q) {
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
static int cr_state(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint32_t p) {
  if (t->bs_strand == 1) {
    const int b = cr_byte(t, seq, seq_bytes, x, y, min_qual, p);
    return b < 0 ? CR_NONE : ((b & 3) == 1 ? CR_M : ((b & 3) == 3 ? CR_U : CR_NONE));
  }
  if (t->bs_strand == 2) {
    const int b = cr_byte(t, seq, seq_bytes, x, y, min_qual, (uint64_t)p + 1);
    return b < 0 ? CR_NONE : ((b & 3) == 2 ? CR_M : ((b & 3) == 0 ? CR_U : CR_NONE));
  }
  return CR_NONE;
}

int bsc_cpg_reads_sites_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                             int32_t min_qual, const bsc_cpg_reads_params *p, bsc_cpg_reads_site *sites, uint64_t cap, uint64_t *n_sites,
                             uint64_t totals[8]) {
  if (!p || !n_sites || !ref || (nr && !tpl) || (cap && !sites)) return bsc_set_error(BSC_ERR_ARG, "bsc_cpg_reads_sites_host: NULL argument");
  *n_sites = 0;
  if (y < x) return bsc_set_error(BSC_ERR_ARG, "bsc_cpg_reads_sites_host: y (%u) < x (%u)", y, x);
  if (p->min_sites == 0) return bsc_set_error(BSC_ERR_ARG, "bsc_cpg_reads_sites_host: min_sites is 0");
  /* every site's record, whatever the room: the counts are the totals' source */
  uint64_t n = 0;
  for (uint64_t q = x; q <= y; q++) n += ref[q - x] == 2 && ref[q - x + 1] == 3;
  bsc_cpg_reads_site *all = calloc(n ? n : 1, sizeof *all);
  uint8_t *st = malloc(n ? n : 1);
  if (!all || !st) {
    free(all);
    free(st);
    return bsc_set_error(BSC_ERR_NOMEM, "bsc_cpg_reads_sites_host: out of memory");
  }
  uint64_t k = 0;
  for (uint64_t q = x; q <= y; q++)
    if (ref[q - x] == 2 && ref[q - x + 1] == 3) all[k++].pos = (uint32_t)q;
  for (k = 0; k + 1 < n; k++) all[k].dist = all[k + 1].pos - all[k].pos;
  uint64_t t[BSC_CPG_READS_N_TOTALS] = {0};
  t[0] = n;
  for (uint32_t i = 0; i < nr; i++) {
    uint64_t kt = 0, n_m = 0, n_u = 0;
    /* the sites outside [lo - 1, hi], the reads' span and the position in front of it, have no byte and so no state: they are not visited */
    uint64_t lo = UINT64_MAX, hi = 0;
    for (int r = 0; r < 2; r++)
      if (tpl[i].len[r]) {
        if (tpl[i].pos[r] < lo) lo = tpl[i].pos[r];
        if ((uint64_t)tpl[i].pos[r] + tpl[i].len[r] > hi) hi = (uint64_t)tpl[i].pos[r] + tpl[i].len[r];
      }
    if (lo == UINT64_MAX) continue;
    uint64_t k0 = 0, k1 = n;
    while (k0 < k1) { /* the first site at or behind lo - 1 */
      const uint64_t mid = (k0 + k1) >> 1;
      if ((uint64_t)all[mid].pos + 1 < lo) k0 = mid + 1; else k1 = mid;
    }
    for (k1 = k0; k1 < n && all[k1].pos < hi; k1++) {}
    for (k = k0; k < k1; k++) {
      st[k] = (uint8_t)cr_state(&tpl[i], seq, seq_bytes, x, y, min_qual, all[k].pos);
      kt += st[k] != CR_NONE;
      n_m += st[k] == CR_M;
      n_u += st[k] == CR_U;
    }
    const int elig = kt >= p->min_sites, disc = elig && n_m && n_u;
    t[4] += kt >= 1;
    t[5] += elig;
    t[6] += disc;
    for (k = k0; k < k1; k++) {
      if (st[k] == CR_NONE) continue;
      bsc_cpg_reads_site *s = &all[k];
      if (st[k] == CR_M) s->m++; else s->u++;
      s->e += elig;
      s->d += disc;
      if (k + 1 < k1 && st[k + 1] != CR_NONE) { /* (a NEXT behind the span has no state) */
        if (st[k] == CR_M) { if (st[k + 1] == CR_M) s->mm++; else s->mu++; }
        else { if (st[k + 1] == CR_M) s->um++; else s->uu++; }
      }
    }
  }
  for (k = 0; k < n; k++) {
    t[1] += all[k].m;
    t[2] += all[k].u;
    t[3] += (uint64_t)all[k].mm + all[k].mu + all[k].um + all[k].uu;
  }
  if (cap) memcpy(sites, all, (size_t)(n < cap ? n : cap) * sizeof *all);
  *n_sites = n;
  if (totals) memcpy(totals, t, sizeof t);
  free(all);
  free(st);
  return BSC_OK;
}

static int cr_line_written(const bsc_cpg_reads_site *s, const bsc_cpg_reads_params *p) {
  return (uint64_t)s->m + s->u >= (uint64_t)(p->min_cov > 1 ? p->min_cov : 1);
}

long bsc_cpg_reads_format(const char *contig, const bsc_cpg_reads_site *sites, size_t n, const bsc_cpg_reads_params *p, char *buf, size_t cap,
                          uint64_t totals2[2]) {
  if (!contig || !p || (n && !sites) || (cap && !buf)) return bsc_set_error(BSC_ERR_ARG, "bsc_cpg_reads_format: NULL argument");
  const size_t cl = strlen(contig);
  if (cl < 1 || cl > 255 || strchr(contig, '\t') || strchr(contig, '\n'))
    return bsc_set_error(BSC_ERR_ARG, "bsc_cpg_reads_format: the contig's name must be 1 .. 255 bytes without tab or newline");
  char line[512];
  uint64_t bytes = 0, lines = 0;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) {
      const bsc_cpg_reads_site *s = &sites[i];
      if (!cr_line_written(s, p)) continue;
      const int l = snprintf(line, sizeof line, "%s\t%u\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", contig, s->pos - 1u,
                             (unsigned long long)s->pos + 1ull, s->m, s->u, s->e, s->d, s->dist, s->mm, s->mu, s->um, s->uu);
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
