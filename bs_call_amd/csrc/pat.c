/*
 * pat.c — the host form of the per-read CpG pattern table (include/bscall_amd.h: COUNTS, SITE, BYTE, STATE of the read-level CpG table;
 * ORDINAL, PATTERN, PIECES, RECORD, TOTALS, LINE): plain loops, a qsort and a run-length pass written from the rule and from nothing else, the
 * checker of the kernels of csrc/patdev.hip.  Host C alone.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

void bsc_pat_params_default(bsc_pat_params *p) {
  if (!p) return;
  p->min_sites = 1;
  p->reserved = 0;
}

int bsc_pat_count_sites(const uint8_t *codes, uint64_t contig_len, uint64_t from, uint64_t to, uint64_t *n) {
  if (!n || (contig_len && !codes)) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_count_sites: NULL argument");
  *n = 0;
  if (from < 1) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_count_sites: positions start at 1");
  if (to > contig_len) to = contig_len; /* the last position has no base behind it: p < contig_len */
  uint64_t c = 0;
  for (uint64_t p = from; p < to; p++) c += codes[p - 1] == 2 && codes[p] == 3;
  *n = c;
  return BSC_OK;
}

enum { PT_NONE = 0, PT_M = 1, PT_U = 2 };

/* BYTE(t, q): -1 = none */
static int pt_byte(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint64_t q) {
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
static int pt_state(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint32_t p) {
  if (t->bs_strand == 1) {
    const int b = pt_byte(t, seq, seq_bytes, x, y, min_qual, p);
    return b < 0 ? PT_NONE : ((b & 3) == 1 ? PT_M : ((b & 3) == 3 ? PT_U : PT_NONE));
  }
  if (t->bs_strand == 2) {
    const int b = pt_byte(t, seq, seq_bytes, x, y, min_qual, (uint64_t)p + 1);
    return b < 0 ? PT_NONE : ((b & 3) == 2 ? PT_M : ((b & 3) == 0 ? PT_U : PT_NONE));
  }
  return PT_NONE;
}

static int pt_cmp(const void *a, const void *b) {
  const bsc_pat_rec *p = a, *q = b;
  if (p->idx != q->idx) return p->idx < q->idx ? -1 : 1;
  if (p->hi != q->hi) return p->hi < q->hi ? -1 : 1;
  if (p->lo != q->lo) return p->lo < q->lo ? -1 : 1;
  return 0;
}

int bsc_pat_recs_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                      int32_t min_qual, const bsc_pat_params *p, bsc_pat_rec *rec, uint64_t cap, uint64_t *n_rec, uint64_t totals[8]) {
  if (!p || !n_rec || !ref || (nr && !tpl) || (cap && !rec)) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_recs_host: NULL argument");
  *n_rec = 0;
  if (y < x) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_recs_host: y (%u) < x (%u)", y, x);
  if (p->reserved) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_recs_host: reserved is %u, not 0", p->reserved);
  const uint64_t need = p->min_sites > 1 ? p->min_sites : 1;
  uint64_t S = 0;
  for (uint64_t q = x; q <= y; q++) S += ref[q - x] == 2 && ref[q - x + 1] == 3;
  uint32_t *site = malloc((S ? S : 1) * sizeof *site);
  uint8_t *st = malloc(S ? S : 1);
  bsc_pat_rec *pc = NULL; /* every piece, count 1 */
  uint64_t n_pc = 0, cap_pc = 0;
  int rc = BSC_OK;
  if (!site || !st) {
    rc = bsc_set_error(BSC_ERR_NOMEM, "bsc_pat_recs_host: out of memory");
    goto done;
  }
  uint64_t k = 0;
  for (uint64_t q = x; q <= y; q++)
    if (ref[q - x] == 2 && ref[q - x + 1] == 3) site[k++] = (uint32_t)q;
  uint64_t t[BSC_PAT_N_TOTALS] = {0};
  t[7] = S;
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
    uint64_t kt = 0, f = 0, l = 0;
    for (k = k0; k < k1; k++) {
      st[k] = (uint8_t)pt_state(&tpl[r], seq, seq_bytes, x, y, min_qual, site[k]);
      if (st[k] != PT_NONE) {
        if (!kt) f = k;
        l = k;
        kt++;
      }
    }
    if (kt < need) continue;
    t[2]++;
    t[6] += l - f + 1 > BSC_PAT_MAX_SITES;
    for (uint64_t a = f; a <= l; a += BSC_PAT_MAX_SITES) { /* the piece of ordinals a .. b, trimmed to a2 .. b2 */
      uint64_t b = a + BSC_PAT_MAX_SITES - 1 < l ? a + BSC_PAT_MAX_SITES - 1 : l, a2 = a, b2 = b;
      while (a2 <= b && st[a2] == PT_NONE) a2++;
      if (a2 > b) continue; /* dots alone */
      while (st[b2] == PT_NONE) b2--;
      if (n_pc == cap_pc) {
        const uint64_t nc = cap_pc ? cap_pc * 2 : 1024;
        bsc_pat_rec *np = realloc(pc, (size_t)nc * sizeof *pc);
        if (!np) {
          rc = bsc_set_error(BSC_ERR_NOMEM, "bsc_pat_recs_host: out of memory");
          goto done;
        }
        pc = np;
        cap_pc = nc;
      }
      bsc_pat_rec *o = &pc[n_pc++];
      o->idx = (uint32_t)a2;
      o->count = 1;
      o->hi = o->lo = 0;
      for (uint64_t j = a2; j <= b2; j++) {
        const uint64_t code = st[j] == PT_M ? 2 : (st[j] == PT_U ? 3 : 1);
        const unsigned at = (unsigned)(j - a2);
        if (at < 32) o->hi |= code << (62 - 2 * at);
        else o->lo |= code << (62 - 2 * (at - 32));
        t[3] += st[j] == PT_M;
        t[4] += st[j] == PT_U;
        t[5] += st[j] == PT_NONE;
      }
    }
  }
  if (n_pc > 0xffffffffull) {
    rc = bsc_set_error(BSC_ERR_RANGE, "bsc_pat_recs_host: %llu pieces in one block, more than 2^32 - 1", (unsigned long long)n_pc);
    goto done;
  }
  if (n_pc) qsort(pc, (size_t)n_pc, sizeof *pc, pt_cmp);
  uint64_t nrec = 0;
  for (uint64_t i = 0; i < n_pc;) {
    uint64_t j = i + 1;
    while (j < n_pc && !pt_cmp(&pc[i], &pc[j])) j++;
    if (nrec < cap) {
      rec[nrec] = pc[i];
      rec[nrec].count = (uint32_t)(j - i);
    }
    nrec++;
    i = j;
  }
  t[0] = nrec;
  t[1] = n_pc;
  *n_rec = nrec;
  if (totals) memcpy(totals, t, sizeof t);
done:
  free(site);
  free(st);
  free(pc);
  return rc;
}

/* the pattern's characters of a record -> s (<= 64); returns their number */
static unsigned pt_chars(const bsc_pat_rec *r, char *s) {
  unsigned n = 0;
  for (; n < BSC_PAT_MAX_SITES; n++) {
    const unsigned code = (unsigned)((n < 32 ? r->hi >> (62 - 2 * n) : r->lo >> (62 - 2 * (n - 32))) & 3u);
    if (!code) break;
    s[n] = code == 2 ? 'C' : (code == 3 ? 'T' : '.');
  }
  return n;
}

long bsc_pat_format(const char *contig, uint64_t index_base, const bsc_pat_rec *rec, size_t n, const bsc_pat_params *p, char *buf, size_t cap,
                    uint64_t totals2[2]) {
  if (!contig || !p || (n && !rec) || (cap && !buf)) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_format: NULL argument");
  if (p->reserved) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_format: reserved is %u, not 0", p->reserved);
  if (index_base > (1ull << 63)) return bsc_set_error(BSC_ERR_ARG, "bsc_pat_format: index_base above 2^63");
  const size_t cl = strlen(contig);
  if (cl < 1 || cl > 255 || strchr(contig, '\t') || strchr(contig, '\n'))
    return bsc_set_error(BSC_ERR_ARG, "bsc_pat_format: the contig's name must be 1 .. 255 bytes without tab or newline");
  char line[384]; /* the name + 98 at the most: a tab, 20 digits, a tab, 64 characters, a tab, 10 digits, '\n' */
  uint64_t bytes = 0, lines = 0;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) {
      char pat[BSC_PAT_MAX_SITES + 1];
      pat[pt_chars(&rec[i], pat)] = 0;
      const int l = snprintf(line, sizeof line, "%s\t%llu\t%s\t%u\n", contig, (unsigned long long)(index_base + rec[i].idx + 1ull), pat, rec[i].count);
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
