/*
 * mbias.c — the host form of the M-bias table (include/bscall_amd.h: READ, END, CYCLE, G(j), COUNTS, CONTEXT, TABLE, TOTALS, LINE): plain
 * loops written from the rule and from nothing else, the checker of the kernel of csrc/mbiasdev.hip.  Host C alone.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

void bsc_mbias_params_default(bsc_mbias_params *p) {
  if (!p) return;
  p->n_cycles = 512;
}

static int mb_params_ok(const bsc_mbias_params *p) { return p->n_cycles >= 1 && p->n_cycles <= BSC_MBIAS_MAX_CYCLES; }

/* the list of one read, walked as G(j) says: 0 = malformed */
static int mb_list_ok(const bsc_misms *m, uint32_t n, uint32_t len) {
  uint64_t cursor = 0;
  for (uint32_t z = 0; z < n; z++) {
    const uint64_t pos = m[z].position, end = pos + m[z].size;
    switch (m[z].type) {
    case BSC_MISMS_MISMS:
      continue;
    case BSC_MISMS_SOFT:
      if (z != 0 && z != n - 1) return 0;
      /* fall through */
    case BSC_MISMS_DEL:
      if (pos < cursor || end > len) return 0;
      cursor = end;
      break;
    case BSC_MISMS_INS:
      if (pos < cursor) return 0;
      cursor = pos;
      break;
    default:
      return 0;
    }
  }
  return 1;
}

/* r(p): N outside x .. y + 2 */
static unsigned mb_ref(const uint8_t *ref, uint32_t x, uint32_t y, int64_t p) {
  if (p < (int64_t)x || p > (int64_t)y + 2) return 0;
  return ref[p - (int64_t)x];
}

int bsc_mbias_host(const bsc_raw_template *raw, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, const bsc_misms *misms, uint64_t n_misms,
                   uint32_t x, uint32_t y, const uint8_t *ref, int32_t min_qual, const bsc_mbias_params *p, uint64_t *counts, uint64_t totals[8]) {
  if (!p || !ref || !counts || (nr && !raw)) return bsc_set_error(BSC_ERR_ARG, "bsc_mbias_host: NULL argument");
  if (!mb_params_ok(p)) return bsc_set_error(BSC_ERR_ARG, "bsc_mbias_host: n_cycles (%u) outside 1 .. %u", p->n_cycles, BSC_MBIAS_MAX_CYCLES);
  if (y < x) return bsc_set_error(BSC_ERR_ARG, "bsc_mbias_host: y (%u) < x (%u)", y, x);
  const uint32_t nc = p->n_cycles;
  uint64_t t[BSC_MBIAS_N_TOTALS] = {0};
  for (uint32_t i = 0; i < nr; i++) {
    const bsc_raw_template *r = &raw[i];
    for (int k = 0; k < 2; k++) {
      const uint32_t len = r->len[k];
      if (len == 0 || r->bs_strand == 0) continue;
      const bsc_misms *m = NULL;
      int ok = seq && r->off[k] <= seq_bytes && len <= seq_bytes - r->off[k] && r->misms_off[k] <= n_misms &&
               r->n_misms[k] <= n_misms - r->misms_off[k] && (r->n_misms[k] == 0 || misms) && r->bs_strand <= 2 && r->orientation <= 1;
      if (ok) {
        m = r->n_misms[k] ? misms + r->misms_off[k] : NULL;
        ok = mb_list_ok(m, r->n_misms[k], len);
      }
      if (!ok) {
        t[6]++;
        continue;
      }
      t[0]++;
      const uint8_t *b = seq + r->off[k];
      const unsigned e = (unsigned)k ^ r->orientation, s = r->bs_strand - 1u;
      uint32_t z = 0;
      uint64_t g = r->pos[k]; /* the genome position of the next byte that is not taken out */
      const uint32_t nm = r->n_misms[k];
      for (uint32_t j = 0; j < len; j++) {
        /* the entries at j: an INS opens a gap in front of byte j, a DEL / SOFT takes bytes out from j on */
        uint32_t skip = 0;
        while (z < nm && (m[z].type == BSC_MISMS_MISMS || m[z].position <= j)) {
          if (m[z].type == BSC_MISMS_INS) g += m[z].size;
          else if (m[z].type != BSC_MISMS_MISMS) skip += m[z].size;
          z++;
          if (skip) break; /* (the next entry's position is at or behind this one's end) */
        }
        if (skip) {
          j += skip - 1;
          continue;
        }
        const uint64_t G = g++;
        if (G < x || G > y) continue;
        t[1]++;
        const int qual = b[j] >> 2;
        if (qual < min_qual || qual >= 63) continue;
        const unsigned base = b[j] & 3u;
        unsigned r0 = mb_ref(ref, x, y, (int64_t)G), n1, n2, ctx, state;
        if (s == 0) { /* C2T */
          if (r0 != 2) continue;
          n1 = mb_ref(ref, x, y, (int64_t)G + 1);
          n2 = mb_ref(ref, x, y, (int64_t)G + 2);
          if (n1 == 3) ctx = 0;
          else if (n1 == 0) continue;
          else if (n2 == 3) ctx = 1;
          else if (n2 == 0) continue;
          else ctx = 2;
          if (base == 1) state = 0;
          else if (base == 3) state = 1;
          else continue;
        } else { /* G2A */
          if (r0 != 3) continue;
          n1 = mb_ref(ref, x, y, (int64_t)G - 1);
          n2 = mb_ref(ref, x, y, (int64_t)G - 2);
          if (n1 == 2) ctx = 0;
          else if (n1 == 0) continue;
          else if (n2 == 2) ctx = 1;
          else if (n2 == 0) continue;
          else ctx = 2;
          if (base == 2) state = 0;
          else if (base == 0) state = 1;
          else continue;
        }
        const uint32_t c = k == 0 ? j : len - 1u - j;
        if (c >= nc) {
          t[3]++;
          continue;
        }
        counts[((size_t)((e * 2u + s) * 3u + ctx) * nc + c) * 2u + state]++;
        t[2]++;
        if (ctx == 0) t[4 + state]++;
      }
    }
  }
  for (int k = 0; totals && k < BSC_MBIAS_N_TOTALS; k++) totals[k] += t[k];
  return BSC_OK;
}

long bsc_mbias_format(const uint64_t *counts, const bsc_mbias_params *p, char *buf, size_t cap) {
  static const char head[] = "#read\tstrand\tcontext\tcycle\tmeth\tunmeth\n";
  static const char *const strand[2] = {"C2T", "G2A"}, *const context[3] = {"CpG", "CHG", "CHH"};
  if (!counts || !p || (cap && !buf)) return bsc_set_error(BSC_ERR_ARG, "bsc_mbias_format: NULL argument");
  if (!mb_params_ok(p)) return bsc_set_error(BSC_ERR_ARG, "bsc_mbias_format: n_cycles (%u) outside 1 .. %u", p->n_cycles, BSC_MBIAS_MAX_CYCLES);
  const uint32_t nc = p->n_cycles;
  int64_t last[2] = {-1, -1}; /* L(e) */
  for (unsigned e = 0; e < 2; e++)
    for (unsigned b = e * 6u; b < e * 6u + 6u; b++)
      for (uint32_t c = 0; c < nc; c++)
        if ((counts[((size_t)b * nc + c) * 2u] | counts[((size_t)b * nc + c) * 2u + 1u]) && (int64_t)c > last[e]) last[e] = c;
  char line[96];
  uint64_t bytes = 0;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t o = sizeof head - 1;
    if (pass) memcpy(buf, head, sizeof head - 1);
    for (unsigned e = 0; e < 2; e++)
      for (unsigned s = 0; s < 2; s++)
        for (unsigned ctx = 0; ctx < 3; ctx++)
          for (int64_t c = 0; c <= last[e]; c++) {
            const uint64_t *cell = counts + ((size_t)((e * 2u + s) * 3u + ctx) * nc + (size_t)c) * 2u;
            const int l = snprintf(line, sizeof line, "%u\t%s\t%s\t%lld\t%llu\t%llu\n", e + 1u, strand[s], context[ctx], (long long)c + 1,
                                   (unsigned long long)cell[0], (unsigned long long)cell[1]);
            if (pass) memcpy(buf + o, line, (size_t)l);
            o += (uint64_t)l;
          }
    bytes = o;
    if (!pass && bytes > cap) break; /* too small: the need, nothing written */
  }
  return (long)bytes;
}
