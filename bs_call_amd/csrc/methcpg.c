/*
 * methcpg.c — host-side rendering of a block's records as the combined-strand CpG table: one bedMethyl line per CpG dinucleotide,
 * the counts of the C at p ('+' strand) and of the G at p + 1 (the '-' strand's C) added.  The reference pairs the two cytosines for
 * its report only (prev_cpg_x, src/print_vcf.c:442-475); include/bscall_amd.h states the rule — halves, pairs and singles, which
 * records give a line, the columns — and this file is written from that text.
 *
 * This is the CHECKER of the device's encoder (csrc/methdev.hip: bsc_meth_cpg_size_kernel / _write_kernel): the device writes, for any
 * array of 128-byte records, exactly the table this file writes; tests/test_gpu_methcpg.py compares them.  Plain C over the C
 * library's formatter, nothing shared with the device code (nor with csrc/methbed.c beyond the parameter block).
 */
#include <stdio.h>
#include <string.h>

#include "../../include/bscall_amd.h"

static const char *const CPG_RGB[11] = {"0,255,0",   "55,255,0",  "105,255,0", "155,255,0", "205,255,0", "255,255,0",
                                        "255,205,0", "255,155,0", "255,105,0", "255,55,0",  "255,0,0"};

typedef struct {
  int minus;
  uint64_t a, b;
} cpg_half;

/* is recs[i] a half?  (the per-cytosine rule for a CpG, without the coverage threshold) */
static int cpg_half_of(const bsc_vcf_rec *r, const bsc_meth_params *p, cpg_half *h) {
  const bsc_vcf_core *c = &r->core;
  if (!c->emit || (c->gt != 4 && c->gt != 7) || c->cg != 'C') return 0;
  if (c->phred < p->min_phred || (p->pass_only && c->flt)) return 0;
  h->minus = c->gt == 7;
  h->a = h->minus ? r->counts[6] : r->counts[5];
  h->b = h->minus ? r->counts[4] : r->counts[7];
  return h->a + h->b >= 1;
}

long bsc_meth_cpg_format_recs(const bsc_vcf_rec *recs, size_t n, const char *contig, const bsc_meth_params *p, char *buf, size_t cap,
                              uint64_t totals[5]) {
  if ((!recs && n) || !contig || !p || (!buf && cap)) return -1;
  if (p->contexts != BSC_METH_CPG) return -1; /* (BSC_METH_ALL: no partner strand outside a CpG) */
  const size_t cl = strnlen(contig, 256);
  if (cl == 0 || cl > 255 || memchr(contig, '\t', cl) || memchr(contig, '\n', cl)) return -1;
  const uint64_t min_cov = p->min_cov > 1 ? p->min_cov : 1;
  uint64_t tot[5] = {0, 0, 0, 0, 0};
  /* two passes over the same rule: the length first — nothing is written unless the whole table fits */
  for (int pass = 0; pass < 2; pass++) {
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
      cpg_half h, o;
      if (!cpg_half_of(&recs[i], p, &h)) continue;
      const uint64_t pos = recs[i].core.pos;
      if (h.minus && i > 0 && cpg_half_of(&recs[i - 1], p, &o) && !o.minus && (uint64_t)recs[i - 1].core.pos + 1 == pos) continue; /* its pair's line is the plus half's */
      uint64_t A = h.a, B = h.b;
      unsigned gq = recs[i].core.phred, flt = recs[i].core.flt;
      const int pair = !h.minus && i + 1 < n && cpg_half_of(&recs[i + 1], p, &o) && o.minus && (uint64_t)recs[i + 1].core.pos == pos + 1;
      if (pair) {
        A += o.a;
        B += o.b;
        if (recs[i + 1].core.phred < gq) gq = recs[i + 1].core.phred;
        flt |= recs[i + 1].core.flt;
      }
      const uint64_t cov = A + B;
      if (cov < min_cov) continue;
      const uint64_t pct = (200 * A + cov) / (2 * cov);
      const uint32_t start = (uint32_t)pos - (h.minus ? 2u : 1u); /* modulo 2^32, as the per-cytosine line's pos - 1 */
      const uint64_t end = (uint64_t)start + 2;
      char line[512]; /* the contig's name + 111 at most */
      const int len = snprintf(line, sizeof line, "%s\t%llu\t%llu\tCG\t%llu\t%c\t%llu\t%llu\t%s\t%llu\t%llu\t%llu\t%llu\t%u\t%s\n", contig,
                               (unsigned long long)start, (unsigned long long)end, (unsigned long long)(cov < 1000 ? cov : 1000),
                               pair ? '.' : (h.minus ? '-' : '+'), (unsigned long long)start, (unsigned long long)end, CPG_RGB[pct / 10],
                               (unsigned long long)cov, (unsigned long long)pct, (unsigned long long)A, (unsigned long long)B, gq,
                               (flt & 127) ? "fail" : ((flt & 128) ? "mac1" : "PASS"));
      if (len < 0 || (size_t)len >= sizeof line) return -1;
      if (pass) memcpy(buf + at, line, (size_t)len);
      else tot[1]++, tot[2] += A, tot[3] += B, tot[4] += (uint64_t)pair;
      at += (size_t)len;
    }
    if (!pass) {
      tot[0] = at;
      if (totals) memcpy(totals, tot, sizeof tot);
      if (at > cap) break;
    }
  }
  return (long)tot[0];
}
