/*
 * asm.c — the host form of the allele-specific methylation table (include/bscall_amd.h: SNP, ALLELE, WINDOW, RECORD, AQ, TOTALS, LINE on top of
 * COUNTS, SITE, BYTE and STATE): plain loops written from the rule and from nothing else, the checker of the kernels of csrc/asmdev.hip.
 * Fisher's test is written from fisher_dev's statements (csrc/callmath.h) with the host forms of bsmath.h.  Host C alone.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bscall_amd.h"
#include "bsmath.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

void bsc_asm_params_default(bsc_asm_params *p) {
  if (!p) return;
  p->min_phred = 20;
  p->pass_only = 0;
  p->max_dist = 500;
  p->min_cov = 2;
}

enum { AS_NONE = 0, AS_M = 1, AS_U = 2 };

/* BYTE(t, q): -1 = none */
static int as_byte(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint64_t q) {
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
static int as_state(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint32_t p) {
  if (t->bs_strand == 1) {
    const int b = as_byte(t, seq, seq_bytes, x, y, min_qual, p);
    return b < 0 ? AS_NONE : ((b & 3) == 1 ? AS_M : ((b & 3) == 3 ? AS_U : AS_NONE));
  }
  if (t->bs_strand == 2) {
    const int b = as_byte(t, seq, seq_bytes, x, y, min_qual, (uint64_t)p + 1);
    return b < 0 ? AS_NONE : ((b & 3) == 2 ? AS_M : ((b & 3) == 0 ? AS_U : AS_NONE));
  }
  return AS_NONE;
}

static const char as_gt_letters[10][3] = {"AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT"};

static int as_base_of(char c) { return c == 'A' ? 0 : (c == 'C' ? 1 : (c == 'G' ? 2 : 3)); }

/* ALLELE(t, h) */
static int as_allele(const bsc_template *t, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, int32_t min_qual, uint32_t h, unsigned gt) {
  const int bs = t->bs_strand;
  if (bs != 1 && bs != 2) return 0;
  if ((bs == 1 && gt == 6) || (bs == 2 && gt == 2)) return 0;
  const int byte = as_byte(t, seq, seq_bytes, x, y, min_qual, h);
  if (byte < 0) return 0;
  const int b = byte & 3;
  int set[4] = {0, 0, 0, 0}; /* the genome bases b may stand for */
  set[b] = 1;
  if (bs == 1 && b == 3) set[1] = 1; /* a read T of a C2T template: C or T */
  if (bs == 2 && b == 0) set[2] = 1; /* a read A of a G2A template: G or A */
  const int in1 = set[as_base_of(as_gt_letters[gt][0])], in2 = set[as_base_of(as_gt_letters[gt][1])];
  return in1 == in2 ? 0 : (in1 ? 1 : 2);
}

static int as_is_snp(const bsc_vcf_core *c, const uint8_t *emit, uint64_t i, const bsc_asm_params *p) {
  if (c[i].emit == 0 || (emit && emit[i] == 0)) return 0;
  const unsigned gt = c[i].gt;
  if (!(gt == 1 || gt == 2 || gt == 3 || gt == 5 || gt == 6 || gt == 8)) return 0;
  return c[i].phred >= p->min_phred && (!p->pass_only || c[i].flt == 0);
}

/* ---- AQ: fisher_dev's statements, a point term clamped as the rule says ------------------------------------------------------------------------ */
static double as_lf(int v, const double *lf) { return v < 256 ? lf[v] : bsm_lfact_big(v); }

static double as_point(double arg) { return arg < -700.0 ? 0.0 : bsm_exp(arg); }

static double as_fisher(int c0, int c1, int c2, int c3, const double *lf) {
#define LF(v) as_lf((v), lf)
  const int row0 = c0 + c1, row1 = c2 + c3, col0 = c0 + c2, col1 = c1 + c3;
  const int n = row0 + row1;
  if (n == 0) return 1.0;
  const double delta = (double)c0 - (double)(row0 * col0) / (double)n;
  const double knst = LF(col0) + LF(col1) + LF(row0) + LF(row1) - LF(n);
  double l = as_point(knst - LF(c0) - LF(c1) - LF(c2) - LF(c3));
  double p = l;
  if (delta > 0.0) {
    int mn = c1 < c2 ? c1 : c2;
    for (int i = 0; i < mn; i++) {
      l *= (double)((c1 - i) * (c2 - i)) / (double)((c0 + i + 1) * (c3 + i + 1));
      p += l;
    }
    mn = c0 < c3 ? c0 : c3;
    const int k = (int)ceil(2.0 * delta);
    if (k <= mn) {
      c0 -= k; c3 -= k; c1 += k; c2 += k;
      l = as_point(knst - LF(c0) - LF(c1) - LF(c2) - LF(c3));
      p += l;
      for (int i = 0; i < mn - k; i++) {
        l *= (double)((c0 - i) * (c3 - i)) / (double)((c1 + i + 1) * (c2 + i + 1));
        p += l;
      }
    }
  } else {
    int mn = c0 < c3 ? c0 : c3;
    for (int i = 0; i < mn; i++) {
      l *= (double)((c0 - i) * (c3 - i)) / (double)((c1 + i + 1) * (c2 + i + 1));
      p += l;
    }
    mn = c1 < c2 ? c1 : c2;
    int k = (int)ceil(-2.0 * delta);
    if (!k) k = 1;
    if (k <= mn) {
      c0 += k; c3 += k; c1 -= k; c2 -= k;
      l = as_point(knst - LF(c0) - LF(c1) - LF(c2) - LF(c3));
      p += l;
      for (int i = 0; i < mn - k; i++) {
        l *= (double)((c1 - i) * (c2 - i)) / (double)((c0 + i + 1) * (c3 + i + 1));
        p += l;
      }
    }
  }
  return p;
#undef LF
}

/* Fisher's p of one table by the rule's statements (the clamp included): what the tests compare with the reference's own */
double bsc_asm_fisher_p(const int32_t c[4], const double *lfact_256) {
  if (!c || !lfact_256 || c[0] < 0 || c[1] < 0 || c[2] < 0 || c[3] < 0 || (int64_t)c[0] + c[1] + c[2] + c[3] > 46340) return -1.0; /* no p is negative */
  return as_fisher(c[0], c[1], c[2], c[3], lfact_256);
}

/* DEEP and aq of a record whose counts are final */
static void as_finish(bsc_asm_pair *r, const double *lf) {
  if ((r->info >> 8) & BSC_ASM_OVERLAPPED) return;
  const uint64_t sum = (uint64_t)r->m1 + r->u1 + r->m2 + r->u2;
  if (sum > 46340) {
    r->info |= BSC_ASM_DEEP << 8;
    r->aq = 0;
    return;
  }
  const double z = as_fisher((int)r->m1, (int)r->u1, (int)r->m2, (int)r->u2, lf);
  r->aq = z >= 1.0e-100 ? (uint32_t)(int)(-(bsm_log(z) / BSM_LN10) * 10.0 + 0.5) : 1000u;
}

int bsc_asm_pairs_host(const bsc_template *tpl, uint32_t nr, const uint8_t *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, const uint8_t *ref,
                       int32_t min_qual, const bsc_vcf_core *core, const uint8_t *emit, const double *lfact_256, const bsc_asm_params *p,
                       bsc_asm_pair *pairs, uint64_t cap, uint64_t *n_pairs, uint64_t totals[8]) {
  static const char who[] = "bsc_asm_pairs_host";
  if (!p || !n_pairs || !ref || !core || !lfact_256 || (nr && !tpl) || (cap && !pairs)) return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  *n_pairs = 0;
  if (y < x) return bsc_set_error(BSC_ERR_ARG, "%s: y (%u) < x (%u)", who, y, x);
  if (p->max_dist < 1 || p->max_dist > 65535) return bsc_set_error(BSC_ERR_ARG, "%s: max_dist %u is not 1 .. 65535", who, p->max_dist);
  const uint64_t n = (uint64_t)y - x + 1, W = p->max_dist;
  /* the sites and the SNPs, as block indices */
  uint64_t n_sites = 0, n_snps = 0;
  for (uint64_t i = 0; i < n; i++) {
    n_sites += ref[i] == 2 && ref[i + 1] == 3;
    n_snps += as_is_snp(core, emit, i, p) != 0;
  }
  uint64_t *site = malloc((n_sites ? n_sites : 1) * sizeof *site), *snp = malloc((n_snps ? n_snps : 1) * sizeof *snp);
  uint64_t *first = malloc((n_snps ? n_snps : 1) * sizeof *first), *off = malloc((n_snps + 1) * sizeof *off);
  bsc_asm_pair *all = NULL;
  int rc = BSC_OK;
  if (!site || !snp || !first || !off) {
    rc = bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
    goto done;
  }
  uint64_t ks = 0, kh = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (ref[i] == 2 && ref[i + 1] == 3) site[ks++] = i;
    if (as_is_snp(core, emit, i, p)) snp[kh++] = i;
  }
  /* WINDOW: the sites of SNP j are site[first[j] .. first[j] + (off[j + 1] - off[j])) */
  off[0] = 0;
  for (uint64_t j = 0; j < n_snps; j++) {
    const uint64_t h = snp[j], lo = h > W ? h - W : 0, hi = h + W < n - 1 ? h + W : n - 1;
    uint64_t a = 0, b;
    while (a < n_sites && site[a] < lo) a++;
    for (b = a; b < n_sites && site[b] <= hi; b++) {}
    first[j] = a;
    off[j + 1] = off[j] + (b - a);
  }
  const uint64_t total = off[n_snps];
  if (total > 0xffffffffull) {
    rc = bsc_set_error(BSC_ERR_RANGE, "%s: %llu records in one block, more than 2^32 - 1", who, (unsigned long long)total);
    goto done;
  }
  /* every record, whatever the room: the counts are the totals' source */
  all = calloc(total ? total : 1, sizeof *all);
  if (!all) {
    rc = bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
    goto done;
  }
  for (uint64_t j = 0; j < n_snps; j++)
    for (uint64_t k = off[j]; k < off[j + 1]; k++) {
      const uint64_t s = site[first[j] + (k - off[j])], h = snp[j];
      all[k].snp_pos = x + (uint32_t)h;
      all[k].cpg_pos = x + (uint32_t)s;
      all[k].info = core[h].gt | ((h == s || h == s + 1) ? BSC_ASM_OVERLAPPED << 8 : 0u);
    }
  uint64_t t[BSC_ASM_N_TOTALS] = {0};
  t[0] = n_snps;
  t[1] = total;
  for (uint32_t i = 0; i < nr; i++)
    for (uint64_t j = 0; j < n_snps; j++) {
      const int al = as_allele(&tpl[i], seq, seq_bytes, x, y, min_qual, x + (uint32_t)snp[j], core[snp[j]].gt);
      if (!al) continue;
      t[2]++;
      t[3] += al == 1;
      for (uint64_t k = off[j]; k < off[j + 1]; k++) {
        if ((all[k].info >> 8) & BSC_ASM_OVERLAPPED) continue;
        const int st = as_state(&tpl[i], seq, seq_bytes, x, y, min_qual, all[k].cpg_pos);
        if (st == AS_NONE) continue;
        uint32_t *w = &all[k].m1;
        w[2 * (al - 1) + (st - 1)]++;
        t[4]++;
      }
    }
  const uint64_t stored = total < cap ? total : cap;
  for (uint64_t k = 0; k < stored; k++) {
    as_finish(&all[k], lfact_256);
    t[5] += ((all[k].info >> 8) & BSC_ASM_DEEP) != 0;
  }
  if (stored) memcpy(pairs, all, (size_t)stored * sizeof *all);
  *n_pairs = total;
  if (totals) memcpy(totals, t, sizeof t);
done:
  free(site);
  free(snp);
  free(first);
  free(off);
  free(all);
  return rc;
}

static int as_line_written(const bsc_asm_pair *r, const bsc_asm_params *p) {
  const uint64_t c = p->min_cov > 1 ? p->min_cov : 1;
  return (r->info >> 8) == 0 && (uint64_t)r->m1 + r->u1 >= c && (uint64_t)r->m2 + r->u2 >= c;
}

long bsc_asm_format(const char *contig, const bsc_asm_pair *pairs, size_t n, const bsc_asm_params *p, char *buf, size_t cap, uint64_t totals2[2]) {
  if (!contig || !p || (n && !pairs) || (cap && !buf)) return bsc_set_error(BSC_ERR_ARG, "bsc_asm_format: NULL argument");
  const size_t cl = strlen(contig);
  if (cl < 1 || cl > 255 || strchr(contig, '\t') || strchr(contig, '\n'))
    return bsc_set_error(BSC_ERR_ARG, "bsc_asm_format: the contig's name must be 1 .. 255 bytes without tab or newline");
  char line[512];
  uint64_t bytes = 0, lines = 0;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) {
      const bsc_asm_pair *r = &pairs[i];
      if (!as_line_written(r, p)) continue;
      const unsigned gt = r->info & 0xffu;
      const int l = snprintf(line, sizeof line, "%s\t%u\t%llu\t%u\t%s\t%u\t%u\t%u\t%u\t%u\t%lld\n", contig, r->cpg_pos - 1u,
                             (unsigned long long)r->cpg_pos + 1ull, r->snp_pos, gt <= 9 ? as_gt_letters[gt] : "NN", r->m1, r->u1, r->m2, r->u2, r->aq,
                             (long long)r->cpg_pos - (long long)r->snp_pos);
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
