/*
 * methbed.c — host-side rendering of one record as a bedMethyl line: the methylation level of one cytosine, from the counts and
 * the call the record carries.  The reference defines the sites and the counts for its report's CpG_ref_meth / CpG_nonref_meth
 * histograms only (src/print_vcf.c:442-515): a homozygous CC (strand +) or GG (strand -) call in a CpG, a = the non-converted
 * and b = the converted count of that strand (counts[5], counts[7] / counts[6], counts[4], :450-451, :472-473), `if(a + b)`.
 * This file restates that rule per record and writes the line; include/bscall_amd.h has the columns.
 *
 * This is the CHECKER of the device's encoder (csrc/methdev.hip): the device writes, for any 128 bytes of record, exactly the
 * line this file writes — change one and the other has to follow; tests/test_gpu_methbed.py compares them.  Plain C over the
 * C library's formatter, nothing shared with the device code.
 */
#include <stdio.h>
#include <string.h>

#include "../../include/bscall_amd.h"

static const char *const METH_RGB[11] = {"0,255,0",   "55,255,0",  "105,255,0", "155,255,0", "205,255,0", "255,255,0",
                                         "255,205,0", "255,155,0", "255,105,0", "255,55,0",  "255,0,0"};

void bsc_meth_params_default(bsc_meth_params *p) {
  if (!p) return;
  p->contexts = BSC_METH_CPG;
  p->min_cov = 1;
  p->min_phred = 0;
  p->pass_only = 0;
}

static const char *meth_label(const bsc_vcf_core *c, int minus) {
  if (c->cg == 'C') return "CG";
  const char n2 = minus ? c->cx_gt[0] : c->cx_gt[4]; /* the called second neighbour, in the cytosine's own direction */
  if (n2 == (minus ? 'C' : 'G')) return "CHG";
  if (n2 == 'A' || n2 == 'C' || n2 == 'G' || n2 == 'T') return "CHH";
  return "CHN";
}

long bsc_meth_format_rec(const bsc_vcf_rec *r, const char *contig, const bsc_meth_params *p, char *buf, size_t cap) {
  if (!r || !contig || !p || (!buf && cap)) return -1;
  if (p->contexts != BSC_METH_CPG && p->contexts != BSC_METH_ALL) return -1;
  const size_t cl = strnlen(contig, 256);
  if (cl == 0 || cl > 255 || memchr(contig, '\t', cl) || memchr(contig, '\n', cl)) return -1;
  const bsc_vcf_core *c = &r->core;
  if (!c->emit || (c->gt != 4 && c->gt != 7)) return 0;
  if (c->cg != 'C' && !(p->contexts == BSC_METH_ALL && c->cg == 'H')) return 0;
  const int minus = c->gt == 7;
  const uint64_t a = minus ? r->counts[6] : r->counts[5], b = minus ? r->counts[4] : r->counts[7], cov = a + b;
  if (cov < (p->min_cov > 1 ? p->min_cov : 1)) return 0;
  if (c->phred < p->min_phred) return 0;
  if (p->pass_only && c->flt) return 0;
  const uint64_t pct = (200 * a + cov) / (2 * cov);
  const uint32_t start = c->pos - 1u; /* (a record with pos = 0, which the chain never writes: modulo 2^32, as the device) */
  char line[512]; /* the contig's name + 111 at most */
  const int n = snprintf(line, sizeof line, "%s\t%llu\t%llu\t%s\t%llu\t%c\t%llu\t%llu\t%s\t%llu\t%llu\t%llu\t%llu\t%u\t%s\n", contig,
                         (unsigned long long)start, (unsigned long long)c->pos, meth_label(c, minus), (unsigned long long)(cov < 1000 ? cov : 1000),
                         minus ? '-' : '+', (unsigned long long)start, (unsigned long long)c->pos, METH_RGB[pct / 10], (unsigned long long)cov,
                         (unsigned long long)pct, (unsigned long long)a, (unsigned long long)b, (unsigned)c->phred,
                         c->flt == 0 ? "PASS" : ((c->flt & 128) ? "mac1" : "fail"));
  if (n < 0 || (size_t)n >= sizeof line) return -1;
  if ((size_t)n <= cap) memcpy(buf, line, (size_t)n);
  return n;
}
