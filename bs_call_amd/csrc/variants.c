/*
 * variants.c — the host form of the variant-only call set (include/bscall_amd.h: VARIANT, PARAMS, SELECTED, TOTALS), over packed records:
 * the checker of the kernels of csrc/variantsdev.hip, written from the rule and from nothing else.  Host C alone.
 */
#include <stdint.h>
#include <string.h>

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

void bsc_var_params_default(bsc_var_params *p) {
  if (p) memset(p, 0, sizeof *p);
}

static int bsc_var_selected(const bsc_vcf_rec *r, const bsc_var_params *p) {
  if (r->core.emit == 0 || r->core.alt[0] == 0) return 0;
  if ((uint32_t)r->core.phred < p->min_phred) return 0;
  if (p->pass_only && r->core.flt != 0) return 0;
  if (p->known_only && r->rs_found == 0) return 0;
  return 1;
}

static void bsc_var_count(const bsc_vcf_rec *r, uint64_t *t) {
  const bsc_vcf_core *c = &r->core;
  t[0]++;
  t[c->alt[1] == 0 ? 1 : 2]++;
  if (c->gt == 1 || c->gt == 2 || c->gt == 3 || c->gt == 5 || c->gt == 6 || c->gt == 8) t[3]++;
  if (c->flt == 0) t[4]++;
  if (r->rs_found != 0) t[5]++;
  if (r->rs_found != 0 && c->flt == 0) t[6]++;
  const char a = c->alt[0];
  if (c->alt[1] == 0 && c->ref_code >= 1 && c->ref_code <= 4 && (a == 'A' || a == 'C' || a == 'G' || a == 'T')) {
    const char ref = "NACGT"[c->ref_code];
    const int ts = (ref == 'A' && a == 'G') || (ref == 'G' && a == 'A') || (ref == 'C' && a == 'T') || (ref == 'T' && a == 'C');
    t[ts ? 7 : 8]++;
  }
  t[9] += c->phred;
}

int bsc_variants_select_recs(const bsc_vcf_rec *recs, size_t n, const bsc_var_params *p, bsc_vcf_rec *out, uint64_t cap, uint64_t *n_out,
                             uint64_t totals[10]) {
  if (!p || !n_out || (n && !recs) || (cap && !out)) return bsc_set_error(BSC_ERR_ARG, "bsc_variants_select_recs: NULL argument");
  *n_out = 0;
  if (p->reserved != 0) return bsc_set_error(BSC_ERR_ARG, "bsc_variants_select_recs: reserved is %u, not 0", p->reserved);
  uint64_t t[BSC_VAR_N_TOTALS] = {0};
  for (size_t i = 0; i < n; i++)
    if (bsc_var_selected(&recs[i], p)) bsc_var_count(&recs[i], t);
  *n_out = t[0];
  if (totals) memcpy(totals, t, sizeof t);
  if (t[0] > cap)
    return bsc_set_error(BSC_ERR_ARG, "bsc_variants_select_recs: %llu records selected, cap is %llu", (unsigned long long)t[0], (unsigned long long)cap);
  uint64_t k = 0;
  for (size_t i = 0; i < n; i++)
    if (bsc_var_selected(&recs[i], p)) memcpy(&out[k++], &recs[i], sizeof recs[i]);
  return BSC_OK;
}
