/*
 * variants_san.c — TEST ONLY: the host form of the variant-only call set (csrc/variants.c: bsc_variants_select_recs) as a stand-alone
 * program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: seeded random records in heap blocks of exactly their size, every
 * room from 0 to the need, NULL totals, the refusals, and the counters against sums formed here from the rule of include/bscall_amd.h.
 * `make variants-san`; tests/test_variants_host.py builds its own copy and runs it: "ok" and exit 0, or the case that failed.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bscall_amd.h>

static char errbuf[512];
int bsc_set_error(int code, const char *fmt, ...) { /* the library's own lives in bscall_api.c */
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, sizeof errbuf, fmt, ap);
  va_end(ap);
  return code;
}

static int failures;
#define CHECK(c, ...)                         \
  do {                                        \
    if (!(c)) {                               \
      failures++;                             \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                    \
      printf("\n");                           \
    }                                         \
  } while (0)

static uint64_t rng_state;
static uint32_t rnd(void) { /* splitmix64 */
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static void fill(bsc_vcf_rec *r, size_t n) {
  static const char alts[] = {0, 0, 'A', 'C', 'G', 'T', 'N', 'x'};
  uint8_t *b = (uint8_t *)r;
  for (size_t i = 0; i < n * sizeof *r; i++) b[i] = (uint8_t)rnd();
  for (size_t i = 0; i < n; i++) {
    r[i].core.emit = (uint8_t)((rnd() % 4u) ? 1 + (rnd() % 3u) * 127u : 0);
    r[i].core.alt[0] = alts[rnd() % sizeof alts];
    r[i].core.alt[1] = (rnd() % 4u) ? 0 : alts[2 + rnd() % 6u];
    r[i].core.gt = (uint8_t)(rnd() % 12u);
    r[i].core.ref_code = (uint8_t)(rnd() % 6u);
    r[i].core.flt = (uint8_t)((rnd() % 2u) ? 0 : rnd());
    r[i].rs_found = (uint8_t)((rnd() % 3u) ? 0 : 1 + rnd() % 3u);
  }
}

/* the rule, record by record, written here a second time */
static int rule(const bsc_vcf_rec *r, const bsc_var_params *p, uint64_t *t) {
  if (!r->core.emit || !r->core.alt[0]) return 0;
  if (r->core.phred < p->min_phred || (p->pass_only && r->core.flt) || (p->known_only && !r->rs_found)) return 0;
  const int snp = !r->core.alt[1];
  t[0]++;
  t[snp ? 1 : 2]++;
  t[3] += (0x16eu >> r->core.gt) & 1u && r->core.gt < 9;
  t[4] += !r->core.flt;
  t[5] += !!r->rs_found;
  t[6] += r->rs_found && !r->core.flt;
  if (snp && r->core.ref_code >= 1 && r->core.ref_code <= 4 && strchr("ACGT", r->core.alt[0])) {
    const int rp = r->core.ref_code == 1 || r->core.ref_code == 3, ap = r->core.alt[0] == 'A' || r->core.alt[0] == 'G';
    const int same = "NACGT"[r->core.ref_code] == r->core.alt[0];
    t[(rp == ap && !same) ? 7 : 8]++;
  }
  t[9] += r->core.phred;
  return 1;
}

int main(void) {
  rng_state = 20261020;
  static const size_t sizes[] = {0, 1, 2, 63, 64, 65, 1000, 4113};
  static const bsc_var_params pars[] = {{0, 0, 0, 0}, {100, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {60, 1, 1, 0}, {256, 0, 0, 0}};
  bsc_var_params d = {9, 9, 9, 9};
  bsc_var_params_default(&d);
  CHECK(!d.min_phred && !d.pass_only && !d.known_only && !d.reserved, "default");
  bsc_var_params_default(NULL);
  for (size_t s = 0; s < sizeof sizes / sizeof *sizes; s++) {
    const size_t n = sizes[s];
    bsc_vcf_rec *recs = malloc(n ? n * sizeof *recs : 1);
    fill(recs, n);
    for (size_t k = 0; k < sizeof pars / sizeof *pars; k++) {
      uint64_t want[10] = {0}, got[10], n_out = 77;
      bsc_vcf_rec *sel = malloc(n ? n * sizeof *sel : 1);
      size_t m = 0;
      for (size_t i = 0; i < n; i++)
        if (rule(&recs[i], &pars[k], want)) sel[m++] = recs[i];
      if (!k && n >= 1000) CHECK(m > n / 8 && want[1] && want[2] && want[3] && want[7] && want[8], "the draw gives every class");
      bsc_vcf_rec *out = malloc(m ? m * sizeof *out : 1); /* exactly the need: a record too many is a heap overflow */
      memset(got, 0xee, sizeof got);
      int rc = bsc_variants_select_recs(n ? recs : NULL, n, &pars[k], m ? out : NULL, m, &n_out, got);
      CHECK(rc == BSC_OK && n_out == m, "n %zu params %zu: rc %d, %llu records, want %zu", n, k, rc, (unsigned long long)n_out, m);
      CHECK(!memcmp(got, want, sizeof want), "n %zu params %zu: totals", n, k);
      CHECK(!m || !memcmp(out, sel, m * sizeof *out), "n %zu params %zu: records", n, k);
      rc = bsc_variants_select_recs(n ? recs : NULL, n, &pars[k], m ? out : NULL, m, &n_out, NULL);
      CHECK(rc == BSC_OK && n_out == m, "NULL totals");
      if (m) { /* one short: the need, the totals, nothing written */
        memset(out, 0x5a, m * sizeof *out);
        n_out = 0;
        rc = bsc_variants_select_recs(recs, n, &pars[k], out, m - 1, &n_out, got);
        CHECK(rc == BSC_ERR_ARG && n_out == m && !memcmp(got, want, sizeof want), "room one short: rc %d", rc);
        for (size_t i = 0; i < m * sizeof *out; i++)
          if (((uint8_t *)out)[i] != 0x5a) {
            CHECK(0, "room one short: byte %zu written", i);
            break;
          }
        rc = bsc_variants_select_recs(recs, n, &pars[k], NULL, 0, &n_out, NULL);
        CHECK(rc == BSC_ERR_ARG && n_out == m, "no room: rc %d", rc);
      }
      free(out);
      free(sel);
    }
    bsc_var_params bad = {0, 0, 0, 1};
    uint64_t n_out = 5;
    CHECK(bsc_variants_select_recs(recs, n, &bad, NULL, 0, &n_out, NULL) == BSC_ERR_ARG && n_out == 0 && strstr(errbuf, "reserved"), "reserved");
    CHECK(bsc_variants_select_recs(recs, n, NULL, NULL, 0, &n_out, NULL) == BSC_ERR_ARG, "NULL params");
    CHECK(bsc_variants_select_recs(recs, n, &pars[0], NULL, 0, NULL, NULL) == BSC_ERR_ARG, "NULL n_out");
    if (n) CHECK(bsc_variants_select_recs(NULL, n, &pars[0], NULL, 0, &n_out, NULL) == BSC_ERR_ARG, "NULL records");
    free(recs);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
