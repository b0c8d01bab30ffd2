/*
 * asm_san.c — TEST ONLY: the host form of the allele-specific methylation table (csrc/asm.c: bsc_asm_pairs_host, bsc_asm_format,
 * bsc_asm_fisher_p) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: seeded random templates, read
 * bytes, reference codes, dense records and emit bytes in heap blocks of exactly their size, rooms of the records from 0 to the need, NULL
 * totals and NULL emit bytes, the formatter's rooms, Fisher's test at the limits of its `int` products, the refusals, and the sums of the
 * records against the totals.
 * `make asm-san`; tests/test_asm_host.py builds its own copy and runs it: "ok" and exit 0, or the case that failed.
 */
#include <math.h>
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

int main(void) {
  rng_state = 20261020;
  double lf[256];
  lf[0] = lf[1] = 0.0;
  for (int i = 2; i < 256; i++) lf[i] = lf[i - 1] + log((double)i);
  bsc_asm_params d = {9, 9, 9, 9};
  bsc_asm_params_default(&d);
  CHECK(d.min_phred == 20 && d.pass_only == 0 && d.max_dist == 500 && d.min_cov == 2, "default");
  bsc_asm_params_default(NULL);
  static const uint8_t het[6] = {1, 2, 3, 5, 6, 8};
  static const uint32_t lens[] = {1, 2, 63, 64, 65, 300, 3000};
  static const uint32_t nrs[] = {0, 1, 7, 200};
  static const uint32_t dists[] = {1, 7, 500, 65535};
  for (size_t s = 0; s < sizeof lens / sizeof *lens; s++)
    for (size_t r = 0; r < sizeof nrs / sizeof *nrs; r++) {
      const uint32_t n = lens[s], nr = nrs[r], x = 1 + rnd() % 1000u, y = x + n - 1;
      uint8_t *ref = malloc((size_t)n + 2); /* x .. y + 2, and not a byte more */
      for (uint32_t i = 0; i < n + 2; i++) ref[i] = (uint8_t)((rnd() % 3u) ? 2 + (i & 1u) : rnd() % 5u); /* many CG */
      bsc_vcf_core *core = calloc(n, sizeof *core);
      uint8_t *emit = malloc(n);
      for (uint32_t i = 0; i < n; i++) {
        emit[i] = (uint8_t)(rnd() % 8u != 0);
        if (rnd() % 6u) continue;
        core[i].pos = x + i;
        core[i].emit = (uint8_t)(rnd() % 8u != 0);
        core[i].gt = (rnd() % 8u) ? het[rnd() % 6u] : (uint8_t)(rnd() % 256u);
        core[i].phred = (uint8_t)(rnd() % 60u);
        core[i].flt = (rnd() % 4u) ? 0 : (uint8_t)(1u << (rnd() % 4u));
      }
      bsc_template *tpl = malloc(nr ? nr * sizeof *tpl : 1);
      uint64_t seq_bytes = 0;
      for (uint32_t i = 0; i < nr; i++) {
        memset(&tpl[i], 0, sizeof tpl[i]);
        tpl[i].bs_strand = (uint8_t)(rnd() % 4u);
        for (int k = 0; k < 2; k++) {
          if (rnd() % 5u == 0) continue; /* absent */
          tpl[i].len[k] = 1 + rnd() % 150u;
          tpl[i].pos[k] = x + rnd() % (n + 20u); /* some reach past y, some start behind it */
          tpl[i].off[k] = seq_bytes;
          seq_bytes += tpl[i].len[k];
        }
      }
      uint8_t *seq = malloc(seq_bytes ? seq_bytes : 1);
      for (uint64_t i = 0; i < seq_bytes; i++) seq[i] = (uint8_t)((rnd() & 3u) | ((rnd() % 4u) ? 30u + rnd() % 10u : rnd() % 64u) << 2);
      if (nr > 2) tpl[2].off[0] = seq_bytes + 5; /* a read outside the buffer: absent */
      bsc_asm_params p = {rnd() % 30u, (int32_t)(rnd() & 1u), dists[(s + r) % 4u], rnd() % 3u};
      uint64_t need = 0, tot[8], tot2[8];
      int rc = bsc_asm_pairs_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, core, (r & 1u) ? emit : NULL, lf, &p, NULL, 0, &need, tot);
      CHECK(rc == BSC_OK && tot[1] == need && tot[5] == 0 && tot[6] == 0 && tot[7] == 0 && tot[3] <= tot[2], "count n %u nr %u: %s", n, nr, errbuf);
      const uint64_t rooms[] = {need, need ? need - 1 : 0, need / 2, need + 3};
      bsc_asm_pair *full = NULL;
      for (int k = 0; k < 4; k++) {
        const uint64_t room = rooms[k];
        bsc_asm_pair *out = malloc(room ? room * sizeof *out : 1); /* exactly the room */
        uint64_t got = 0;
        rc = bsc_asm_pairs_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, core, (r & 1u) ? emit : NULL, lf, &p, out, room, &got, k == 1 ? NULL : tot2);
        CHECK(rc == BSC_OK && got == need, "room %llu of %llu", (unsigned long long)room, (unsigned long long)need);
        if (k != 1) CHECK(!memcmp(tot, tot2, 5 * sizeof *tot), "the totals depend on the room");
        if (k == 0) {
          full = out;
          uint64_t sum = 0, deep = 0;
          for (uint64_t i = 0; i < need; i++) {
            sum += (uint64_t)out[i].m1 + out[i].u1 + out[i].m2 + out[i].u2;
            deep += ((out[i].info >> 8) & BSC_ASM_DEEP) != 0;
            CHECK(out[i].snp_pos >= x && out[i].snp_pos <= y && out[i].cpg_pos >= x && out[i].cpg_pos <= y && out[i].aq <= 1000, "record %llu", (unsigned long long)i);
            const int64_t dd = (int64_t)out[i].cpg_pos - (int64_t)out[i].snp_pos;
            CHECK(dd >= -(int64_t)p.max_dist && dd <= (int64_t)p.max_dist, "record %llu outside the window", (unsigned long long)i);
            if ((out[i].info >> 8) & BSC_ASM_OVERLAPPED) CHECK((dd == 0 || dd == -1) && out[i].m1 + out[i].u1 + out[i].m2 + out[i].u2 + out[i].aq == 0, "overlapped");
            if (i) CHECK(out[i - 1].snp_pos < out[i].snp_pos || (out[i - 1].snp_pos == out[i].snp_pos && out[i - 1].cpg_pos < out[i].cpg_pos), "order");
          }
          CHECK(sum == tot[4] && deep == tot2[5], "sums");
        } else {
          CHECK(!memcmp(out, full, (size_t)(room < need ? room : need) * sizeof *out), "the records depend on the room");
          free(out);
        }
      }
      /* the formatter: the need, then exactly the need, then one short */
      uint64_t t2[2];
      const long len = bsc_asm_format("chr1", full, (size_t)need, &p, NULL, 0, t2);
      CHECK(len >= 0 && (uint64_t)len == t2[0], "format need");
      char *buf = malloc(len ? (size_t)len : 1);
      CHECK(bsc_asm_format("chr1", full, (size_t)need, &p, buf, (size_t)len, NULL) == len, "format exact");
      uint64_t nl = 0;
      for (long i = 0; i < len; i++) nl += buf[i] == '\n';
      CHECK(nl == t2[1], "lines");
      if (len) {
        char *small = malloc((size_t)len - 1 ? (size_t)len - 1 : 1);
        CHECK(bsc_asm_format("chr1", full, (size_t)need, &p, small, (size_t)len - 1, NULL) == len, "format one short");
        free(small);
      }
      free(buf);
      free(full);
      free(seq);
      free(tpl);
      free(emit);
      free(core);
      free(ref);
    }
  /* Fisher's test: the limits of the `int` products, the clamp, the empty table */
  {
    const int32_t t0[4] = {0, 0, 0, 0}, t1[4] = {20000, 0, 0, 20000}, t2[4] = {23170, 0, 0, 23170}, t3[4] = {11585, 11585, 11585, 11585}, t4[4] = {46340, 0, 0, 0},
                  t5[4] = {0, 23170, 23170, 0};
    const int32_t neg[4] = {0, -1, 0, 0}, deep[4] = {46340, 1, 0, 0}, wrap[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    CHECK(bsc_asm_fisher_p(neg, lf) == -1.0 && bsc_asm_fisher_p(deep, lf) == -1.0 && bsc_asm_fisher_p(wrap, lf) == -1.0 && bsc_asm_fisher_p(NULL, lf) == -1.0 &&
              bsc_asm_fisher_p(t0, NULL) == -1.0,
          "tables outside the range");
    CHECK(bsc_asm_fisher_p(t0, lf) == 1.0, "empty table");
    CHECK(bsc_asm_fisher_p(t1, lf) < 1e-100 && bsc_asm_fisher_p(t2, lf) < 1e-100 && bsc_asm_fisher_p(t5, lf) < 1e-100, "extreme tables");
    const double p3 = bsc_asm_fisher_p(t3, lf), p4 = bsc_asm_fisher_p(t4, lf);
    CHECK(p3 > 0.99 && p3 < 1.01 && p4 > 0.99 && p4 < 1.01, "p = 1 tables: %g %g", p3, p4);
  }
  /* the refusals */
  {
    uint8_t ref[3] = {2, 3, 1};
    bsc_vcf_core core[1];
    memset(core, 0, sizeof core);
    bsc_asm_pair out[1];
    uint64_t n = 7;
    bsc_asm_params p;
    bsc_asm_params_default(&p);
    CHECK(bsc_asm_pairs_host(NULL, 0, NULL, 0, 5, 5, ref, 20, core, NULL, lf, &p, out, 1, &n, NULL) == BSC_OK && n == 0, "a block of one position");
    CHECK(bsc_asm_pairs_host(NULL, 0, NULL, 0, 5, 4, ref, 20, core, NULL, lf, &p, out, 1, &n, NULL) == BSC_ERR_ARG, "y < x");
    CHECK(bsc_asm_pairs_host(NULL, 1, NULL, 0, 5, 5, ref, 20, core, NULL, lf, &p, out, 1, &n, NULL) == BSC_ERR_ARG, "NULL templates");
    CHECK(bsc_asm_pairs_host(NULL, 0, NULL, 0, 5, 5, ref, 20, NULL, NULL, lf, &p, out, 1, &n, NULL) == BSC_ERR_ARG, "NULL records");
    CHECK(bsc_asm_pairs_host(NULL, 0, NULL, 0, 5, 5, ref, 20, core, NULL, NULL, &p, out, 1, &n, NULL) == BSC_ERR_ARG, "NULL table");
    p.max_dist = 0;
    CHECK(bsc_asm_pairs_host(NULL, 0, NULL, 0, 5, 5, ref, 20, core, NULL, lf, &p, out, 1, &n, NULL) == BSC_ERR_ARG, "max_dist 0");
    p.max_dist = 65536;
    CHECK(bsc_asm_pairs_host(NULL, 0, NULL, 0, 5, 5, ref, 20, core, NULL, lf, &p, out, 1, &n, NULL) == BSC_ERR_ARG, "max_dist 65536");
    p.max_dist = 500;
    char name[300];
    memset(name, 'x', sizeof name);
    name[256] = 0;
    CHECK(bsc_asm_format(name, out, 0, &p, NULL, 0, NULL) == BSC_ERR_ARG && bsc_asm_format("", out, 0, &p, NULL, 0, NULL) == BSC_ERR_ARG &&
              bsc_asm_format("a\tb", out, 0, &p, NULL, 0, NULL) == BSC_ERR_ARG && bsc_asm_format(NULL, out, 0, &p, NULL, 0, NULL) == BSC_ERR_ARG,
          "contig names");
    /* the longest line: 255 + 104 bytes */
    name[255] = 0;
    const bsc_asm_pair big = {0xffffffffu, 1000000001u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 3u};
    char line[400];
    const long l = bsc_asm_format(name, &big, 1, &p, line, sizeof line, NULL);
    CHECK(l == 255 + 104, "the longest line has %ld bytes", l);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
