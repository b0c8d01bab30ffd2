/*
 * epi_san.c — TEST ONLY: the host form of the epiallele table (csrc/epi.c: bsc_epi_windows_host, bsc_epi_format) as a stand-alone program
 * under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: seeded random templates, read bytes and reference codes in heap blocks of
 * exactly their size, every room of the records from 0 to the need, NULL totals, the formatter's rooms, the refusals, and the sums of the
 * records against the totals.
 * `make epi-san`; tests/test_epi_host.py builds its own copy and runs it: "ok" and exit 0, or the case that failed.
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

int main(void) {
  rng_state = 20261021;
  bsc_epi_params d = {9, 9};
  bsc_epi_params_default(&d);
  CHECK(d.min_cov == 10 && d.reserved == 0, "default");
  bsc_epi_params_default(NULL);
  static const uint32_t lens[] = {1, 2, 7, 8, 63, 64, 65, 300, 5000};
  static const uint32_t nrs[] = {0, 1, 7, 200};
  uint64_t seen = 0;
  for (size_t s = 0; s < sizeof lens / sizeof *lens; s++)
    for (size_t r = 0; r < sizeof nrs / sizeof *nrs; r++) {
      const uint32_t n = lens[s], nr = nrs[r], x = 1 + rnd() % 1000u, y = x + n - 1;
      uint8_t *ref = malloc((size_t)n + 2); /* x .. y + 2, and not a byte more */
      for (uint32_t i = 0; i < n + 2; i++) ref[i] = (uint8_t)((rnd() % 3u) ? 2 + (i & 1u) : rnd() % 5u); /* many CG */
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
      for (uint64_t i = 0; i < seq_bytes; i++) seq[i] = (uint8_t)((rnd() & 3u) | ((rnd() % 8u) ? 30u + rnd() % 10u : rnd() % 64u) << 2);
      if (nr > 2) tpl[nr - 1].off[0] = seq_bytes; /* a read outside the buffer is absent, never read */
      for (uint32_t mc = 0; mc <= 4; mc += 2) {
        const bsc_epi_params par = {mc, 0};
        uint64_t need = 77, tot[8], n2;
        memset(tot, 0xee, sizeof tot);
        int rc = bsc_epi_windows_host(nr ? tpl : NULL, nr, seq, seq_bytes, x, y, ref, 20, &par, NULL, 0, &need, tot);
        CHECK(rc == BSC_OK && tot[0] == need && tot[5] == 0 && tot[6] == 0 && tot[7] == 0, "len %u nr %u: count rc %d", n, nr, rc);
        bsc_epi_window *out = malloc(need ? need * sizeof *out : 1); /* exactly the need */
        rc = bsc_epi_windows_host(nr ? tpl : NULL, nr, seq, seq_bytes, x, y, ref, 20, &par, need ? out : NULL, need, &n2, NULL);
        CHECK(rc == BSC_OK && n2 == need, "len %u nr %u: exact room rc %d", n, nr, rc);
        uint64_t sc = 0, sb = 0, sites = 0;
        for (uint32_t i = 0; i < n; i++) sites += ref[i] == 2 && ref[i + 1] == 3;
        CHECK(need == (sites >= 4 ? sites - 3 : 0), "len %u: %llu sites, %llu windows", n, (unsigned long long)sites, (unsigned long long)need);
        for (uint64_t i = 0; i < need; i++) {
          for (unsigned c = 0; c < 16; c++) {
            sc += out[i].c[c];
            sb += (uint64_t)out[i].c[c] * (unsigned)__builtin_popcount(c);
          }
          CHECK(out[i].pos >= x && out[i].pos <= y && ref[out[i].pos - x] == 2 && ref[out[i].pos - x + 1] == 3, "a window that starts at no site");
          const uint64_t e = (uint64_t)out[i].pos + out[i].span;
          CHECK(out[i].span >= 6 && e <= y && ref[e - x] == 2 && ref[e - x + 1] == 3, "a window that ends at no site");
          CHECK(i + 1 >= need || out[i + 1].pos > out[i].pos, "order");
        }
        seen += sc;
        CHECK(sc == tot[1] && sb == tot[3] && tot[2] <= tot[4] && tot[4] <= nr && tot[2] <= tot[1], "totals");
        if (need > 1) { /* one short: counted, not stored */
          bsc_epi_window *part = malloc((need - 1) * sizeof *part);
          rc = bsc_epi_windows_host(nr ? tpl : NULL, nr, seq, seq_bytes, x, y, ref, 20, &par, part, need - 1, &n2, NULL);
          CHECK(rc == BSC_OK && n2 == need && !memcmp(part, out, (need - 1) * sizeof *part), "room one short");
          free(part);
        }
        /* the formatter: the need, the exact room, one short */
        uint64_t t2[2] = {0, 0};
        const long len = bsc_epi_format("chr1", need ? out : NULL, need, &par, NULL, 0, t2);
        CHECK(len >= 0 && (uint64_t)len == t2[0], "format: the need");
        char *buf = malloc(len ? (size_t)len : 1);
        CHECK(bsc_epi_format("chr1", need ? out : NULL, need, &par, buf, (size_t)len, NULL) == len, "format: exact room");
        uint64_t nl = 0;
        for (long i = 0; i < len; i++) nl += buf[i] == '\n';
        CHECK(nl == t2[1] && (!len || buf[len - 1] == '\n'), "format: lines");
        if (len) {
          memset(buf, 0x5a, (size_t)len);
          CHECK(bsc_epi_format("chr1", out, need, &par, buf, (size_t)len - 1, NULL) == len && buf[0] == 0x5a && buf[len - 2] == 0x5a, "format: one short");
        }
        free(buf);
        free(out);
      }
      const bsc_epi_params bad = {1, 1}, ok = {1, 0};
      uint64_t n_out = 5;
      CHECK(bsc_epi_windows_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, &bad, NULL, 0, &n_out, NULL) == BSC_ERR_ARG && n_out == 0 && strstr(errbuf, "reserved"),
            "reserved 1");
      CHECK(bsc_epi_windows_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, NULL, NULL, 0, &n_out, NULL) == BSC_ERR_ARG, "NULL params");
      CHECK(bsc_epi_windows_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, &ok, NULL, 0, NULL, NULL) == BSC_ERR_ARG, "NULL n_win");
      CHECK(bsc_epi_windows_host(tpl, nr, seq, seq_bytes, y + 1, y, ref, 20, &ok, NULL, 0, &n_out, NULL) == BSC_ERR_ARG, "y < x");
      free(seq);
      free(tpl);
      free(ref);
    }
  CHECK(seen > 1000, "the random blocks gave %llu patterns", (unsigned long long)seen);
  const bsc_epi_params ok = {1, 0}, bad = {1, 7};
  char name[300];
  memset(name, 'c', sizeof name);
  name[256] = 0;
  CHECK(bsc_epi_format(name, NULL, 0, &ok, NULL, 0, NULL) < 0, "a name of 256 bytes");
  name[255] = 0;
  CHECK(bsc_epi_format(name, NULL, 0, &ok, NULL, 0, NULL) == 0, "a name of 255 bytes");
  CHECK(bsc_epi_format("", NULL, 0, &ok, NULL, 0, NULL) < 0, "an empty name");
  CHECK(bsc_epi_format("a\tb", NULL, 0, &ok, NULL, 0, NULL) < 0, "a tab in the name");
  CHECK(bsc_epi_format("a\nb", NULL, 0, &ok, NULL, 0, NULL) < 0, "a newline in the name");
  CHECK(bsc_epi_format("chr1", NULL, 0, &bad, NULL, 0, NULL) < 0, "reserved 7");
  { /* the longest line: ten digits everywhere, eleven in n */
    bsc_epi_window big;
    big.pos = 0xffffffffu - 7u;
    big.span = 6;
    for (int c = 0; c < 16; c++) big.c[c] = 0xffffffffu;
    const long len = bsc_epi_format(name, &big, 1, &ok, NULL, 0, NULL);
    CHECK(len == 255 + 214, "the longest line has %ld bytes", len);
    char *buf = malloc((size_t)len);
    CHECK(bsc_epi_format(name, &big, 1, &ok, buf, (size_t)len, NULL) == len && !memcmp(buf + 255, "\t4294967287\t4294967295\t68719476720\t16\t4294967295\t", 48),
          "its columns");
    free(buf);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
