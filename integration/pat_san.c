/*
 * pat_san.c — TEST ONLY: the host form of the per-read CpG pattern table (csrc/pat.c: bsc_pat_recs_host, bsc_pat_format, bsc_pat_count_sites) as
 * a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: seeded random templates, read bytes and reference
 * codes in heap blocks of exactly their size, every room of the records from 0 to the need, NULL totals, the formatter's rooms, the site count
 * in two halves, the refusals, and the sums of the records against the totals.
 * `make pat-san`; tests/test_pat_host.py builds its own copy and runs it: "ok" and exit 0, or the case that failed.
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

/* the sites, C's, T's and dots of a record's pattern */
static unsigned pattern(const bsc_pat_rec *r, unsigned *c, unsigned *t, unsigned *dot, unsigned *first, unsigned *last) {
  unsigned n = 0;
  *c = *t = *dot = *first = *last = 0;
  for (; n < BSC_PAT_MAX_SITES; n++) {
    const unsigned code = (unsigned)((n < 32 ? r->hi >> (62 - 2 * n) : r->lo >> (62 - 2 * (n - 32))) & 3u);
    if (!code) break;
    *c += code == 2;
    *t += code == 3;
    *dot += code == 1;
    if (!n) *first = code;
    *last = code;
  }
  for (unsigned k = n; k < BSC_PAT_MAX_SITES; k++) /* nothing behind the last site */
    if ((k < 32 ? r->hi >> (62 - 2 * k) : r->lo >> (62 - 2 * (k - 32))) & 3u) return 0;
  return n;
}

int main(void) {
  rng_state = 20261021;
  bsc_pat_params d = {9, 9};
  bsc_pat_params_default(&d);
  CHECK(d.min_sites == 1 && d.reserved == 0, "default");
  bsc_pat_params_default(NULL);
  static const uint32_t lens[] = {1, 2, 7, 8, 63, 64, 65, 300, 5000};
  static const uint32_t nrs[] = {0, 1, 7, 200};
  uint64_t seen = 0, seen_cut = 0;
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
          tpl[i].len[k] = 1 + rnd() % (i % 9u == 8u ? 1500u : 150u); /* some span more than 64 sites */
          tpl[i].pos[k] = x + rnd() % (n + 20u); /* some reach past y, some start behind it */
          tpl[i].off[k] = seq_bytes;
          seq_bytes += tpl[i].len[k];
        }
      }
      uint8_t *seq = malloc(seq_bytes ? seq_bytes : 1);
      for (uint64_t i = 0; i < seq_bytes; i++) seq[i] = (uint8_t)((rnd() & 3u) | ((rnd() % 8u) ? 30u + rnd() % 10u : rnd() % 64u) << 2);
      if (nr > 2) tpl[nr - 1].off[0] = seq_bytes; /* a read outside the buffer is absent, never read */
      for (uint32_t ms = 0; ms <= 4; ms += 2) {
        const bsc_pat_params par = {ms, 0};
        uint64_t need = 77, tot[8], n2;
        memset(tot, 0xee, sizeof tot);
        int rc = bsc_pat_recs_host(nr ? tpl : NULL, nr, seq, seq_bytes, x, y, ref, 20, &par, NULL, 0, &need, tot);
        CHECK(rc == BSC_OK && tot[0] == need && tot[1] >= need && tot[2] <= nr && tot[2] <= tot[1] && tot[6] <= tot[2], "len %u nr %u: count rc %d", n, nr, rc);
        bsc_pat_rec *out = malloc(need ? need * sizeof *out : 1); /* exactly the need */
        rc = bsc_pat_recs_host(nr ? tpl : NULL, nr, seq, seq_bytes, x, y, ref, 20, &par, need ? out : NULL, need, &n2, NULL);
        CHECK(rc == BSC_OK && n2 == need, "len %u nr %u: exact room rc %d", n, nr, rc);
        uint64_t sites = 0, sn = 0, sc = 0, st = 0, sd = 0;
        for (uint32_t i = 0; i < n; i++) sites += ref[i] == 2 && ref[i + 1] == 3;
        CHECK(tot[7] == sites, "len %u: %llu sites, totals say %llu", n, (unsigned long long)sites, (unsigned long long)tot[7]);
        for (uint64_t i = 0; i < need; i++) {
          unsigned c, t, dot, first, last;
          const unsigned len = pattern(&out[i], &c, &t, &dot, &first, &last);
          CHECK(len >= 1 && first >= 2 && last >= 2 && out[i].count >= 1 && (uint64_t)out[i].idx + len <= sites, "record %llu", (unsigned long long)i);
          sn += out[i].count;
          sc += (uint64_t)c * out[i].count;
          st += (uint64_t)t * out[i].count;
          sd += (uint64_t)dot * out[i].count;
          if (i + 1 < need) {
            const bsc_pat_rec *a = &out[i], *b = &out[i + 1];
            CHECK(a->idx < b->idx || (a->idx == b->idx && (a->hi < b->hi || (a->hi == b->hi && a->lo < b->lo))), "order at %llu", (unsigned long long)i);
          }
        }
        seen += sn;
        seen_cut += tot[6];
        CHECK(sn == tot[1] && sc == tot[3] && st == tot[4] && sd == tot[5], "totals");
        if (need > 1) { /* one short: counted, not stored */
          bsc_pat_rec *part = malloc((need - 1) * sizeof *part);
          rc = bsc_pat_recs_host(nr ? tpl : NULL, nr, seq, seq_bytes, x, y, ref, 20, &par, part, need - 1, &n2, NULL);
          CHECK(rc == BSC_OK && n2 == need && !memcmp(part, out, (need - 1) * sizeof *part), "room one short");
          free(part);
        }
        /* the formatter: the need, the exact room, one short */
        uint64_t t2[2] = {0, 0};
        const long len = bsc_pat_format("chr1", 12345, need ? out : NULL, need, &par, NULL, 0, t2);
        CHECK(len >= 0 && (uint64_t)len == t2[0] && t2[1] == need, "format: the need");
        char *buf = malloc(len ? (size_t)len : 1);
        CHECK(bsc_pat_format("chr1", 12345, need ? out : NULL, need, &par, buf, (size_t)len, NULL) == len, "format: exact room");
        uint64_t nl = 0;
        for (long i = 0; i < len; i++) nl += buf[i] == '\n';
        CHECK(nl == t2[1] && (!len || buf[len - 1] == '\n'), "format: lines");
        if (len) {
          memset(buf, 0x5a, (size_t)len);
          CHECK(bsc_pat_format("chr1", 12345, out, need, &par, buf, (size_t)len - 1, NULL) == len && buf[0] == 0x5a && buf[len - 2] == 0x5a, "format: one short");
        }
        free(buf);
        free(out);
      }
      /* the site count over the same codes read as a contig of n + 2 bases: two halves are the whole, the last base is no site */
      {
        uint64_t whole = 9, a = 9, b = 9;
        const uint64_t cl = (uint64_t)n + 2, mid = 1 + rnd() % cl;
        CHECK(bsc_pat_count_sites(ref, cl, 1, cl + 1, &whole) == BSC_OK && bsc_pat_count_sites(ref, cl, 1, mid, &a) == BSC_OK &&
                  bsc_pat_count_sites(ref, cl, mid, cl + 50, &b) == BSC_OK && a + b == whole,
              "count_sites: halves");
        uint64_t want = 0;
        for (uint64_t i = 0; i + 1 < cl; i++) want += ref[i] == 2 && ref[i + 1] == 3;
        CHECK(whole == want, "count_sites: %llu, not %llu", (unsigned long long)whole, (unsigned long long)want);
        CHECK(bsc_pat_count_sites(ref, cl, cl, cl + 1, &a) == BSC_OK && a == 0, "count_sites: the last base");
        CHECK(bsc_pat_count_sites(ref, cl, 0, 5, &a) == BSC_ERR_ARG && a == 0, "count_sites: position 0");
        CHECK(bsc_pat_count_sites(ref, cl, 1, 5, NULL) == BSC_ERR_ARG, "count_sites: NULL");
        CHECK(bsc_pat_count_sites(ref, cl, 5, 3, &a) == BSC_OK && a == 0, "count_sites: an empty stretch");
      }
      const bsc_pat_params bad = {1, 1}, ok = {1, 0};
      uint64_t n_out = 5;
      CHECK(bsc_pat_recs_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, &bad, NULL, 0, &n_out, NULL) == BSC_ERR_ARG && n_out == 0 && strstr(errbuf, "reserved"),
            "reserved 1");
      CHECK(bsc_pat_recs_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, NULL, NULL, 0, &n_out, NULL) == BSC_ERR_ARG, "NULL params");
      CHECK(bsc_pat_recs_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, &ok, NULL, 0, NULL, NULL) == BSC_ERR_ARG, "NULL n_rec");
      CHECK(bsc_pat_recs_host(tpl, nr, seq, seq_bytes, y + 1, y, ref, 20, &ok, NULL, 0, &n_out, NULL) == BSC_ERR_ARG, "y < x");
      free(seq);
      free(tpl);
      free(ref);
    }
  CHECK(seen > 1000 && seen_cut > 0, "the random blocks gave %llu pieces, %llu templates cut", (unsigned long long)seen, (unsigned long long)seen_cut);
  const bsc_pat_params ok = {1, 0}, bad = {1, 7};
  char name[300];
  memset(name, 'c', sizeof name);
  name[256] = 0;
  CHECK(bsc_pat_format(name, 0, NULL, 0, &ok, NULL, 0, NULL) < 0, "a name of 256 bytes");
  name[255] = 0;
  CHECK(bsc_pat_format(name, 0, NULL, 0, &ok, NULL, 0, NULL) == 0, "a name of 255 bytes");
  CHECK(bsc_pat_format("", 0, NULL, 0, &ok, NULL, 0, NULL) < 0, "an empty name");
  CHECK(bsc_pat_format("a\tb", 0, NULL, 0, &ok, NULL, 0, NULL) < 0, "a tab in the name");
  CHECK(bsc_pat_format("a\nb", 0, NULL, 0, &ok, NULL, 0, NULL) < 0, "a newline in the name");
  CHECK(bsc_pat_format("chr1", 0, NULL, 0, &bad, NULL, 0, NULL) < 0, "reserved 7");
  CHECK(bsc_pat_format("chr1", (1ull << 63) + 1, NULL, 0, &ok, NULL, 0, NULL) < 0, "index_base above 2^63");
  CHECK(bsc_pat_format("chr1", 1ull << 63, NULL, 0, &ok, NULL, 0, NULL) == 0, "index_base 2^63");
  { /* the longest line: 64 sites, a count of ten digits, an index of nineteen */
    bsc_pat_rec big;
    big.idx = 0xfffffffeu;
    big.count = 0xffffffffu;
    big.hi = 0xaaaaaaaaaaaaaaaaull; /* 32 C */
    big.lo = 0xffffffffffffffffull; /* 32 T */
    const long len = bsc_pat_format(name, 1ull << 63, &big, 1, &ok, NULL, 0, NULL);
    CHECK(len == 255 + 1 + 19 + 1 + 64 + 1 + 10 + 1, "the longest line has %ld bytes", len);
    char *buf = malloc((size_t)len);
    CHECK(bsc_pat_format(name, 1ull << 63, &big, 1, &ok, buf, (size_t)len, NULL) == len && !memcmp(buf + 255, "\t9223372041149743103\tCCCC", 25) &&
              !memcmp(buf + len - 16, "TTTT\t4294967295\n", 16),
          "its columns");
    free(buf);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
