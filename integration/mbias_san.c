/*
 * mbias_san.c — TEST ONLY (make mbias-san; tests/test_mbias_host.py builds its own copy): the host form of the M-bias table (csrc/mbias.c) as a
 * stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer.  Seeded random raw blocks whose templates, read bytes, lists,
 * reference codes and table each live in a heap block of EXACTLY their size, so that a byte read or written beyond any of them stops the
 * program; every malformed-list form of the rule, reads and lists one beyond their buffers, extreme positions and sizes; the formatter at the
 * exact room, one short, and none.  Prints "ok" and exits 0, or names the case that failed.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bscall_amd.h"

/* csrc/mbias.c reports through bscall_api.c's channel; this program stands in for it */
#include <stdarg.h>
static char errbuf[512];
int bsc_set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, sizeof errbuf, fmt, ap);
  va_end(ap);
  return code;
}

#define CHECK(c, ...)                     \
  do {                                    \
    if (!(c)) {                           \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
      exit(1);                            \
    }                                     \
  } while (0)

static uint64_t rng_state;
static uint32_t rnd(void) { /* splitmix64 */
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
static uint32_t below(uint32_t n) { return n ? rnd() % n : 0; }

/* a heap block of exactly n bytes (n == 0: one that must never be touched is not needed — NULL) */
static void *exact(size_t n) {
  if (!n) return NULL;
  void *p = malloc(n);
  CHECK(p, "out of memory");
  return p;
}

/* one random block: mode 0 = mostly legal lists, 1 = arbitrary entries (mostly malformed), 2 = extreme values */
static void one_block(uint64_t seed, int mode, uint32_t n_cycles) {
  rng_state = seed;
  const uint32_t nr = below(40), x = 1000 + below(50), n_pos = 1 + below(300), y = x + n_pos - 1;
  bsc_raw_template *raw = exact((size_t)nr * sizeof *raw);
  /* sizes first */
  uint64_t seq_bytes = 0, n_misms = 0;
  for (uint32_t i = 0; i < nr; i++) {
    memset(&raw[i], 0, sizeof raw[i]);
    raw[i].bs_strand = (uint8_t)(mode == 2 ? below(5) : 1 + below(2));
    raw[i].orientation = (uint8_t)(mode == 2 ? below(3) : below(2));
    for (int k = 0; k < 2; k++) {
      if (below(4) == 0) continue;
      raw[i].len[k] = 1 + below(150);
      raw[i].off[k] = seq_bytes;
      seq_bytes += raw[i].len[k];
      raw[i].n_misms[k] = below(6);
      raw[i].misms_off[k] = n_misms;
      n_misms += raw[i].n_misms[k];
      raw[i].pos[k] = mode == 2 && below(4) == 0 ? 0xFFFFFFFFu - below(100) : x - 100 + below(n_pos + 200);
    }
  }
  uint8_t *seq = exact(seq_bytes);
  for (uint64_t i = 0; i < seq_bytes; i++) seq[i] = (uint8_t)rnd();
  bsc_misms *misms = exact(n_misms * sizeof *misms);
  for (uint32_t i = 0; i < nr; i++)
    for (int k = 0; k < 2; k++) {
      const uint32_t len = raw[i].len[k];
      uint32_t cursor = 0;
      for (uint32_t z = 0; z < raw[i].n_misms[k]; z++) {
        bsc_misms *m = &misms[raw[i].misms_off[k] + z];
        if (mode == 0) {
          m->type = z == 0 && below(3) == 0 ? BSC_MISMS_SOFT : below(3);
          m->position = m->type == BSC_MISMS_SOFT ? 0 : cursor + below(20);
          m->size = below(4);
          if (m->type != BSC_MISMS_INS && m->type != BSC_MISMS_MISMS) {
            if ((uint64_t)m->position + m->size > len) m->size = m->position <= len ? len - m->position : 0;
            if (m->position > len) m->position = len;
            cursor = m->position + m->size;
          } else if (m->type == BSC_MISMS_INS) cursor = m->position;
        } else {
          m->type = mode == 2 && below(8) == 0 ? rnd() : below(4);
          m->position = mode == 2 && below(4) == 0 ? 0xFFFFFFFFu - below(3) : below(len + 3);
          m->size = mode == 2 && below(4) == 0 ? 0xFFFFFFFFu - below(3) : below(len + 3);
        }
      }
    }
  if (mode == 2 && nr) { /* reads and lists one beyond their buffers, and far beyond */
    for (uint32_t i = 0; i < nr; i++) {
      const int k = (int)below(2);
      switch (below(6)) {
      case 0: raw[i].off[k] += seq_bytes - (raw[i].off[k] + raw[i].len[k]) + 1; break;
      case 1: raw[i].misms_off[k] = n_misms - raw[i].n_misms[k] + 1; break;
      case 2: raw[i].off[k] = UINT64_MAX - below(3); break;
      case 3: raw[i].misms_off[k] = UINT64_MAX - below(3); break;
      case 4: raw[i].len[k] = 0xFFFFFFFFu; break;
      default: break;
      }
    }
  }
  uint8_t *ref = exact((size_t)n_pos + 2);
  for (uint32_t i = 0; i < n_pos + 2; i++) ref[i] = (uint8_t)below(5);
  const size_t cells = (size_t)BSC_MBIAS_N_BINS * n_cycles * 2u;
  uint64_t *counts = exact(cells * sizeof *counts);
  memset(counts, 0, cells * sizeof *counts);
  uint64_t tot[8] = {0};
  const bsc_mbias_params p = {n_cycles};
  int rc = bsc_mbias_host(raw, nr, seq, seq_bytes, misms, n_misms, x, y, ref, 20, &p, counts, tot);
  CHECK(rc == BSC_OK, "seed %llu mode %d: rc %d (%s)", (unsigned long long)seed, mode, rc, errbuf);
  uint64_t sum = 0, n_reads = 0;
  for (size_t i = 0; i < cells; i++) sum += counts[i];
  for (uint32_t i = 0; i < nr; i++)
    for (int k = 0; k < 2; k++) n_reads += raw[i].len[k] != 0 && raw[i].bs_strand != 0;
  CHECK(sum == tot[2], "seed %llu mode %d: the cells sum to %llu, totals[2] is %llu", (unsigned long long)seed, mode, (unsigned long long)sum,
        (unsigned long long)tot[2]);
  CHECK(tot[0] + tot[6] == n_reads && tot[7] == 0 && tot[2] + tot[3] <= tot[1], "seed %llu mode %d: totals", (unsigned long long)seed, mode);
  /* NULL totals; twice the call doubles the table */
  rc = bsc_mbias_host(raw, nr, seq, seq_bytes, misms, n_misms, x, y, ref, 20, &p, counts, NULL);
  CHECK(rc == BSC_OK, "seed %llu: NULL totals", (unsigned long long)seed);
  uint64_t sum2 = 0;
  for (size_t i = 0; i < cells; i++) sum2 += counts[i];
  CHECK(sum2 == 2 * sum, "seed %llu: adding", (unsigned long long)seed);
  /* the formatter: the need, the exact room, one short */
  const long need = bsc_mbias_format(counts, &p, NULL, 0);
  CHECK(need >= 38, "seed %llu: format need %ld", (unsigned long long)seed, need);
  char *buf = exact((size_t)need);
  CHECK(bsc_mbias_format(counts, &p, buf, (size_t)need) == need && buf[need - 1] == '\n' && buf[0] == '#', "seed %llu: format", (unsigned long long)seed);
  char *small = exact((size_t)need - 1);
  memset(small, 0x5A, (size_t)need - 1);
  CHECK(bsc_mbias_format(counts, &p, small, (size_t)need - 1) == need, "seed %llu: format one short", (unsigned long long)seed);
  for (long i = 0; i < need - 1; i++) CHECK(small[i] == 0x5A, "seed %llu: a refused format wrote", (unsigned long long)seed);
  free(small);
  free(buf);
  free(counts);
  free(ref);
  free(misms);
  free(seq);
  free(raw);
}

/* every malformed-list form, each in a list buffer of exactly its size, with a read of 20 bytes in a buffer of exactly 20 */
static void malformed(void) {
  static const bsc_misms lists[][3] = {
      {{BSC_MISMS_DEL, 5, 2}, {BSC_MISMS_DEL, 6, 1}, {0, 0, 0}},
      {{BSC_MISMS_DEL, 5, 2}, {BSC_MISMS_INS, 6, 1}, {0, 0, 0}},
      {{BSC_MISMS_INS, 6, 1}, {BSC_MISMS_INS, 5, 1}, {0, 0, 0}},
      {{BSC_MISMS_DEL, 18, 3}, {0, 0, 0}, {0, 0, 0}},
      {{BSC_MISMS_MISMS, 0, 0}, {BSC_MISMS_SOFT, 15, 6}, {0, 0, 0}},
      {{BSC_MISMS_DEL, 0xFFFFFFFFu, 2}, {0, 0, 0}, {0, 0, 0}},
      {{BSC_MISMS_DEL, 2, 0xFFFFFFFFu}, {0, 0, 0}, {0, 0, 0}},
      {{BSC_MISMS_INS, 1, 1}, {BSC_MISMS_SOFT, 5, 2}, {BSC_MISMS_INS, 9, 1}},
      {{4, 1, 1}, {0, 0, 0}, {0, 0, 0}},
      {{0xFFFFFFFFu, 0, 0}, {0, 0, 0}, {0, 0, 0}},
  };
  const bsc_mbias_params p = {64};
  for (size_t c = 0; c < sizeof lists / sizeof lists[0]; c++) {
    bsc_misms *m = exact(sizeof lists[c]);
    memcpy(m, lists[c], sizeof lists[c]);
    uint8_t *seq = exact(20), *ref = exact(43);
    memset(seq, 1 | (40 << 2), 20);
    memset(ref, 2, 43);
    bsc_raw_template t;
    memset(&t, 0, sizeof t);
    t.bs_strand = 1;
    t.len[0] = 20;
    t.pos[0] = 1010;
    t.n_misms[0] = 3;
    uint64_t *counts = exact(12 * 64 * 2 * 8), tot[8] = {0};
    memset(counts, 0, 12 * 64 * 2 * 8);
    CHECK(bsc_mbias_host(&t, 1, seq, 20, m, 3, 1000, 1040, ref, 20, &p, counts, tot) == BSC_OK, "malformed %zu", c);
    CHECK(tot[6] == 1 && tot[0] == 0 && tot[1] == 0, "malformed %zu: not skipped", c);
    /* the read one beyond seq_bytes, the list one beyond n_misms */
    memset(tot, 0, sizeof tot);
    t.n_misms[0] = 0;
    CHECK(bsc_mbias_host(&t, 1, seq, 19, m, 3, 1000, 1040, ref, 20, &p, counts, tot) == BSC_OK && tot[6] == 1 && tot[0] == 0, "read one beyond");
    memset(tot, 0, sizeof tot);
    t.n_misms[0] = 1;
    t.misms_off[0] = 3;
    CHECK(bsc_mbias_host(&t, 1, seq, 20, m, 3, 1000, 1040, ref, 20, &p, counts, tot) == BSC_OK && tot[6] == 1 && tot[0] == 0, "list one beyond");
    /* and the legal read: 20 unconverted Cs in CHH context */
    memset(tot, 0, sizeof tot);
    t.n_misms[0] = 0;
    t.misms_off[0] = 0;
    CHECK(bsc_mbias_host(&t, 1, seq, 20, NULL, 0, 1000, 1040, ref, 20, &p, counts, tot) == BSC_OK && tot[0] == 1 && tot[1] == 20 && tot[2] == 20, "legal read");
    free(counts);
    free(ref);
    free(seq);
    free(m);
  }
}

int main(void) {
  static const uint32_t cycles[] = {1, 7, 64, 512, 1024};
  for (uint64_t seed = 1; seed <= 300; seed++)
    for (int mode = 0; mode < 3; mode++) one_block(seed * 3 + (uint64_t)mode, mode, cycles[seed % 5]);
  malformed();
  /* the refusals */
  uint64_t c[24] = {0};
  uint8_t ref[3] = {0, 0, 0};
  bsc_mbias_params p = {0};
  CHECK(bsc_mbias_host(NULL, 0, NULL, 0, NULL, 0, 1, 1, ref, 20, &p, c, NULL) == BSC_ERR_ARG, "n_cycles 0");
  p.n_cycles = 1025;
  CHECK(bsc_mbias_host(NULL, 0, NULL, 0, NULL, 0, 1, 1, ref, 20, &p, c, NULL) == BSC_ERR_ARG && bsc_mbias_format(c, &p, NULL, 0) < 0, "n_cycles 1025");
  p.n_cycles = 1;
  CHECK(bsc_mbias_host(NULL, 0, NULL, 0, NULL, 0, 2, 1, ref, 20, &p, c, NULL) == BSC_ERR_ARG, "y < x");
  CHECK(bsc_mbias_host(NULL, 0, NULL, 0, NULL, 0, 1, 1, ref, 20, &p, c, NULL) == BSC_OK, "no template");
  CHECK(bsc_mbias_host(NULL, 0, NULL, 0, NULL, 0, 1, 1, ref, 20, NULL, c, NULL) == BSC_ERR_ARG, "NULL params");
  bsc_mbias_params_default(&p);
  CHECK(p.n_cycles == 512, "default");
  printf("ok\n");
  return 0;
}
