/*
 * frag_san.c — TEST ONLY: the host form of the per-region fragment methylation summary (csrc/frag.c) as a stand-alone program, built with
 * -fsanitize=address,undefined (make frag-san): seeded random templates, read bytes, reference codes and regions in heap blocks of exactly
 * their size, so that one byte read or written too far is an error; reads that claim to lie outside the read buffer; NULL totals; regions
 * in front of, across and behind the block; the formatter's rooms (too small by one, exact, none) and the refusals.  Prints "ok" and exits
 * 0, or names the case that failed.  No GPU, no Python.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bscall_amd.h"

/* csrc/frag.c reports through the library's channel; here it is this */
#include <stdarg.h>
static char errbuf[512];
int bsc_set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, sizeof errbuf, fmt, ap);
  va_end(ap);
  return code;
}

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}

#define FAIL(...)                 \
  do {                            \
    fprintf(stderr, __VA_ARGS__); \
    fprintf(stderr, "\n");        \
    return 1;                     \
  } while (0)

static int one_block(uint32_t n_pos, uint32_t nr, uint32_t n_reg, int null_totals) {
  const uint32_t x = 1 + rnd(5000), y = x + n_pos - 1;
  uint8_t *ref = malloc(n_pos + 2);
  for (uint32_t i = 0; i < n_pos + 2; i++) ref[i] = (uint8_t)(1 + rnd(4));
  for (uint32_t i = rnd(6); i + 1 < n_pos + 2; i += 3 + rnd(12)) ref[i] = 2, ref[i + 1] = 3;
  bsc_template *tpl = calloc(nr ? nr : 1, sizeof *tpl);
  uint64_t seq_bytes = 0;
  for (uint32_t r = 0; r < nr; r++) {
    tpl[r].bs_strand = (uint8_t)rnd(4);
    for (int k = 0; k < 2; k++) {
      if (rnd(4) == 0) continue;
      tpl[r].len[k] = 1 + rnd(150);
      tpl[r].pos[k] = x > 80 ? x - 80 + rnd(n_pos + 120) : 1 + rnd(n_pos + 120);
      tpl[r].off[k] = seq_bytes;
      seq_bytes += tpl[r].len[k];
    }
  }
  uint8_t *seq = malloc(seq_bytes ? seq_bytes : 1);
  for (uint64_t i = 0; i < seq_bytes; i++) seq[i] = (uint8_t)(rnd(4) | (rnd(8) ? 20 + rnd(22) : rnd(64)) << 2);
  if (nr > 2) { /* a read one byte beyond the buffer and one far beyond it: both absent */
    tpl[0].len[0] = 10, tpl[0].off[0] = seq_bytes - 9;
    tpl[1].len[1] = 5, tpl[1].off[1] = seq_bytes + 1000;
  }
  bsc_meth_region *reg = malloc((n_reg ? n_reg : 1) * sizeof *reg);
  for (uint32_t k = 0; k < n_reg; k++) {
    reg[k].start = (x > 60 ? x - 60 : 0) + rnd(n_pos + 100);
    reg[k].end = reg[k].start + (rnd(5) ? rnd(400) : 0);
  }
  if (n_reg > 1) reg[0].start = x - 1, reg[0].end = y;
  uint64_t *acc = calloc((size_t)(n_reg ? n_reg : 1) * 8, sizeof *acc), tot[8];
  bsc_frag_params p;
  bsc_frag_params_default(&p);
  p.min_sites = 1 + rnd(4);
  int rc = bsc_frag_regions_host(tpl, nr, seq, seq_bytes, x, y, ref, 20, &p, n_reg ? reg : NULL, n_reg, n_reg ? acc : NULL, null_totals ? NULL : tot);
  if (rc) FAIL("bsc_frag_regions_host: %d (%s)", rc, errbuf);
  uint64_t sum[7] = {0};
  for (uint32_t k = 0; k < n_reg; k++) {
    const uint64_t *a = acc + 8 * (size_t)k;
    if (a[0] != a[1] + a[2] + a[3] || a[5] > a[4] || a[6] > a[0] || a[4] < a[0] * p.min_sites) FAIL("region %u: sums that cannot be", k);
    for (int c = 0; c < 7; c++) sum[c] += a[c];
  }
  if (!null_totals)
    for (int c = 0; c < 7; c++)
      if (tot[1 + c] != sum[c]) FAIL("totals[%d] is not the column's sum", 1 + c);
  if (!null_totals && tot[0] > nr) FAIL("more templates with a state than templates");
  /* the formatter: the need, a room one short (nothing written), the exact room */
  const long need = bsc_frag_format("chr1", reg, NULL, acc, n_reg, NULL, 0);
  if (need < 0) FAIL("bsc_frag_format: %ld", need);
  char *buf = malloc(need ? (size_t)need : 1);
  if (need > 0) {
    memset(buf, 0x5a, (size_t)need);
    if (bsc_frag_format("chr1", reg, NULL, acc, n_reg, buf, (size_t)need - 1) != need || buf[0] != 0x5a) FAIL("a room one short");
    if (bsc_frag_format("chr1", reg, NULL, acc, n_reg, buf, (size_t)need) != need || buf[need - 1] != '\n') FAIL("the exact room");
    uint32_t lines = 0;
    for (long i = 0; i < need; i++) lines += buf[i] == '\n';
    if (lines != n_reg) FAIL("%u lines for %u regions", lines, n_reg);
  }
  free(buf);
  free(acc);
  free(reg);
  free(seq);
  free(tpl);
  free(ref);
  return 0;
}

int main(void) {
  static const uint32_t shapes[][3] = {{1, 0, 0}, {1, 1, 1}, {63, 5, 3}, {64, 70, 9}, {65, 64, 64}, {300, 200, 65}, {2000, 700, 129}, {5000, 50, 300}};
  for (size_t s = 0; s < sizeof shapes / sizeof shapes[0]; s++)
    for (int nt = 0; nt < 2; nt++)
      if (one_block(shapes[s][0], shapes[s][1], shapes[s][2], nt)) {
        fprintf(stderr, "frag_san: shape %zu (%u positions, %u templates, %u regions) failed\n", s, shapes[s][0], shapes[s][1], shapes[s][2]);
        return 1;
      }
  /* the refusals */
  bsc_frag_params p;
  uint8_t ref[3] = {2, 3, 1};
  uint64_t acc[8] = {0};
  bsc_meth_region r = {0, 5}, bad_r = {5, 4};
  const char *names[1] = {"a\tb"};
  bsc_frag_params_default(&p);
  bsc_frag_params_default(NULL);
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, ref, 20, &p, &r, 1, acc, NULL) != BSC_OK) FAIL("an empty block is legal");
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 2, 1, ref, 20, &p, &r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("y < x");
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, ref, 20, &p, &bad_r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("start > end");
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, NULL, 20, &p, &r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("NULL ref");
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, ref, 20, NULL, &r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("NULL params");
  p.min_sites = 0;
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, ref, 20, &p, &r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("min_sites 0");
  bsc_frag_params_default(&p);
  p.m_min_pct = 101;
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, ref, 20, &p, &r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("a percentage above 100");
  bsc_frag_params_default(&p);
  p.u_max_pct = 75;
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, ref, 20, &p, &r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("u_max_pct == m_min_pct");
  bsc_frag_params_default(&p);
  p.reserved = 1;
  if (bsc_frag_regions_host(NULL, 0, NULL, 0, 1, 1, ref, 20, &p, &r, 1, acc, NULL) != BSC_ERR_ARG) FAIL("reserved");
  if (bsc_frag_format("", &r, NULL, acc, 1, NULL, 0) >= 0 || bsc_frag_format("c", &r, names, acc, 1, NULL, 0) >= 0 ||
      bsc_frag_format(NULL, &r, NULL, acc, 1, NULL, 0) >= 0 || bsc_frag_format("c", NULL, NULL, acc, 1, NULL, 0) >= 0 ||
      bsc_frag_format("c", &r, NULL, acc, 1, NULL, 4) >= 0)
    FAIL("the formatter's refusals");
  if (bsc_frag_format("c", NULL, NULL, NULL, 0, NULL, 0) != 0) FAIL("no region, no byte");
  puts("ok");
  return 0;
}
