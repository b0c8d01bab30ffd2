/*
 * tabix_san.c — TEST ONLY: the writer of the methylation tables' index (csrc/tabix.c: bsc_tbx_open_detached / _add / _members / _finish) and the
 * host form of the device scan (bsc_bed_entries_host over csrc/bedidx_core.h), stand-alone under AddressSanitizer + UndefinedBehaviorSanitizer
 * (make tabix-san; tests/test_tabix_host.py builds its own copy).  Streams, interval offsets and entries live in heap blocks of exactly their
 * size, so a read behind a stream or an entry behind the capacity stops the program.  Prints "ok" and returns 0, or names the case.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bscall_amd.h"

static char errbuf[512];
int bsc_set_error(int code, const char *fmt, ...) { /* the library's own lives in bscall_api.c */
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, sizeof errbuf, fmt, ap);
  va_end(ap);
  return code;
}

#define FAIL(...) do { fprintf(stderr, "tabix_san: " __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

/* a copy of exactly n bytes */
static void *exact(const void *src, size_t n) {
  void *p = malloc(n ? n : 1);
  if (n) memcpy(p, src, n);
  return p;
}

/* the host scan over a stream in a block of its own size: entries (cap of them, in a block of that size), totals */
static int scan(const char *text, size_t n, const uint64_t *sync, uint32_t n_sync, int min_shift, bsc_bed_entry **ent, uint64_t cap, uint64_t tot[3]) {
  uint8_t *s = exact(text, n);
  uint64_t *sy = sync ? exact(sync, ((size_t)n_sync + 1) * 8) : NULL;
  *ent = malloc(cap ? cap * sizeof **ent : 1);
  const int rc = bsc_bed_entries_host(n ? s : NULL, n, sy, n_sync, min_shift, cap ? *ent : NULL, cap, tot);
  free(s);
  free(sy);
  return rc;
}

static int scans(void) {
  static const char good[] = "c\t10\t12\tx\nc\t20\t22\tx\nc\t16383\t16385\tx\nc\t16390\t16392\tx\nc\t16391\t16392\n";
  const size_t n = sizeof good - 1;
  bsc_bed_entry *e = NULL;
  uint64_t tot[3];
  if (scan(good, n, NULL, 0, 14, &e, 8, tot) || tot[0] != 3 || tot[1] != 5 || tot[2]) FAIL("whole stream: %llu %llu %llu", (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2]);
  if (e[0].win_beg != 0 || e[0].win_last != 0 || e[0].n_lines != 2 || e[0].u_beg != 0 || e[1].win_beg != 0 || e[1].win_last != 1 || e[1].n_lines != 1 ||
      e[1].u_beg != 20 || e[2].win_beg != 1 || e[2].win_last != 1 || e[2].n_lines != 2 || e[2].zero || e[2].u_beg != 36)
    FAIL("whole stream: the entries");
  free(e);
  if (scan(good, n, NULL, 0, 14, &e, 2, tot) || tot[0] != 3 || tot[1] != 5) FAIL("a capacity one short"); /* (ASan: nothing behind the two) */
  free(e);
  if (scan(good, n, NULL, 0, 14, &e, 0, tot) || tot[0] != 3) FAIL("no capacity");
  free(e);
  const uint64_t sync[] = {0, 0, 10, 20, 20, 36, n, n};
  if (scan(good, n, sync, 7, 14, &e, 16, tot) || tot[0] != 4 || tot[1] != 5 || tot[2]) FAIL("intervals");
  free(e);
  for (int ms = 0; ms <= 31; ms++) {
    if (scan(good, n, sync, 7, ms, &e, 16, tot) || tot[1] != 5 || tot[2]) FAIL("min_shift %d", ms);
    free(e);
  }
  if (scan(good, 0, NULL, 0, 14, &e, 4, tot) || tot[0] || tot[1] || tot[2]) FAIL("an empty stream");
  free(e);
  /* every prefix of the stream: a walk never reads behind its interval */
  for (size_t k = 0; k <= n; k++) {
    if (scan(good, k, NULL, 0, 14, &e, 8, tot)) FAIL("prefix %zu", k);
    const int whole = k == 0 || good[k - 1] == '\n';
    if ((tot[2] != 0) == whole) FAIL("prefix %zu: error bits %llu", k, (unsigned long long)tot[2]);
    free(e);
  }
  static const struct {
    const char *s;
    uint64_t err;
  } bad[] = {{"c\t5\t7\nc\t4\t9\n", 2},    {"c 5 7\n", 4},      {"c\tx\t7\n", 4},         {"c\t5\n", 4},          {"c\t5\t5\n", 4},
             {"c\t5\t4294967297\n", 4}, {"c\t5\t4294967296\n", 0}, {"c\t12345678901\t7\n", 4}, {"c\t5\t12345678901\n", 4}, {"\n", 4},
             {"c\t5\t7", 1},            {"c\t5", 1},           {"c", 1},                 {"c\t5\t7x\n", 4},      {"c\t4294967295\t4294967296\n", 0}};
  for (size_t k = 0; k < sizeof bad / sizeof bad[0]; k++) {
    if (scan(bad[k].s, strlen(bad[k].s), NULL, 0, 14, &e, 4, tot) || tot[2] != bad[k].err) FAIL("damaged stream %zu: error bits %llu", k, (unsigned long long)tot[2]);
    free(e);
  }
  const uint64_t desc[] = {0, 36, 20, n}, beyond[] = {0, n + 1};
  if (scan(good, n, desc, 3, 14, &e, 8, tot) || !(tot[2] & 8)) FAIL("descending offsets");
  free(e);
  if (scan(good, n, beyond, 1, 14, &e, 8, tot) || tot[2] != 8) FAIL("offsets beyond the stream");
  free(e);
  if (bsc_bed_entries_host(good, n, NULL, 0, 32, NULL, 0, tot) != BSC_ERR_ARG || bsc_bed_entries_host(good, n, NULL, 0, 14, NULL, 0, NULL) != BSC_ERR_ARG)
    FAIL("the argument checks");
  return 0;
}

static long finish(bsc_tbx *ix, uint8_t **out) {
  const long need = bsc_tbx_finish(ix, NULL, 0);
  if (need < 0) return need;
  *out = malloc((size_t)need); /* exactly: a byte too many written stops the program */
  if (bsc_tbx_finish(ix, *out, (uint64_t)need - 1) != need) return -100;
  return bsc_tbx_finish(ix, *out, (uint64_t)need);
}

static int writer(int kind) {
  enum { NREF = 300 };
  char *names[NREF];
  uint32_t lens[NREF];
  for (int i = 0; i < NREF; i++) {
    char b[16];
    snprintf(b, sizeof b, "c%d", i);
    names[i] = exact(b, strlen(b) + 1);
    lens[i] = kind == BSC_TBX_TBI ? (uint32_t)1 << 29 : ((uint32_t)1 << 29) + 1;
  }
  bsc_tbx *ix = NULL;
  if (bsc_tbx_open_detached(kind, 14, NREF, (const char *const *)names, lens, 0, &ix)) FAIL("open: %s", errbuf);
  uint64_t logical = 0;
  for (int t = 1; t < NREF; t += 2) { /* every other contig has lines: one add of scanned text, one of crafted entries up to the last window */
    char text[256];
    const int n = snprintf(text, sizeof text, "c%d\t%d\t%d\nc%d\t16383\t16385\nc%d\t16383\t16384\nc%d\t%d\t%d\n", t, t, t + 1, t, t, t, 5 << 14, (5 << 14) + 40000);
    bsc_bed_entry *e = NULL;
    uint64_t tot[3];
    if (scan(text, (size_t)n, NULL, 0, 14, &e, 8, tot) || tot[2] || tot[0] != 4) FAIL("contig %d: the scan", t);
    if (bsc_tbx_add(ix, t, e, tot[0], (uint64_t)n)) FAIL("contig %d: add: %s", t, errbuf);
    free(e);
    logical += (uint64_t)n;
    const uint32_t top = kind == BSC_TBX_TBI ? 32767u : 32768u;
    const bsc_bed_entry c[3] = {{8, 8, 70000, 0, 0}, {4095, 4096, 1, 0, 70000}, {top - 1, top, 2, 0, 70010}};
    bsc_bed_entry *ce = exact(c, sizeof c);
    if (bsc_tbx_add(ix, t, ce, 3, 0x20000)) FAIL("contig %d: crafted add: %s", t, errbuf);
    logical += 0x20000;
    /* refusals: each leaves the index as it was */
    const bsc_bed_entry r[][2] = {{{7, 7, 1, 0, 0}, {0}},          {{top, top, 0, 0, 0}, {0}}, {{top, top - 1, 1, 0, 0}, {0}}, {{top, top, 1, 0, 1}, {0}},
                                  {{top, top, 1, 0, 0}, {top, top, 1, 0, 0}}, {{top, 1u << 18, 1, 0, 0}, {0}}, {{1u << 18, 1u << 18, 1, 0, 0}, {0}}};
    for (size_t k = 0; k < sizeof r / sizeof r[0]; k++) {
      bsc_bed_entry *re = exact(r[k], sizeof r[k]);
      if (bsc_tbx_add(ix, t, re, k == 4 ? 2 : 1, 50) != BSC_ERR_ARG) FAIL("contig %d: refusal %zu was taken", t, k);
      free(re);
    }
    if (t > 1 && bsc_tbx_add(ix, t - 1, ce, 3, 0x20000) != BSC_ERR_ARG) FAIL("a descending contig was taken");
    free(ce);
    if (bsc_tbx_add(ix, t, NULL, 0, 0)) FAIL("an empty block: %s", errbuf);
  }
  uint8_t *out = NULL;
  if (finish(ix, &out) != BSC_ERR_ARG) FAIL("finish before the members");
  const uint64_t nm = (logical + 0xFEFF) / 0xFF00;
  uint64_t *sizes = malloc(nm * 8);
  for (uint64_t k = 0; k < nm; k++) sizes[k] = 28 + (k * 7919) % 65000;
  if (bsc_tbx_members(ix, sizes, nm - 1) != BSC_ERR_ARG || bsc_tbx_members(ix, sizes, nm)) FAIL("members: %s", errbuf);
  free(sizes);
  const long got = finish(ix, &out);
  if (got < 28 + 31) FAIL("finish: %ld %s", got, errbuf);
  if (memcmp(out + got - 28, "\x1f\x8b\x08\x04", 4) || memcmp(out + 18 + 5, kind == BSC_TBX_TBI ? "TBI\1" : "CSI\1", 4)) FAIL("the file's frame");
  free(out);
  if (bsc_tbx_add(ix, NREF - 1, NULL, 0, 0) != BSC_ERR_ARG) FAIL("an add after the members");
  bsc_tbx_close(ix);
  if (bsc_tbx_finish(ix, NULL, 0) != BSC_ERR_ARG) FAIL("a closed index");
  bsc_tbx_close(ix);
  for (int i = 0; i < NREF; i++) free(names[i]);
  return 0;
}

int main(void) {
  if (scans()) return 1;
  if (writer(BSC_TBX_TBI) || writer(BSC_TBX_CSI)) return 1;
  bsc_tbx *ix = NULL;
  const char *nm[1] = {"big"};
  const uint32_t ln[1] = {((uint32_t)1 << 29) + 1};
  if (bsc_tbx_open_detached(BSC_TBX_TBI, 14, 1, nm, ln, 0, &ix) != BSC_ERR_ARG || !strstr(errbuf, "csi")) FAIL("a long contig for a .tbi: %s", errbuf);
  if (bsc_tbx_open_detached(BSC_TBX_TBI, 10, 1, nm, ln, 0, &ix) != BSC_ERR_ARG || bsc_tbx_open_detached(5, 14, 1, nm, ln, 0, &ix) != BSC_ERR_ARG) FAIL("open's checks");
  if (bsc_tbx_open_detached(BSC_TBX_CSI, 14, 0, NULL, NULL, 0, &ix)) FAIL("no contigs: %s", errbuf);
  if (bsc_tbx_members(ix, NULL, 0)) FAIL("no members: %s", errbuf);
  uint8_t *out = NULL;
  if (finish(ix, &out) < 28) FAIL("an empty index: %s", errbuf);
  free(out);
  bsc_tbx_close(ix);
  puts("ok");
  return 0;
}
