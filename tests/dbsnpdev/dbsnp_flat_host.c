/*
 * csrc/dbsnpdev_core.h and the flattening of csrc/dbsnp.c on the CPU: a stand-alone program (tests/test_dbsnp_flat_host.py compiles it
 * with csrc/dbsnp.c under AddressSanitizer + UndefinedBehaviorSanitizer and runs it).  For every contig named on the command line
 * (one the index lacks attaches empty) the flat arrays are read with the statements the kernels of csrc/dbsnpdev.hip run and compared
 * with the reader's own answers, bsc_dbsnp_flags / bsc_dbsnp_name / bsc_dbsnp_names:
 *   - every entry: position, length, bytes; every position of the contig (and 200 beyond either end): the flag
 *   - around chosen bins: every x0 of the bin +- 1, every n of 0 .. 200: the flags as the kernel forms them (a head of bytes, 16-byte
 *     words from bsc_dbf_window, a tail), for every head 0 .. 15; bsc_dbf_count's names and bytes; the names table
 *   - ranges that start before the first bin, end behind the last, and end at position 2^32 - 1
 *
 *   dbsnp_flat_host INDEX CONTIG...          prints "ok"
 *   dbsnp_flat_host --refuse INDEX CONTIG    the flattening must refuse the contig with BSC_ERR_ARG: prints its message
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bscall_amd.h"
#include "dbsnpdev_core.h"

static char errbuf[512];
int bsc_set_error(int code, const char *fmt, ...) { /* bscall_api.c's, which dbsnp.c reports through */
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, sizeof errbuf, fmt, ap);
  va_end(ap);
  return code;
}

#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                             \
      printf("\n");                                    \
      exit(1);                                         \
    }                                                  \
  } while (0)

/* the flags of x0 .. x0 + n - 1 the way bsc_dbsnp_flags_kernel forms them when `head` bytes lie in front of the first 16-byte boundary */
static void flags_like_kernel(const bsc_dbsnp_flat *f, uint32_t x0, uint32_t n, uint32_t head, uint8_t *out) {
  if (head > n) head = n;
  const uint32_t n_vec = (n - head) / 16u, edge = n - 16u * n_vec;
  for (uint32_t i = 0; i < n_vec + edge; i++) {
    if (i < n_vec) {
      const uint32_t k = head + 16u * i;
      uint64_t m, q;
      bsc_dbf_window(f, (uint64_t)x0 + k, &m, &q);
      for (unsigned w = 0; w < 4; w++) {
        const uint32_t v = bsc_dbf_flags4((unsigned)(m >> (4 * w)) & 15u, (unsigned)(q >> (4 * w)) & 15u);
        memcpy(out + k + 4u * w, &v, 4);
      }
    } else {
      const uint32_t j = i - n_vec, k = j < head ? j : head + 16u * n_vec + (j - head);
      out[k] = (uint8_t)bsc_dbf_flag(f, (uint64_t)x0 + k);
    }
  }
}

#define MAXN 200u
static void check_range(const bsc_dbsnp *db, const bsc_dbsnp_flat *f, uint32_t x0, uint32_t n, int all_heads) {
  static uint8_t want[MAXN + 64], got[MAXN + 64];
  static uint32_t pos[MAXN + 1], off[MAXN + 2];
  static char by[(MAXN + 1) * 600];
  CHECK(n <= MAXN, "n");
  CHECK(bsc_dbsnp_flags(db, x0, n, want) == BSC_OK, "%s", errbuf);
  for (uint32_t head = 0; head < (all_heads ? 16u : 1u); head++) {
    memset(got, 0xee, sizeof got);
    flags_like_kernel(f, x0, n, head, got);
    CHECK(!memcmp(got, want, n) && got[n] == 0xee, "flags x0=%u n=%u head=%u", x0, n, head);
  }
  uint32_t k = 0, e0, nn;
  uint64_t nb = 0, nbytes;
  CHECK(bsc_dbsnp_names(db, x0, n, NULL, NULL, NULL, 0, 0, &k, &nb) == BSC_OK, "%s", errbuf);
  bsc_dbf_count(f, x0, n, &e0, &nn, &nbytes);
  CHECK(nn == k && nbytes == nb, "count x0=%u n=%u: %u names / %llu bytes, the reader has %u / %llu", x0, n, nn, (unsigned long long)nbytes, k,
        (unsigned long long)nb);
  CHECK(bsc_dbsnp_names(db, x0, n, pos, off, by, MAXN + 1, sizeof by, &k, &nb) == BSC_OK, "%s", errbuf);
  for (uint32_t i = 0; i <= nn; i++) {
    CHECK(f->txt[e0 + i] - f->txt[e0] == off[i], "off[%u] x0=%u n=%u", i, x0, n);
    if (i == nn) break;
    char nm[600];
    const uint32_t l = bsc_dbf_entry_len(f, e0 + i);
    CHECK(bsc_dbf_entry_pos(f, e0 + i) == pos[i], "pos[%u] x0=%u n=%u", i, x0, n);
    CHECK(l == off[i + 1] - off[i], "length of name %u x0=%u n=%u", i, x0, n);
    bsc_dbf_entry_name(f, e0 + i, nm);
    CHECK(!memcmp(nm, by + off[i], l), "bytes of name %u x0=%u n=%u", i, x0, n);
  }
}

static void check_contig(bsc_dbsnp *db, const char *name) {
  uint64_t n_snps = 0;
  CHECK(bsc_dbsnp_load_contig(db, name, &n_snps) == BSC_OK, "%s", errbuf);
  bsc_dbsnp_flat_blob blob;
  CHECK(bsc_dev_dbsnp_flatten(db, &blob) == BSC_OK, "%s", errbuf);
  const bsc_dbsnp_flat f = bsc_dbf_view(&blob, blob.blob);
  CHECK(f.n_entries == n_snps, "%s: %u entries flattened, %llu loaded", name, f.n_entries, (unsigned long long)n_snps);
  CHECK(f.ent_first[f.n_bins] == f.n_entries && f.ent_first[0] == 0, "ent_first");
  /* every entry, against the reader's lookup at its position */
  uint32_t prev = 0;
  for (uint32_t e = 0; e < f.n_entries; e++) {
    const uint32_t x = bsc_dbf_entry_pos(&f, e);
    CHECK(e == 0 || x > prev, "entry %u: positions must ascend", e);
    prev = x;
    CHECK((x & 63u) == (f.ent[e] & 63u), "entry %u: select and the entry's own bit differ", e);
    char rs[600], nm[600];
    size_t l = 0;
    const int r = bsc_dbsnp_name(db, x, rs, sizeof rs, &l);
    CHECK(r == 1 || r == 3, "entry %u at %u: the reader finds %d", e, x, r);
    CHECK((unsigned)r == bsc_dbf_flag(&f, x), "entry %u at %u: flag", e, x);
    CHECK(bsc_dbf_entry_len(&f, e) == l && f.txt[e + 1] - f.txt[e] == l, "entry %u at %u: length %u, the reader has %zu", e, x, bsc_dbf_entry_len(&f, e), l);
    memset(nm, 0x55, sizeof nm);
    bsc_dbf_entry_name(&f, e, nm);
    CHECK(!memcmp(nm, rs, l) && nm[l] == 0x55, "entry %u at %u: bytes", e, x);
    CHECK(bsc_dbf_rank(&f, x) == e && bsc_dbf_rank(&f, (uint64_t)x + 1) == e + 1, "entry %u at %u: rank", e, x);
  }
  /* every position of the contig and 200 to either side */
  const uint64_t first = (uint64_t)f.min_bin * 64u > 200u ? (uint64_t)f.min_bin * 64u - 200u : 1u;
  const uint64_t last = ((uint64_t)f.min_bin + f.n_bins) * 64u + 200u;
  {
    const uint32_t chunk = 1u << 16;
    uint8_t *want = malloc(chunk);
    CHECK(want != NULL, "malloc");
    uint64_t flagged = 0;
    for (uint64_t x = first; x <= last; x += chunk) {
      const uint32_t n = (uint32_t)(last - x + 1 < chunk ? last - x + 1 : chunk);
      CHECK(bsc_dbsnp_flags(db, (uint32_t)x, n, want) == BSC_OK, "%s", errbuf);
      for (uint32_t i = 0; i < n; i++) {
        CHECK(bsc_dbf_flag(&f, x + i) == want[i], "flag of position %llu", (unsigned long long)(x + i));
        flagged += want[i] != 0;
      }
    }
    free(want);
    CHECK(flagged == f.n_entries, "%llu positions flagged, %u entries", (unsigned long long)flagged, f.n_entries);
  }
  /* the ranges: around the first bin, the last bin, the bins behind the widest gap, and the fullest bin */
  uint32_t pick[8], np = 0, fullest = 0, gap_at = 0, gap = 0, run = 0;
  for (uint32_t b = 0; b < f.n_bins; b++) {
    if (__builtin_popcountll(f.mask[b]) > __builtin_popcountll(f.mask[fullest])) fullest = b;
    if (!f.mask[b]) run++;
    else {
      if (run > gap) {
        gap = run;
        gap_at = b;
      }
      run = 0;
    }
  }
  pick[np++] = f.min_bin;
  pick[np++] = f.min_bin + (f.n_bins ? f.n_bins - 1u : 0u);
  pick[np++] = f.min_bin + fullest;
  pick[np++] = f.min_bin + fullest + 1u;
  pick[np++] = f.min_bin + gap_at;
  pick[np++] = f.min_bin + f.n_bins + 3u; /* behind everything */
  if (f.min_bin > 2u) pick[np++] = f.min_bin - 2u; /* in front of everything */
  for (uint32_t p = 0; p < np; p++)
    for (uint64_t x0 = (uint64_t)pick[p] * 64u - (pick[p] ? 1u : 0u); x0 <= (uint64_t)pick[p] * 64u + 64u; x0++) {
      if (x0 < 1u) continue;
      for (uint32_t n = 0; n <= MAXN; n++) check_range(db, &f, (uint32_t)x0, n, n <= 40u || n >= MAXN - 2u);
    }
  /* the end of the 32-bit positions: x0 + n - 1 = 2^32 - 1 asks bsc_dbf_rank for position 2^32 */
  for (uint32_t n = 1; n <= 70u; n++) check_range(db, &f, 0xffffffffu - n + 1u, n, 0);
  bsc_dev_dbsnp_flat_free(&blob);
  CHECK(blob.blob == NULL, "free");
}

int main(int argc, char **argv) {
  bsc_dbsnp *db = NULL;
  if (argc == 4 && !strcmp(argv[1], "--refuse")) {
    CHECK(bsc_dbsnp_open(argv[2], &db) == BSC_OK, "%s", errbuf);
    CHECK(bsc_dbsnp_load_contig(db, argv[3], NULL) == BSC_OK, "%s", errbuf);
    bsc_dbsnp_flat_blob blob;
    const int rc = bsc_dev_dbsnp_flatten(db, &blob);
    CHECK(rc == BSC_ERR_ARG && blob.blob == NULL, "the flattening answered %d", rc);
    printf("%s\n", errbuf);
    bsc_dbsnp_close(db);
    return 0;
  }
  if (argc < 3) {
    fprintf(stderr, "usage: %s [--refuse] INDEX CONTIG...\n", argv[0]);
    return 2;
  }
  CHECK(bsc_dbsnp_open(argv[1], &db) == BSC_OK, "%s", errbuf);
  { /* nothing loaded yet: an empty block */
    bsc_dbsnp_flat_blob blob;
    CHECK(bsc_dev_dbsnp_flatten(db, &blob) == BSC_OK && blob.n_entries == 0 && blob.n_bins == 0, "%s", errbuf);
    const bsc_dbsnp_flat f = bsc_dbf_view(&blob, blob.blob);
    check_range(db, &f, 1, 200, 1);
    bsc_dev_dbsnp_flat_free(&blob);
  }
  for (int i = 2; i < argc; i++) check_contig(db, argv[i]);
  bsc_dbsnp_close(db);
  printf("ok\n");
  return 0;
}
