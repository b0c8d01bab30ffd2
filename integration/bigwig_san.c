/*
 * bigwig_san.c — the writer of the methylation bigWig file (csrc/bigwig.c: bsc_bigwig_open / _add / _finish / _close, and the host form
 * bsc_bigwig_sections_recs) as a stand-alone program for the address and undefined-behaviour sanitizers: `make bigwig-san` compiles this
 * file and csrc/bigwig.c with -fsanitize=address,undefined and nothing else — no device, no library.  It drives the writer over crafted
 * entries — 0, 1, 256, 257 and 65 537 sections; 1, 2, 256, 257 and 300 contigs; one and several blocks; refused calls — and checks what
 * the file's own offsets say.  Prints "ok" and returns 0, or names the case that failed.
 */
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

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
#define EXPECT(cond, what)                                         \
  do {                                                             \
    if (!(cond)) {                                                 \
      fprintf(stderr, "bigwig_san: %s (line %d): %s\n", what, __LINE__, errbuf); \
      failures++;                                                  \
    }                                                              \
  } while (0)

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

/* n_sites sites on contig tid at starts first, first + step, ..: as packed records the host form turns into a block */
static bsc_vcf_rec *make_recs(uint64_t n_sites, uint32_t first, uint32_t step) {
  bsc_vcf_rec *r = calloc(n_sites ? n_sites : 1, sizeof *r);
  for (uint64_t i = 0; i < n_sites; i++) {
    r[i].core.pos = first + 1u + (uint32_t)i * step;
    r[i].core.emit = 1;
    r[i].core.gt = i % 3 ? 4 : 7;
    r[i].core.cg = 'C';
    r[i].counts[5] = r[i].counts[6] = (uint32_t)(i % 7);
    r[i].counts[7] = r[i].counts[4] = (uint32_t)(1 + i % 5);
  }
  return r;
}

/* one file: n_refs contigs, the given blocks of (tid, n_sites); returns the bytes (malloc) */
static uint8_t *one_file(uint32_t n_refs, uint32_t S, uint32_t red, const uint32_t *tids, const uint64_t *sites, int n_blocks, size_t *len, const char *what) {
  char path[] = "/tmp/bigwig_san_XXXXXX";
  const int fd = mkstemp(path);
  EXPECT(fd >= 0, "mkstemp");
  char **names = calloc(n_refs ? n_refs : 1, sizeof *names);
  uint32_t *lens = calloc(n_refs ? n_refs : 1, sizeof *lens);
  for (uint32_t k = 0; k < n_refs; k++) {
    names[k] = malloc(32);
    snprintf(names[k], 32, "c%u%s", (n_refs - k) * 7u % 1000u, k % 3 ? "_long_name" : ""); /* not in memcmp order; two lengths */
    lens[k] = 4000000u;
  }
  const bsc_bw_params bp = {S, red};
  bsc_meth_params mp;
  memset(&mp, 0, sizeof mp);
  mp.min_cov = 1;
  bsc_bigwig *bw = NULL;
  EXPECT(bsc_bigwig_open(fd, n_refs, (const char *const *)names, lens, &bp, &bw) == BSC_OK && bw, what);
  uint64_t total_sec = 0;
  uint32_t next_start = 0, last_tid = 0;
  for (int b = 0; b < n_blocks && bw; b++) {
    if (b && tids[b] != last_tid) next_start = 0;
    last_tid = tids[b];
    bsc_vcf_rec *recs = make_recs(sites[b], next_start, 3);
    uint64_t nb = 0, ns = 0, nz = 0;
    const int rc0 = bsc_bigwig_sections_recs(recs, sites[b], tids[b], &mp, &bp, NULL, 0, &nb, NULL, &ns, NULL, &nz);
    EXPECT(sites[b] ? rc0 == BSC_ERR_ARG : rc0 == BSC_OK, "the sizing call");
    uint8_t *data = malloc(nb ? nb : 1);
    bsc_bw_sum *sec = malloc((ns ? ns : 1) * sizeof *sec), *zoom = malloc((nz ? nz : 1) * sizeof *zoom);
    EXPECT(bsc_bigwig_sections_recs(recs, sites[b], tids[b], &mp, &bp, data, nb, &nb, sec, &ns, zoom, &nz) == BSC_OK, "the host form");
    EXPECT(ns == (sites[b] + S - 1) / S && nb == 24 * ns + 8 * sites[b], "the block's sizes");
    EXPECT(bsc_bigwig_add(bw, tids[b], data, nb, sec, ns, zoom, nz) == BSC_OK, what);
    total_sec += ns;
    next_start += (uint32_t)sites[b] * 3u;
    free(recs);
    free(data);
    free(sec);
    free(zoom);
  }
  EXPECT(bw && bsc_bigwig_finish(bw) == BSC_OK, what);
  EXPECT(bw && bsc_bigwig_finish(bw) == BSC_ERR_ARG, "a second finish is refused");
  bsc_bigwig_close(bw);
  const off_t end = lseek(fd, 0, SEEK_END);
  uint8_t *raw = malloc((size_t)end + 1);
  EXPECT(pread(fd, raw, (size_t)end, 0) == end, "reading the file back");
  close(fd);
  unlink(path);
  *len = (size_t)end;
  EXPECT(end >= 300 && rd32(raw) == 0x888FFC26u && rd32(raw + end - 4) == 0x888FFC26u, "the two magics");
  const uint64_t data_at = rd64(raw + 16), index_at = rd64(raw + 24);
  EXPECT(rd64(raw + 8) == 296 && rd32(raw + 296) == 0x78CA8C91u && rd64(raw + 296 + 16) == n_refs, "the chromosome tree's header");
  EXPECT(data_at < (uint64_t)end && rd64(raw + data_at) == total_sec, "the section count");
  EXPECT(index_at + 48 <= (uint64_t)end && rd32(raw + index_at) == 0x2468ACE0u && rd64(raw + index_at + 8) == total_sec, "the R-tree's header");
  const unsigned levels = raw[6] | raw[7] << 8;
  EXPECT(levels >= 1 && levels <= 8, "the zoom level count");
  for (unsigned l = 0; l < levels; l++) {
    const uint64_t zd = rd64(raw + 64 + 24 * l + 8), zi = rd64(raw + 64 + 24 * l + 16);
    EXPECT(zd < zi && zi + 48 <= (uint64_t)end && rd32(raw + zi) == 0x2468ACE0u, "a zoom level's offsets");
  }
  for (uint32_t k = 0; k < n_refs; k++) free(names[k]);
  free(names);
  free(lens);
  return raw;
}

static int open_ro(const char *path) { return open(path, O_RDONLY); }

int main(void) {
  static const uint64_t section_counts[] = {0, 1, 256, 257, 65537};
  static const uint32_t contig_counts[] = {1, 2, 256, 257, 300};
  size_t len = 0;
  for (int a = 0; a < 5; a++) { /* S = 1: a section per site */
    const uint32_t tid = 0;
    free(one_file(2, 1, 4, &tid, &section_counts[a], 1, &len, "section counts"));
  }
  for (int a = 0; a < 5; a++) { /* a block on the first, the middle and the last contig */
    const uint32_t n = contig_counts[a], tids[3] = {0, n / 2, n - 1};
    const uint64_t sites[3] = {5, 700, 1};
    free(one_file(n, 3, 16, tids, sites, n == 1 ? 1 : (n == 2 ? 2 : 3), &len, "contig counts"));
  }
  { /* several blocks on one contig, a window two blocks share, eight levels */
    const uint32_t tids[4] = {1, 1, 1, 2};
    const uint64_t sites[4] = {1000, 1, 70000, 3000};
    uint8_t *raw = one_file(3, 1024, 1, tids, sites, 4, &len, "blocks");
    EXPECT((raw[6] | raw[7] << 8) >= 4, "several zoom levels");
    free(raw);
  }
  free(one_file(0, 1024, 1024, NULL, NULL, 0, &len, "no contig at all"));
  /* refusals: each leaves the writer usable */
  {
    char path[] = "/tmp/bigwig_san_XXXXXX";
    const int fd = mkstemp(path);
    const char *names[2] = {"b", "a"};
    const uint32_t lens[2] = {1000, 1000};
    bsc_bw_params bp = {2, 10};
    bsc_bigwig *bw = NULL;
    bsc_bw_params bad = {0, 10};
    EXPECT(bsc_bigwig_open(fd, 2, names, lens, &bad, &bw) == BSC_ERR_ARG && !bw, "items_per_section = 0");
    bad.items_per_section = 65536;
    EXPECT(bsc_bigwig_open(fd, 2, names, lens, &bad, &bw) == BSC_ERR_ARG && !bw, "items_per_section = 65536");
    bad.items_per_section = 1, bad.reduction = 0;
    EXPECT(bsc_bigwig_open(fd, 2, names, lens, &bad, &bw) == BSC_ERR_ARG && !bw, "reduction = 0");
    EXPECT(bsc_bigwig_open(fd, 2, names, lens, &bp, &bw) == BSC_OK && bw, "open");
    uint8_t data[24 + 16 + 24 + 8] = {0};
    const bsc_bw_sum sec[2] = {{100, 103, 2, 0, 5, 0, 5, 25}, {105, 106, 1, 7, 7, 0, 7, 49}};
    const bsc_bw_sum zoom[1] = {{100, 106, 3, 0, 7, 0, 12, 74}};
    EXPECT(bsc_bigwig_add(bw, 2, data, sizeof data, sec, 2, zoom, 1) == BSC_ERR_ARG, "a contig beyond the header");
    EXPECT(bsc_bigwig_add(bw, 1, data, sizeof data - 8, sec, 2, zoom, 1) == BSC_ERR_ARG, "bytes that are not the sections'");
    EXPECT(bsc_bigwig_add(bw, 1, data, sizeof data, sec, 2, zoom, 1) == BSC_OK, "a good block");
    EXPECT(bsc_bigwig_add(bw, 0, data, sizeof data, sec, 2, zoom, 1) == BSC_ERR_ARG, "a contig behind the last");
    EXPECT(bsc_bigwig_add(bw, 1, data, sizeof data, sec, 2, zoom, 1) == BSC_ERR_ARG, "a start below the previous end");
    const bsc_bw_sum sec2[1] = {{106, 107, 1, 1, 1, 0, 1, 1}};
    EXPECT(bsc_bigwig_add(bw, 1, data, 32, sec2, 1, sec2, 1) == BSC_OK, "a start at the previous end");
    EXPECT(bsc_bigwig_add(bw, 1, NULL, 0, NULL, 0, NULL, 0) == BSC_OK, "an empty block");
    EXPECT(bsc_bigwig_finish(bw) == BSC_OK, "finish");
    EXPECT(bsc_bigwig_add(bw, 1, NULL, 0, NULL, 0, NULL, 0) == BSC_ERR_ARG, "add behind finish");
    bsc_bigwig_close(bw);
    close(fd);
    /* a descriptor that cannot be written to: the failure is reported */
    const int ro = open_ro(path);
    bw = NULL;
    EXPECT(bsc_bigwig_open(ro, 2, names, lens, &bp, &bw) == BSC_OK && bw, "open on a read-only descriptor");
    EXPECT(bsc_bigwig_add(bw, 1, data, sizeof data, sec, 2, zoom, 1) == BSC_ERR_ARG && strstr(errbuf, "write failed"), "a failed data write");
    EXPECT(bsc_bigwig_finish(bw) == BSC_ERR_ARG && strstr(errbuf, "write failed"), "a failed finish");
    bsc_bigwig_close(bw);
    close(ro);
    unlink(path);
    bsc_bigwig_close(NULL);
  }
  if (failures) return 1;
  puts("ok");
  return 0;
}
