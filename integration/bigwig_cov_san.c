/*
 * bigwig_cov_san.c — the COVERAGE track's host code (csrc/bigwig.c: bsc_bigwig_cov_sections_recs, bsc_bigwig_open_track and a coverage
 * writer's bsc_bigwig_add / _add_z / _finish) as a stand-alone program for the address and undefined-behaviour sanitizers: `make
 * bigwig-cov-san` compiles this file and csrc/bigwig.c with -fsanitize=address,undefined and -lz — no device, no library.  The host form
 * writes into heap blocks of exactly the bytes it asked for, with each room one short; the value floats at the ties around 2^24 and 2^32;
 * sums of squares beyond 2^64 in a section, in a window two adds share and in the total; plain and compressed files of 0, 1, 256 and 257
 * sections over 1, 2 and 300 contigs, read back by their own offsets; the refusals.  Prints "ok" and returns 0, or names the case.
 */
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

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
#define EXPECT(cond, what)                                                           \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      fprintf(stderr, "bigwig_cov_san: %s (line %d): %s\n", what, __LINE__, errbuf); \
      failures++;                                                                    \
    }                                                                                \
  } while (0)

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }
static float rdf32(const uint8_t *p) {
  const uint32_t v = rd32(p);
  float f;
  memcpy(&f, &v, 4);
  return f;
}
static double rdf64(const uint8_t *p) {
  const uint64_t v = rd64(p);
  double d;
  memcpy(&d, &v, 8);
  return d;
}

/* n sites at starts first, first + step, ..: a = b = half (the coverage is 2 * half, saturated) */
static bsc_vcf_rec *make_recs(uint64_t n, uint32_t first, uint32_t step, uint32_t half) {
  bsc_vcf_rec *r = calloc(n ? n : 1, sizeof *r);
  for (uint64_t i = 0; i < n; i++) {
    r[i].core.pos = first + 1u + (uint32_t)i * step;
    r[i].core.emit = 1;
    r[i].core.gt = i % 3 ? 4 : 7;
    r[i].core.cg = 'C';
    r[i].counts[5] = r[i].counts[6] = half ? half : (uint32_t)(i % 7);
    r[i].counts[7] = r[i].counts[4] = half ? half : (uint32_t)(1 + i % 5);
  }
  return r;
}

typedef struct {
  uint8_t *data;
  bsc_bw_sum *sec, *zoom;
  uint64_t nb, ns, nz;
} block;

/* the host form into heap blocks of exactly the sizes it reports; each room one short is refused with nothing written */
static block host_form(const bsc_vcf_rec *recs, uint64_t n, uint32_t tid, const bsc_bw_params *bp) {
  bsc_meth_params mp;
  memset(&mp, 0, sizeof mp);
  mp.min_cov = 1;
  block b;
  memset(&b, 0, sizeof b);
  bsc_bigwig_cov_sections_recs(recs, n, tid, &mp, bp, NULL, 0, &b.nb, NULL, &b.ns, NULL, &b.nz);
  b.data = malloc(b.nb ? b.nb : 1);
  b.sec = malloc((b.ns ? b.ns : 1) * sizeof *b.sec);
  b.zoom = malloc((b.nz ? b.nz : 1) * sizeof *b.zoom);
  for (int k = 0; k < 3 && b.nb; k++) {
    uint64_t nb = 0, ns = b.ns - (k == 1), nz = b.nz - (k == 2);
    memset(b.data, 0x5A, b.nb);
    EXPECT(bsc_bigwig_cov_sections_recs(recs, n, tid, &mp, bp, b.data, b.nb - (k == 0), &nb, b.sec, &ns, b.zoom, &nz) == BSC_ERR_ARG, "a room one short");
    EXPECT(nb == b.nb && ns == b.ns && nz == b.nz && b.data[0] == 0x5A, "the needs reported, nothing written");
  }
  uint64_t nb = 0, ns = b.ns, nz = b.nz;
  EXPECT(bsc_bigwig_cov_sections_recs(recs, n, tid, &mp, bp, b.data, b.nb, &nb, b.sec, &ns, b.zoom, &nz) == BSC_OK, "the host form");
  EXPECT(nb == b.nb && ns == b.ns && nz == b.nz, "the host form's counts");
  return b;
}
static void block_free(block *b) {
  free(b->data);
  free(b->sec);
  free(b->zoom);
}

static uint8_t *slurp(const char *path, uint64_t *n) {
  struct stat st;
  if (stat(path, &st)) return NULL;
  uint8_t *raw = malloc((size_t)st.st_size ? (size_t)st.st_size : 1);
  FILE *f = fopen(path, "rb");
  *n = f ? fread(raw, 1, (size_t)st.st_size, f) : 0;
  if (f) fclose(f);
  return raw;
}

/* one coverage file of n_refs contigs: blocks of (tid, sites); z: compressed.  Checked by its own offsets. */
static void one_file(uint32_t n_refs, uint32_t S, uint32_t red, const uint32_t *tids, const uint64_t *sites, int n_blocks, int z, unsigned want_levels,
                     const char *what) {
  char path[] = "/tmp/bigwig_cov_san_XXXXXX";
  const int fd = mkstemp(path);
  EXPECT(fd >= 0, "mkstemp");
  char **names = calloc(n_refs ? n_refs : 1, sizeof *names);
  uint32_t *lens = calloc(n_refs ? n_refs : 1, sizeof *lens);
  for (uint32_t k = 0; k < n_refs; k++) {
    names[k] = malloc(32);
    snprintf(names[k], 32, "c%u%s", (n_refs - k) * 7u % 1000u, k % 3 ? "_long_name" : "");
    lens[k] = 4000000u;
  }
  const bsc_bw_params bp = {S, red};
  bsc_bigwig *bw = NULL;
  EXPECT(bsc_bigwig_open_track(fd, n_refs, (const char *const *)names, lens, &bp, BSC_BW_COVERAGE, &bw) == BSC_OK && bw, what);
  uint64_t total_sec = 0, total_sites = 0;
  unsigned __int128 sum = 0, sum2 = 0;
  uint64_t min_c = ~0ull, max_c = 0;
  uint32_t next_start = 0, last_tid = 0;
  for (int k = 0; k < n_blocks && bw; k++) {
    if (k && tids[k] != last_tid) next_start = 0;
    last_tid = tids[k];
    bsc_vcf_rec *recs = make_recs(sites[k], next_start, 3, 0);
    block b = host_form(recs, sites[k], tids[k], &bp);
    for (uint64_t i = 0; i < sites[k]; i++) {
      const uint64_t c = (uint64_t)(i % 7) + 1 + i % 5;
      sum += c;
      sum2 += c * c;
      if (c < min_c) min_c = c;
      if (c > max_c) max_c = c;
    }
    if (z) {
      const uint64_t piece = 24 + 8 * (uint64_t)S;
      uint8_t *zdata = malloc(b.nb + 64 * b.ns + 1);
      uint32_t *zs = malloc((b.ns ? b.ns : 1) * sizeof *zs);
      uint64_t zn = 0;
      for (uint64_t s = 0; s < b.ns; s++) {
        const uint64_t len = s + 1 < b.ns ? piece : b.nb - s * piece;
        uLongf n = (uLongf)(len + 64);
        EXPECT(compress2(zdata + zn, &n, b.data + s * piece, (uLong)len, 1) == Z_OK, "compress2");
        zs[s] = (uint32_t)n;
        zn += n;
      }
      EXPECT(bsc_bigwig_add_z(bw, tids[k], zdata, zn, zs, b.sec, b.ns, b.zoom, b.nz) == BSC_OK, what);
      free(zdata);
      free(zs);
    } else {
      EXPECT(bsc_bigwig_add(bw, tids[k], b.data, b.nb, b.sec, b.ns, b.zoom, b.nz) == BSC_OK, what);
    }
    total_sec += b.ns;
    total_sites += sites[k];
    next_start += (uint32_t)sites[k] * 3u;
    block_free(&b);
    free(recs);
  }
  EXPECT(bsc_bigwig_finish(bw) == BSC_OK, what);
  EXPECT(bsc_bigwig_finish(bw) == BSC_ERR_ARG, "finish twice");
  bsc_bigwig_close(bw);
  close(fd);
  uint64_t n = 0;
  uint8_t *raw = slurp(path, &n);
  EXPECT(raw && n >= 300 && rd32(raw) == 0x888FFC26u && rd32(raw + n - 4) == 0x888FFC26u, "the magics");
  if (raw && n >= 300) {
    EXPECT((raw[6] | raw[7] << 8) == (int)want_levels, "the zoom level count");
    EXPECT(rd64(raw + rd64(raw + 16)) == total_sec, "the section count");
    EXPECT((rd32(raw + 52) != 0) == (z && total_sec), "uncompressBufSize");
    EXPECT(rd64(raw + 256) == total_sites, "basesCovered");
    if (total_sites) {
      EXPECT(rdf64(raw + 264) == (double)min_c && rdf64(raw + 272) == (double)max_c, "minVal / maxVal of the total");
      EXPECT(rdf64(raw + 280) == (double)(uint64_t)sum && rdf64(raw + 288) == (double)(uint64_t)sum2, "sumData / sumSquares of the total");
    }
  }
  free(raw);
  unlink(path);
  for (uint32_t k = 0; k < n_refs; k++) free(names[k]);
  free(names);
  free(lens);
}

/* the value floats: c -> the float the rule names, at the ties */
static void value_floats(void) {
  static const struct {
    uint64_t ab;
    uint32_t bits;
  } T[] = {{1, 0x3F800000u},          {(1u << 24) - 1, 0x4B7FFFFFu},   {1u << 24, 0x4B800000u},       {(1u << 24) + 1, 0x4B800000u},
           {(1u << 24) + 3, 0x4B800002u}, {(1u << 25) + 2, 0x4C000000u}, {(1u << 25) + 6, 0x4C000002u}, {1u << 31, 0x4F000000u},
           {0xFFFFFF7Full, 0x4F7FFFFFu},  {0xFFFFFF80ull, 0x4F800000u},  {0xFFFFFFFFull, 0x4F800000u},  {0x100000000ull, 0x4F800000u},
           {0x1FFFFFFFEull, 0x4F800000u}};
  const bsc_bw_params bp = {1024, 1024};
  const size_t n = sizeof T / sizeof T[0];
  bsc_vcf_rec *recs = make_recs(n, 10, 1, 1);
  for (size_t i = 0; i < n; i++) {
    const uint32_t a = (uint32_t)(T[i].ab / 2), b = (uint32_t)(T[i].ab - a);
    recs[i].counts[5] = recs[i].counts[6] = a;
    recs[i].counts[7] = recs[i].counts[4] = b;
  }
  block b = host_form(recs, n, 0, &bp);
  EXPECT(b.ns == 1 && b.nb == 24 + 8 * n, "one section");
  for (size_t i = 0; i < n && b.nb == 24 + 8 * n; i++) {
    EXPECT(rd32(b.data + 24 + 8 * i + 4) == T[i].bits, "a value float");
    const uint32_t c = T[i].ab > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)T[i].ab;
    const float f = (float)c;
    EXPECT(!memcmp(&f, b.data + 24 + 8 * i + 4, 4), "a value float is C's conversion");
  }
  EXPECT(b.sec[0].min_m == 1 && b.sec[0].max_m == 0xFFFFFFFFu, "min / max");
  block_free(&b);
  free(recs);
}

/* sums of squares beyond 2^64: in a section, in a window two adds share, in the total; sums whose f32 differs once / through a double */
static void wide_sums(void) {
  char path[] = "/tmp/bigwig_cov_san_XXXXXX";
  const int fd = mkstemp(path);
  const char *names[] = {"chr1"};
  const uint32_t lens[] = {100000};
  const bsc_bw_params bp = {64, 1000};
  bsc_bigwig *bw = NULL;
  EXPECT(bsc_bigwig_open_track(fd, 1, names, lens, &bp, BSC_BW_COVERAGE, &bw) == BSC_OK, "open");
  const unsigned __int128 top = 0xFFFFFFFFull, sq = top * top;
  uint32_t at = 0;
  for (int k = 0; k < 2; k++) { /* two adds of 70 sites of c = 2^32 - 1 in ONE window of 1000 */
    bsc_vcf_rec *recs = make_recs(70, at, 1, 0xFFFFFFFFu);
    block b = host_form(recs, 70, 0, &bp);
    EXPECT(b.ns == 2 && b.nz == 1, "two sections, one window");
    EXPECT(b.sec[0]._pad == (uint32_t)((64 * sq) >> 64) && b.sec[0].sum_m2 == (uint64_t)(64 * sq) && b.sec[0]._pad > 0, "a section's 96-bit sum");
    EXPECT(b.zoom[0]._pad == (uint32_t)((70 * sq) >> 64) && b.zoom[0].sum_m2 == (uint64_t)(70 * sq) && b.zoom[0].sum_m == 70 * 0xFFFFFFFFull, "a window's sums");
    EXPECT(bsc_bigwig_add(bw, 0, b.data, b.nb, b.sec, b.ns, b.zoom, b.nz) == BSC_OK, "add");
    at += 70;
    block_free(&b);
    free(recs);
  }
  EXPECT(bsc_bigwig_finish(bw) == BSC_OK, "finish");
  bsc_bigwig_close(bw);
  close(fd);
  uint64_t n = 0;
  uint8_t *raw = slurp(path, &n);
  EXPECT(raw && n > 400, "the file");
  if (raw && n > 400) {
    /* 140 c^2 = 140 2^64 - 140 2^33 + 140: the last term is far below half a double's step there (2^18), and below half a float's (2^47)
     * with the middle one */
    EXPECT(rdf64(raw + 288) == 140.0 * (0x1p64 - 0x1p33), "sumSquares of the total beyond 2^64");
    EXPECT(rdf64(raw + 280) == 140.0 * 4294967295.0 && rdf64(raw + 264) == 4294967295.0, "sumData / minVal of the total");
    const uint64_t z0 = rd64(raw + 64 + 8); /* level 0's data: recordCount, then one record */
    EXPECT(rd32(raw + z0) == 1 && rd32(raw + z0 + 4 + 12) == 140, "the shared window is one record of 140 sites");
    EXPECT(rdf32(raw + z0 + 4 + 28) == 140.0f * 0x1p64f, "its sumSquares");
  }
  free(raw);
  unlink(path);
}

/* a window whose sum's f32 differs between "once" and "through a double": 2^60 + 2^36 + 1 lies just above the tie 2^60 + 2^36 of two
 * neighbouring floats (2^60 and 2^60 + 2^37) and rounds UP; its double is the tie itself (the 1 is below the double's last bit), which the
 * second rounding sends DOWN, to even. */
static void once_not_twice(void) {
  char path[] = "/tmp/bigwig_cov_san_XXXXXX";
  const int fd = mkstemp(path);
  const char *names[] = {"chr1"};
  const uint32_t lens[] = {100000};
  const bsc_bw_params bp = {4, 1000};
  bsc_bigwig *bw = NULL;
  EXPECT(bsc_bigwig_open_track(fd, 1, names, lens, &bp, BSC_BW_COVERAGE, &bw) == BSC_OK, "open");
  bsc_bw_sum s;
  memset(&s, 0, sizeof s);
  s.start = 5;
  s.end = 6;
  s.count = 1;
  s.min_m = s.max_m = 7;
  s.sum_m = (1ull << 60) + (1ull << 36) + 1;
  s.sum_m2 = 49;
  const uint8_t data[32] = {0};
  EXPECT(bsc_bigwig_add(bw, 0, data, 32, &s, 1, &s, 1) == BSC_OK, "add");
  EXPECT(bsc_bigwig_finish(bw) == BSC_OK, "finish");
  bsc_bigwig_close(bw);
  close(fd);
  uint64_t n = 0;
  uint8_t *raw = slurp(path, &n);
  if (raw && n > 400) {
    const uint64_t z0 = rd64(raw + 64 + 8);
    const float once = rdf32(raw + z0 + 4 + 24), twice = (float)(double)s.sum_m;
    EXPECT(once == 0x1.000002p60f && twice == 0x1p60f, "sumData is rounded once from the integer");
  } else {
    EXPECT(0, "the file");
  }
  free(raw);
  unlink(path);
}

static void refusals(void) {
  char path[] = "/tmp/bigwig_cov_san_XXXXXX";
  const int fd = mkstemp(path);
  const char *names[] = {"chr1", "chr2"};
  const uint32_t lens[] = {1000, 1000};
  const bsc_bw_params bp = {4, 10}, bad = {0, 10};
  bsc_bigwig *bw = NULL;
  EXPECT(bsc_bigwig_open_track(fd, 2, names, lens, &bp, 0, &bw) == BSC_ERR_ARG && !bw, "track 0");
  EXPECT(bsc_bigwig_open_track(fd, 2, names, lens, &bp, 3, &bw) == BSC_ERR_ARG && !bw, "track 3");
  EXPECT(bsc_bigwig_open_track(fd, 2, names, lens, &bad, BSC_BW_COVERAGE, &bw) == BSC_ERR_ARG && !bw, "S = 0");
  EXPECT(bsc_bigwig_open_track(-1, 2, names, lens, &bp, BSC_BW_COVERAGE, &bw) == BSC_ERR_ARG && !bw, "fd < 0");
  EXPECT(bsc_bigwig_open_track(fd, 2, names, lens, &bp, BSC_BW_COVERAGE, &bw) == BSC_OK && bw, "open");
  bsc_vcf_rec *recs = make_recs(6, 20, 2, 0);
  block b = host_form(recs, 6, 1, &bp);
  EXPECT(bsc_bigwig_add(bw, 1, b.data, b.nb, b.sec, b.ns, b.zoom, b.nz) == BSC_OK, "add");
  struct stat st0, st1;
  fstat(fd, &st0);
  EXPECT(bsc_bigwig_add(bw, 0, b.data, b.nb, b.sec, b.ns, b.zoom, b.nz) == BSC_ERR_ARG, "a lower contig");
  EXPECT(bsc_bigwig_add(bw, 2, b.data, b.nb, b.sec, b.ns, b.zoom, b.nz) == BSC_ERR_ARG, "a contig not in the header");
  EXPECT(bsc_bigwig_add(bw, 1, b.data, b.nb, b.sec, b.ns, b.zoom, b.nz) == BSC_ERR_ARG, "a start below the previous end");
  EXPECT(bsc_bigwig_add(bw, 1, b.data, b.nb - 8, b.sec, b.ns, b.zoom, b.nz) == BSC_ERR_ARG, "bytes the entries do not describe");
  EXPECT(bsc_bigwig_add(bw, 1, b.data, b.nb, b.sec, b.ns, NULL, 0) == BSC_ERR_ARG, "sections without a window");
  const uint32_t zs[2] = {40, 30};
  EXPECT(bsc_bigwig_add_z(bw, 1, b.data, 70, zs, b.sec, b.ns, b.zoom, b.nz) == BSC_ERR_ARG, "add_z into a plain file");
  fstat(fd, &st1);
  EXPECT(st0.st_size == st1.st_size, "a refusal writes nothing");
  EXPECT(bsc_bigwig_finish(bw) == BSC_OK, "finish");
  EXPECT(bsc_bigwig_add(bw, 1, NULL, 0, NULL, 0, NULL, 0) == BSC_ERR_ARG, "add behind finish");
  bsc_bigwig_close(bw);
  bsc_bigwig_close(NULL);
  block_free(&b);
  free(recs);
  close(fd);
  unlink(path);
}

int main(void) {
  value_floats();
  wide_sums();
  once_not_twice();
  {
    const uint32_t t1[] = {0};
    const uint64_t none[] = {0}, one[] = {1}, s256[] = {256}, s257[] = {257};
    for (int z = 0; z < 2; z++) {
      one_file(1, 1, 1024, t1, none, 1, z, 1, "no section");
      one_file(1, 1024, 1024, t1, one, 1, z, 1, "one section");
      one_file(1, 1, 1024, t1, s256, 1, z, 1, "256 sections");
      one_file(1, 1, 1, t1, s257, 1, z, 2, "257 sections, two levels");
      const uint32_t t2[] = {0, 1, 1};
      const uint64_t s2[] = {700, 600, 5};
      one_file(2, 64, 1, t2, s2, 3, z, 3, "two contigs, three levels");
      const uint32_t t300[] = {0, 7, 299};
      const uint64_t s300[] = {10, 300, 2500};
      one_file(300, 1024, 64, t300, s300, 3, z, 1, "300 contigs");
      const uint32_t t8[] = {0};
      const uint64_t s8[] = {70000};
      one_file(1, 1024, 1, t8, s8, 1, z, 6, "six levels");
    }
  }
  refusals();
  if (failures) return 1;
  puts("ok");
  return 0;
}
