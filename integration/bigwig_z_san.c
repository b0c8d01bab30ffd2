/*
 * bigwig_z_san.c — the COMPRESSED writer of the methylation bigWig file (csrc/bigwig.c: bsc_bigwig_add_z, and bsc_bigwig_finish deflating
 * the zoom blocks with libz) as a stand-alone program for the address and undefined-behaviour sanitizers: `make bigwig-z-san` compiles this
 * file and csrc/bigwig.c with -fsanitize=address,undefined and -lz — no device, no library.  The section streams are libz's here (compress2);
 * the program writes files of 1, 256, 257 and 65 537 sections, 1, 2 and 257 contigs, 1 to 8 zoom levels, a window two blocks share and zoom
 * blocks cut at a contig's end, walks every R-tree of the file by its own offsets, inflates every leaf's bytes (uncompress) into a buffer of
 * uncompressBufSize bytes and compares the sections with the plain stream; then the refusals.  Prints "ok" and returns 0, or names the case.
 */
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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
#define EXPECT(cond, what)                                                         \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      fprintf(stderr, "bigwig_z_san: %s (line %d): %s\n", what, __LINE__, errbuf); \
      failures++;                                                                  \
    }                                                                              \
  } while (0)

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

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

/* the leaves of the R-tree at `at`, in order: each inflated into buf[room]; want != NULL: the inflated bytes, one behind the other, are
 * want[0 .. want_n).  Returns the leaves seen. */
typedef struct {
  const uint8_t *raw;
  uint64_t end;
  uint8_t *buf;
  uint32_t room;
  const uint8_t *want;
  uint64_t want_n, want_at, leaves, largest;
} walk;
static void walk_node(walk *w, uint64_t at) {
  EXPECT(at + 4 <= w->end, "a node inside the file");
  if (at + 4 > w->end) return;
  const int leaf = w->raw[at];
  const unsigned count = w->raw[at + 2] | w->raw[at + 3] << 8;
  EXPECT(at + 4 + (uint64_t)count * (leaf ? 32 : 24) <= w->end, "a node's items inside the file");
  for (unsigned k = 0; k < count; k++) {
    const uint8_t *it = w->raw + at + 4 + (uint64_t)k * (leaf ? 32 : 24);
    if (!leaf) {
      walk_node(w, rd64(it + 16));
      continue;
    }
    const uint64_t off = rd64(it + 16), size = rd64(it + 24);
    EXPECT(off + size <= w->end && size >= 1, "a leaf's bytes inside the file");
    uLongf n = w->room;
    EXPECT(uncompress(w->buf, &n, w->raw + off, (uLong)size) == Z_OK, "a leaf's bytes inflate into uncompressBufSize bytes");
    if (n > w->largest) w->largest = n;
    if (w->want) {
      EXPECT(w->want_at + n <= w->want_n && !memcmp(w->buf, w->want + w->want_at, n), "a section inflates to the plain stream's bytes");
      w->want_at += n;
    }
    w->leaves++;
  }
}

/* one compressed file: n_refs contigs, the given blocks of (tid, n_sites); returns the zoom level count */
static unsigned one_file(uint32_t n_refs, uint32_t S, uint32_t red, const uint32_t *tids, const uint64_t *sites, int n_blocks, const char *what) {
  char path[] = "/tmp/bigwig_z_san_XXXXXX";
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
  bsc_meth_params mp;
  memset(&mp, 0, sizeof mp);
  mp.min_cov = 1;
  bsc_bigwig *bw = NULL;
  EXPECT(bsc_bigwig_open(fd, n_refs, (const char *const *)names, lens, &bp, &bw) == BSC_OK && bw, what);
  uint64_t total_sec = 0, plain_n = 0, plain_cap = 0;
  uint8_t *plain = NULL; /* every block's plain stream, one behind the other */
  uint32_t next_start = 0, last_tid = 0;
  const uint64_t piece = 24 + 8 * (uint64_t)S;
  for (int b = 0; b < n_blocks && bw; b++) {
    if (b && tids[b] != last_tid) next_start = 0;
    last_tid = tids[b];
    bsc_vcf_rec *recs = make_recs(sites[b], next_start, 3);
    uint64_t nb = 0, ns = 0, nz = 0;
    bsc_bigwig_sections_recs(recs, sites[b], tids[b], &mp, &bp, NULL, 0, &nb, NULL, &ns, NULL, &nz);
    uint8_t *data = malloc(nb ? nb : 1), *zdata = malloc(nb + 64 * ns + 1);
    uint32_t *zs = malloc((ns ? ns : 1) * sizeof *zs);
    bsc_bw_sum *sec = malloc((ns ? ns : 1) * sizeof *sec), *zoom = malloc((nz ? nz : 1) * sizeof *zoom);
    EXPECT(bsc_bigwig_sections_recs(recs, sites[b], tids[b], &mp, &bp, data, nb, &nb, sec, &ns, zoom, &nz) == BSC_OK, "the host form");
    uint64_t zn = 0;
    for (uint64_t k = 0; k < ns; k++) { /* every section through libz at level 1; where that grows it beyond raw + 11, stored (level 0) */
      const uint64_t at = k * piece, len = nb - at < piece ? nb - at : piece;
      uLongf n = (uLongf)(len + 64);
      EXPECT(compress2(zdata + zn, &n, data + at, (uLong)len, 1) == Z_OK, "compress2");
      if (n > len + 11) {
        n = (uLongf)(len + 64);
        EXPECT(compress2(zdata + zn, &n, data + at, (uLong)len, 0) == Z_OK && n == len + 11, "compress2, stored");
      }
      zs[k] = (uint32_t)n;
      zn += n;
    }
    EXPECT(bsc_bigwig_add_z(bw, tids[b], zdata, zn, zs, sec, ns, zoom, nz) == BSC_OK, what);
    if (plain_n + nb > plain_cap) {
      plain_cap = (plain_n + nb) * 2 + 64;
      plain = realloc(plain, plain_cap);
    }
    if (nb) memcpy(plain + plain_n, data, nb);
    plain_n += nb;
    total_sec += ns;
    next_start += (uint32_t)sites[b] * 3u;
    free(recs);
    free(data);
    free(zdata);
    free(zs);
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
  EXPECT(end >= 300 && rd32(raw) == 0x888FFC26u && rd32(raw + end - 4) == 0x888FFC26u, "the two magics");
  const uint64_t data_at = rd64(raw + 16), index_at = rd64(raw + 24);
  const uint32_t room = rd32(raw + 52);
  const unsigned levels = raw[6] | raw[7] << 8;
  EXPECT(data_at < (uint64_t)end && rd64(raw + data_at) == total_sec, "the section count");
  EXPECT(index_at + 48 <= (uint64_t)end && rd32(raw + index_at) == 0x2468ACE0u && rd64(raw + index_at + 8) == total_sec, "the R-tree's header");
  EXPECT(total_sec ? room >= 32 : room == 0, "uncompressBufSize");
  uint8_t *buf = malloc(room ? room : 1); /* exactly the room the header promises: the sanitizer sees a byte beyond it */
  walk w = {raw, (uint64_t)end, buf, room, plain, plain_n, 0, 0, 0};
  walk_node(&w, index_at + 48);
  EXPECT(w.leaves == total_sec && w.want_at == plain_n, "every section, once");
  EXPECT(levels >= 1 && levels <= 8, "the zoom level count");
  for (unsigned l = 0; l < levels; l++) {
    const uint64_t zd = rd64(raw + 64 + 24 * l + 8), zi = rd64(raw + 64 + 24 * l + 16);
    EXPECT(zd < zi && zi + 48 <= (uint64_t)end && rd32(raw + zi) == 0x2468ACE0u, "a zoom level's offsets");
    walk z = {raw, (uint64_t)end, buf, room, NULL, 0, 0, 0, w.largest};
    const uint64_t before = z.leaves;
    walk_node(&z, zi + 48);
    EXPECT(z.leaves - before == rd64(raw + zi + 8), "every zoom block, once");
    w.largest = z.largest;
  }
  EXPECT(w.largest == room, "uncompressBufSize is the largest raw block");
  free(buf);
  free(raw);
  free(plain);
  for (uint32_t k = 0; k < n_refs; k++) free(names[k]);
  free(names);
  free(lens);
  return levels;
}

int main(void) {
  static const uint64_t section_counts[] = {1, 256, 257, 65537};
  static const uint32_t contig_counts[] = {1, 2, 257};
  for (int a = 0; a < 4; a++) { /* S = 1: a section per site */
    const uint32_t tid = 0;
    one_file(2, 1, 4, &tid, &section_counts[a], 1, "section counts");
  }
  for (int a = 0; a < 3; a++) { /* a block on the first, the middle and the last contig; 700 sites 3 apart at reduction 1: zoom blocks of 512 + 188 records */
    const uint32_t n = contig_counts[a], tids[3] = {0, n / 2, n - 1};
    const uint64_t sites[3] = {600, 700, 1};
    const unsigned levels = one_file(n, 3, 1, tids, sites, n == 1 ? 1 : (n == 2 ? 2 : 3), "contig counts");
    EXPECT(levels >= 2, "more than one zoom level");
  }
  { /* several blocks on one contig, a window two blocks share, eight levels */
    const uint32_t tids[4] = {1, 1, 1, 2};
    const uint64_t sites[4] = {1000, 1, 70000, 3000};
    EXPECT(one_file(3, 1024, 1, tids, sites, 4, "blocks") >= 4, "several zoom levels");
    const uint64_t many = 400000;
    const uint32_t tid = 0;
    EXPECT(one_file(1, 8157, 1, &tid, &many, 1, "eight levels") == 8, "eight zoom levels");
    const uint64_t one = 1;
    EXPECT(one_file(1, 1024, 1024, &tid, &one, 1, "one level") == 1, "one zoom level");
  }
  EXPECT(one_file(0, 1024, 1024, NULL, NULL, 0, "no contig at all") == 1, "no contig at all");
  /* refusals: each leaves the writer usable and the file as it was */
  {
    char path[] = "/tmp/bigwig_z_san_XXXXXX";
    const int fd = mkstemp(path);
    const char *names[2] = {"b", "a"};
    const uint32_t lens[2] = {1000, 1000};
    const bsc_bw_params bp = {2, 10};
    bsc_bigwig *bw = NULL;
    EXPECT(bsc_bigwig_open(fd, 2, names, lens, &bp, &bw) == BSC_OK && bw, "open");
    uint8_t data[24 + 16 + 24 + 8] = {0}, z[2 * (40 + 11)];
    memset(z, 0x5a, sizeof z);
    const bsc_bw_sum sec[2] = {{100, 103, 2, 0, 5, 0, 5, 25}, {105, 106, 1, 7, 7, 0, 7, 49}};
    const bsc_bw_sum zoom[1] = {{100, 106, 3, 0, 7, 0, 12, 74}};
    uint32_t zs[2] = {30, 20};
    EXPECT(bsc_bigwig_add_z(bw, 1, NULL, 0, NULL, NULL, 0, NULL, 0) == BSC_OK, "an empty block decides nothing");
    EXPECT(bsc_bigwig_add(bw, 1, NULL, 0, NULL, 0, NULL, 0) == BSC_OK, "an empty block decides nothing");
    EXPECT(bsc_bigwig_add_z(bw, 2, z, 50, zs, sec, 2, zoom, 1) == BSC_ERR_ARG, "a contig beyond the header");
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 51, zs, sec, 2, zoom, 1) == BSC_ERR_ARG && strstr(errbuf, "add up"), "sizes that do not add up to z_bytes");
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 50, NULL, sec, 2, zoom, 1) == BSC_ERR_ARG, "no sizes");
    zs[1] = 0;
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 30, zs, sec, 2, zoom, 1) == BSC_ERR_ARG && strstr(errbuf, "stream of"), "a size of 0");
    zs[1] = 24 + 8 + 12;
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 30 + 44, zs, sec, 2, zoom, 1) == BSC_ERR_ARG && strstr(errbuf, "stream of"), "a size above raw + 11");
    EXPECT(lseek(fd, 0, SEEK_END) == 0, "nothing written by a refused call");
    zs[1] = 24 + 8 + 11;
    zs[0] = 1;
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 1 + 43, zs, sec, 2, zoom, 1) == BSC_OK, "sizes of 1 and raw + 11");
    const off_t size1 = lseek(fd, 0, SEEK_END);
    EXPECT(bsc_bigwig_add(bw, 1, data, 32, sec + 1, 1, sec + 1, 1) == BSC_ERR_ARG && strstr(errbuf, "compressed"), "a plain add to a compressed file");
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 44, zs, sec, 2, zoom, 1) == BSC_ERR_ARG, "a start below the previous end");
    EXPECT(bsc_bigwig_add_z(bw, 0, z, 44, zs, sec, 2, zoom, 1) == BSC_ERR_ARG, "a contig behind the last");
    EXPECT(lseek(fd, 0, SEEK_END) == size1, "nothing written by a refused call");
    EXPECT(bsc_bigwig_finish(bw) == BSC_OK, "finish");
    EXPECT(bsc_bigwig_add_z(bw, 1, NULL, 0, NULL, NULL, 0, NULL, 0) == BSC_ERR_ARG, "add behind finish");
    bsc_bigwig_close(bw);
    /* the reverse: a compressed add to a plain file */
    bw = NULL;
    EXPECT(ftruncate(fd, 0) == 0, "truncate");
    EXPECT(bsc_bigwig_open(fd, 2, names, lens, &bp, &bw) == BSC_OK && bw, "open");
    EXPECT(bsc_bigwig_add(bw, 1, data, sizeof data, sec, 2, zoom, 1) == BSC_OK, "a plain block");
    const off_t size2 = lseek(fd, 0, SEEK_END);
    const bsc_bw_sum sec2[1] = {{106, 107, 1, 1, 1, 0, 1, 1}};
    zs[0] = 10;
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 10, zs, sec2, 1, sec2, 1) == BSC_ERR_ARG && strstr(errbuf, "plain"), "a compressed add to a plain file");
    EXPECT(lseek(fd, 0, SEEK_END) == size2, "nothing written by a refused call");
    EXPECT(bsc_bigwig_add(bw, 1, data, 32, sec2, 1, sec2, 1) == BSC_OK, "a plain block behind it");
    EXPECT(bsc_bigwig_finish(bw) == BSC_OK, "finish");
    uint8_t head[64];
    EXPECT(pread(fd, head, 64, 0) == 64 && rd32(head + 52) == 0, "a plain file's uncompressBufSize is 0");
    bsc_bigwig_close(bw);
    close(fd);
    /* a descriptor that cannot be written to */
    const int ro = open(path, O_RDONLY);
    bw = NULL;
    EXPECT(bsc_bigwig_open(ro, 2, names, lens, &bp, &bw) == BSC_OK && bw, "open on a read-only descriptor");
    zs[0] = 1, zs[1] = 43;
    EXPECT(bsc_bigwig_add_z(bw, 1, z, 44, zs, sec, 2, zoom, 1) == BSC_ERR_ARG && strstr(errbuf, "write failed"), "a failed data write");
    bsc_bigwig_close(bw);
    close(ro);
    unlink(path);
  }
  if (failures) return 1;
  puts("ok");
  return 0;
}
