/*
 * bigbed_san.c — the host form of the bigBed items (csrc/bigbed.c over csrc/methbed.c) as a stand-alone program, meant to be built with
 * -fsanitize=address,undefined (make bigbed-san; tests/test_bigbed_host.py builds its own copy): the records that attain BSC_BB_ITEM_MIN
 * and BSC_BB_ITEM_MAX, every room exact and one short — the arrays are heap blocks of exactly the room, so a byte behind one is an
 * error the sanitizer reports —, blocks of 1, 3 and 512 items, windows that several sites share.  Then the file's writer
 * (bsc_bigbed_open / _add / _add_z / _finish / _close) over the host form's blocks, plain and compressed (zlib's compress2 makes the
 * streams), with 0, 1, 257 and 65 537 blocks, 300 contigs, a window two adds share and every refusal, each checked to leave the file's
 * length as it was.  Prints "ok" and returns 0, or the case that failed.
 */
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include "bscall_amd.h"

static char errbuf[512];
int bsc_set_error(int code, const char *fmt, ...) { /* the library's own lives in bscall_api.c */
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, sizeof errbuf, fmt, ap);
  va_end(ap);
  return code;
}

#define FAIL(...) do { fprintf(stderr, "bigbed_san: " __VA_ARGS__); fputc('\n', stderr); return 1; } while (0)

static void site(bsc_vcf_rec *r, uint32_t pos, int minus, char cg, char n2, uint32_t a, uint32_t b, unsigned phred, unsigned flt) {
  memset(r, 0, sizeof *r);
  r->core.pos = pos;
  r->core.emit = 1;
  r->core.gt = minus ? 7 : 4;
  r->core.cg = cg;
  r->core.cx_gt[minus ? 0 : 4] = n2;
  r->core.phred = (uint8_t)phred;
  r->core.flt = (uint8_t)flt;
  r->counts[minus ? 6 : 5] = a;
  r->counts[minus ? 4 : 7] = b;
}

/* the call with heap rooms of exactly (cap, blk_room, zoom_room); *out_p etc. are the caller's to free */
static int run(const bsc_vcf_rec *recs, size_t n, uint32_t cid, const bsc_meth_params *mp, const bsc_bb_params *bp, uint64_t cap, uint64_t blk_room,
               uint64_t zoom_room, uint8_t **out_p, bsc_bb_sum **blk_p, bsc_bb_sum **zoom_p, uint64_t need[3]) {
  *out_p = malloc(cap ? cap : 1);
  *blk_p = malloc(blk_room ? blk_room * sizeof(bsc_bb_sum) : 1);
  *zoom_p = malloc(zoom_room ? zoom_room * sizeof(bsc_bb_sum) : 1);
  if (!*out_p || !*blk_p || !*zoom_p) return -100;
  need[1] = blk_room;
  need[2] = zoom_room;
  return bsc_bigbed_blocks_recs(recs, n, cid, mp, bp, cap ? *out_p : NULL, cap, &need[0], blk_room ? *blk_p : NULL, &need[1], zoom_room ? *zoom_p : NULL,
                                &need[2]);
}

static off_t size_of(int fd) {
  struct stat st;
  return fstat(fd, &st) ? (off_t)-1 : st.st_size;
}

/* n sites at start0, start0 + step, .. on contig tid through the host form and into the writer, plain or as zlib streams */
static int add_sites(bsc_bigbed *bb, uint32_t tid, uint32_t start0, uint32_t step, uint32_t n, const bsc_bb_params *bp, int z, int expect) {
  bsc_meth_params mp;
  bsc_meth_params_default(&mp);
  bsc_vcf_rec *recs = malloc((n ? n : 1) * sizeof *recs);
  if (!recs) return -100;
  for (uint32_t i = 0; i < n; i++) site(&recs[i], start0 + 1 + i * step, (int)(i & 1), 'C', 'G', i % 97, 1 + i % 13, i % 256, i % 5 ? 0 : 1);
  uint64_t need[3] = {0, 0, 0};
  int rc = bsc_bigbed_blocks_recs(recs, n, tid, &mp, bp, NULL, 0, &need[0], NULL, &need[1], NULL, &need[2]);
  if (n && rc != BSC_ERR_ARG) return -101;
  uint8_t *out = malloc(need[0] ? need[0] : 1);
  bsc_bb_sum *blk = malloc((need[1] ? need[1] : 1) * sizeof *blk), *zoom = malloc((need[2] ? need[2] : 1) * sizeof *zoom);
  uint32_t *zs = malloc((need[1] ? need[1] : 1) * sizeof *zs);
  uint8_t *zbuf = malloc(need[0] + 64 * need[1] + 64);
  if (!out || !blk || !zoom || !zs || !zbuf) return -100;
  const uint64_t nb = need[0], nk = need[1], nz = need[2];
  if (n && bsc_bigbed_blocks_recs(recs, n, tid, &mp, bp, out, nb, &need[0], blk, &need[1], zoom, &need[2])) return -102;
  if (!z) {
    rc = bsc_bigbed_add(bb, tid, nb ? out : NULL, nb, nk ? blk : NULL, nk, nz ? zoom : NULL, nz);
  } else {
    uint64_t zat = 0;
    for (uint64_t k = 0; k < nk; k++) {
      const uint64_t len = (k + 1 < nk ? blk[k + 1].off : nb) - blk[k].off;
      uLongf zn = (uLongf)(len + 64);
      if (compress2(zbuf + zat, &zn, out + blk[k].off, (uLong)len, 1) != Z_OK) return -103;
      if (zn > len + 11) return -104; /* (the rule's bound; zlib's stored form stays inside it for blocks of this size) */
      zs[k] = (uint32_t)zn;
      zat += zn;
    }
    rc = bsc_bigbed_add_z(bb, tid, zat ? zbuf : NULL, zat, nk ? zs : NULL, nb, nk ? blk : NULL, nk, nz ? zoom : NULL, nz);
  }
  free(recs), free(out), free(blk), free(zoom), free(zs), free(zbuf);
  return rc == expect ? 0 : (rc ? rc : -105);
}

static int writer_cases(void) {
  enum { N_REFS = 300 };
  static char name_buf[N_REFS][12];
  const char *names[N_REFS];
  uint32_t lens[N_REFS];
  for (int k = 0; k < N_REFS; k++) {
    snprintf(name_buf[k], sizeof name_buf[k], "c%d%s", k * 7919 % 1000, k % 3 ? "" : "xy");
    names[k] = name_buf[k];
    lens[k] = 4000000000u;
  }
  char path[] = "/tmp/bigbed_san_XXXXXX";
  const int fd = mkstemp(path);
  if (fd < 0) FAIL("no temporary file");
  unlink(path);
  for (int z = 0; z < 2; z++) {
    static const uint32_t Bs[4] = {1, 3, 512, 652};
    for (int c = 0; c < 4; c++) {
      bsc_bb_params bp = {Bs[c], c == 1 ? 1u : 1000u};
      bsc_bigbed *bb = NULL;
      if (ftruncate(fd, 0)) FAIL("ftruncate");
      if (bsc_bigbed_open(fd, N_REFS, names, lens, &bp, &bb) || !bb) FAIL("open: %s", errbuf);
      if (add_sites(bb, 0, 0, 1, 0, &bp, z, BSC_OK)) FAIL("z %d B %u: an add without a site: %s", z, Bs[c], errbuf);
      if (add_sites(bb, 0, 10, 7, c == 0 ? 65537 : 3000, &bp, z, BSC_OK)) FAIL("z %d B %u: first add: %s", z, Bs[c], errbuf);
      off_t len = size_of(fd);
      if (len <= 0) FAIL("nothing written");
      /* refusals: nothing is written by any of them */
      if (add_sites(bb, 0, 10, 7, 10, &bp, z, BSC_ERR_ARG) || size_of(fd) != len) FAIL("z %d: a start below the previous end accepted: %s", z, errbuf);
      if (add_sites(bb, N_REFS, 10, 7, 10, &bp, z, BSC_ERR_ARG) || size_of(fd) != len) FAIL("z %d: a contig not in the header accepted", z);
      if (add_sites(bb, 0, 600000, 7, 10, &bp, !z, BSC_ERR_ARG) || size_of(fd) != len) FAIL("z %d: the other kind of add accepted", z);
      if (add_sites(bb, 0, 600000, 300, 771, &bp, z, BSC_OK)) FAIL("z %d B %u: second add: %s", z, Bs[c], errbuf); /* shares a window when reduction = 1000 */
      for (uint32_t t = 1; t < N_REFS; t += c == 2 ? 1 : 37)
        if (add_sites(bb, t, t, 5000, 2 + t % 3, &bp, z, BSC_OK)) FAIL("z %d: contig %u: %s", z, t, errbuf);
      len = size_of(fd);
      if (add_sites(bb, 5, 10, 7, 10, &bp, z, BSC_ERR_ARG) || size_of(fd) != len) FAIL("z %d: a contig behind the last accepted", z);
      if (bsc_bigbed_finish(bb)) FAIL("z %d B %u: finish: %s", z, Bs[c], errbuf);
      if (bsc_bigbed_finish(bb) != BSC_ERR_ARG) FAIL("a second finish accepted");
      if (add_sites(bb, N_REFS - 1, 900000, 7, 10, &bp, z, BSC_ERR_ARG)) FAIL("an add behind finish accepted");
      uint8_t head[8];
      if (pread(fd, head, 8, 0) != 8 || head[0] != 0xEB || head[1] != 0xF2 || head[2] != 0x89 || head[3] != 0x87 || head[4] != 4) FAIL("the header's magic");
      bsc_bigbed_close(bb);
    }
  }
  { /* no site at all; a compressed writer above the cap; bad parameters */
    bsc_bb_params bp = {512, 1024};
    bsc_bigbed *bb = NULL;
    if (ftruncate(fd, 0)) FAIL("ftruncate");
    if (bsc_bigbed_open(fd, 0, NULL, NULL, &bp, &bb) || bsc_bigbed_finish(bb)) FAIL("an empty file: %s", errbuf);
    bsc_bigbed_close(bb);
    bp.items_per_block = 653;
    if (bsc_bigbed_open(fd, N_REFS, names, lens, &bp, &bb)) FAIL("open");
    if (add_sites(bb, 0, 10, 7, 700, &bp, 1, BSC_ERR_ARG)) FAIL("653 items a block accepted by a compressed add");
    if (add_sites(bb, 0, 10, 7, 700, &bp, 0, BSC_OK)) FAIL("653 items a block refused by a plain add: %s", errbuf);
    bsc_bigbed_close(bb); /* unfinished: freed all the same */
    bp.items_per_block = 0;
    if (bsc_bigbed_open(fd, N_REFS, names, lens, &bp, &bb) != BSC_ERR_ARG || bb) FAIL("B = 0 accepted");
    bsc_bigbed_close(NULL);
  }
  close(fd);
  return 0;
}

int main(void) {
  bsc_meth_params mp;
  bsc_bb_params bp;
  bsc_meth_params_default(&mp);
  bsc_bb_params_default(&bp);
  if (bp.items_per_block != 512 || bp.reduction != 1024) FAIL("defaults");
  mp.contexts = BSC_METH_ALL;
  uint8_t *out;
  bsc_bb_sum *blk, *zoom;
  uint64_t need[3];

  { /* the shortest and the longest item */
    bsc_vcf_rec r[2];
    site(&r[0], 9, 0, 'C', 'G', 0, 1, 9, 0);
    site(&r[1], 0xffffffffu, 1, 'H', 'C', 4000000000u, 4000000000u, 255, 1);
    if (run(r, 2, 7, &mp, &bp, BSC_BB_ITEM_MIN + BSC_BB_ITEM_MAX, 1, 2, &out, &blk, &zoom, need)) FAIL("min/max: refused");
    if (need[0] != BSC_BB_ITEM_MIN + BSC_BB_ITEM_MAX || need[1] != 1 || need[2] != 2) FAIL("min/max: %llu bytes", (unsigned long long)need[0]);
    static const char lo[] = "CG\t1\t+\t8\t9\t0,255,0\t1\t0\t0\t1\t9\tPASS";
    static const char hi[] = "CHG\t1000\t-\t4294967294\t4294967295\t255,255,0\t8000000000\t50\t4000000000\t4000000000\t255\tfail";
    if (sizeof lo != BSC_BB_ITEM_MIN - 12 || memcmp(out + 12, lo, sizeof lo)) FAIL("the shortest item's text");
    if (sizeof hi != BSC_BB_ITEM_MAX - 12 || memcmp(out + BSC_BB_ITEM_MIN + 12, hi, sizeof hi)) FAIL("the longest item's text");
    static const uint8_t head[12] = {7, 0, 0, 0, 0xfe, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
    if (memcmp(out + BSC_BB_ITEM_MIN, head, 12)) FAIL("the longest item's head");
    if (blk[0].start != 8 || blk[0].end != 0xffffffffu || blk[0].count != 2 || blk[0].off != 0 || blk[0]._pad) FAIL("min/max: block");
    if (zoom[0].start != 8 || zoom[0].end != 9 || zoom[1].start != 0xfffffffeu || zoom[1].count != 1 || zoom[1].off) FAIL("min/max: windows");
    free(out), free(blk), free(zoom);
  }

  enum { N = 1300 };
  bsc_vcf_rec *recs = malloc(N * sizeof *recs);
  if (!recs) FAIL("out of memory");
  uint64_t sites = 0;
  for (uint32_t i = 0; i < N; i++) {
    site(&recs[i], 1000 + i, i % 3 == 0, i % 5 ? 'C' : 'H', "ACGTN"[i % 5], i * 7919u, i % 11 ? i * 104729u : 0u, i % 256, i % 4 ? 0 : (i % 8 ? 128 : 3));
    if (i % 7 == 0) recs[i].core.gt = 5; /* no site */
    else if (recs[i].counts[5] + recs[i].counts[7] + recs[i].counts[6] + recs[i].counts[4]) sites++;
  }
  static const uint32_t Bs[3] = {1, 3, 512}, reds[3] = {1, 100, 1024};
  for (int k = 0; k < 3; k++) {
    bp.items_per_block = Bs[k];
    bp.reduction = reds[k];
    uint64_t ask[3] = {0, 0, 0};
    if (bsc_bigbed_blocks_recs(recs, N, 1, &mp, &bp, NULL, 0, &ask[0], NULL, &ask[1], NULL, &ask[2]) != BSC_ERR_ARG) FAIL("B %u: no room accepted", Bs[k]);
    if (ask[1] != (sites + Bs[k] - 1) / Bs[k] || !ask[2] || ask[0] < sites * BSC_BB_ITEM_MIN || ask[0] > sites * BSC_BB_ITEM_MAX) FAIL("B %u: the needs", Bs[k]);
    if (run(recs, N, 1, &mp, &bp, ask[0], ask[1], ask[2], &out, &blk, &zoom, need)) FAIL("B %u: exact rooms refused", Bs[k]);
    uint64_t cnt = 0, zc = 0;
    for (uint64_t j = 0; j < need[1]; j++) {
      if (!j && blk[j].off) FAIL("B %u: the first offset", Bs[k]);
      if (j && blk[j].off <= blk[j - 1].off) FAIL("B %u: offsets do not ascend", Bs[k]);
      if (j + 1 < need[1] && blk[j].count != Bs[k]) FAIL("B %u: a short block that is not the last", Bs[k]);
      if (out[blk[j].off + 4] != (uint8_t)blk[j].start) FAIL("B %u: a block's offset is not at an item", Bs[k]);
      cnt += blk[j].count;
    }
    for (uint64_t j = 0; j < need[2]; j++) {
      if (j && zoom[j].start / reds[k] <= zoom[j - 1].start / reds[k]) FAIL("red %u: windows do not ascend", reds[k]);
      if ((zoom[j].end - 1) / reds[k] != zoom[j].start / reds[k]) FAIL("red %u: a window over a border", reds[k]);
      zc += zoom[j].count;
    }
    if (cnt != sites || zc != sites || out[need[0] - 1] != 0) FAIL("B %u: %llu sites, %llu in windows, not %llu", Bs[k], (unsigned long long)cnt, (unsigned long long)zc, (unsigned long long)sites);
    free(out), free(blk), free(zoom);
    for (int s = 0; s < 3; s++) { /* each room one short: the needs, and not one byte written (the rooms are exact heap blocks) */
      if (run(recs, N, 1, &mp, &bp, ask[0] - (s == 0), ask[1] - (s == 1), ask[2] - (s == 2), &out, &blk, &zoom, need) != BSC_ERR_ARG) FAIL("B %u: room %d short accepted", Bs[k], s);
      if (need[0] != ask[0] || need[1] != ask[1] || need[2] != ask[2]) FAIL("B %u: room %d short: the needs", Bs[k], s);
      free(out), free(blk), free(zoom);
    }
  }
  need[0] = need[1] = need[2] = 0;
  if (bsc_bigbed_blocks_recs(recs, 0, 1, &mp, &bp, NULL, 0, &need[0], NULL, &need[1], NULL, &need[2]) != BSC_OK || need[0] || need[1] || need[2]) FAIL("no record");
  bp.items_per_block = 0;
  if (bsc_bigbed_blocks_recs(recs, N, 1, &mp, &bp, NULL, 0, &need[0], NULL, &need[1], NULL, &need[2]) != BSC_ERR_ARG) FAIL("B = 0 accepted");
  bp.items_per_block = 65536;
  if (bsc_bigbed_blocks_recs(recs, N, 1, &mp, &bp, NULL, 0, &need[0], NULL, &need[1], NULL, &need[2]) != BSC_ERR_ARG) FAIL("B = 65536 accepted");
  free(recs);
  if (writer_cases()) return 1;
  puts("ok");
  return 0;
}
