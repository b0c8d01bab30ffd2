/*
 * bigbed.c — the bedMethyl bigBed on the host: the host form of a call's stream of items, the summary of every block of B items and of
 * every level-0 zoom window, from packed records (bsc_bigbed_blocks_recs), and the writer of the file (bsc_bigbed_open / _add / _add_z /
 * _finish / _close).  include/bscall_amd.h has the rule and the file's layout; everything here is written from that text.  The writer
 * never walks the item bytes: a block's place is arithmetic on its offsets (or the sum of the streams' sizes), the trees (csrc/bbi_trees.h,
 * shared with bigwig.c) and the zoom levels are arithmetic on the summaries.  integration/bigbed_san.c drives both under the sanitizers.
 *
 * This is the CHECKER of the device's encoder (csrc/bigbeddev.hip): the device writes, for any records, exactly the bytes this file
 * writes; tests/test_gpu_bigbed.py compares them.  Plain C over bsc_meth_format_rec — an item's text is that function's line, cut behind
 * its third tab —, nothing shared with the device code.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

/* libz is wanted by a compressed writer's bsc_bigbed_finish alone: a weak reference, as in bigwig.c */
extern int compress2(Bytef *dest, uLongf *destLen, const Bytef *source, uLong sourceLen, int level) __attribute__((weak));

#include "../../include/bscall_amd.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

#include "bbi_trees.h" /* the byte buffer, the checked pwrite, the two trees: shared with bigwig.c */

#define BB_MAGIC 0x8789F2EBu
#define BB_ZBLOCK 512u /* records a zoom block */
#define BB_LEVELS 8

void bsc_bb_params_default(bsc_bb_params *p) {
  if (!p) return;
  p->items_per_block = 512;
  p->reduction = 1024;
}

/* record r's item -> item[BSC_BB_ITEM_MAX]; returns its length, 0 when the record is no site, < 0 for a bad argument */
static long bb_item_of(const bsc_vcf_rec *r, uint32_t chrom_id, const bsc_meth_params *p, uint8_t *item) {
  char line[160]; /* "c" + 111 at most */
  const long n = bsc_meth_format_rec(r, "c", p, line, sizeof line);
  if (n <= 0) return n;
  if ((size_t)n > sizeof line) return -1;
  const char *q = line;
  for (int tabs = 0; tabs < 3; q++) { /* behind the third tab: the name */
    if (q >= line + n) return -1;
    if (*q == '\t') tabs++;
  }
  const size_t text = (size_t)(line + n - q); /* the newline included */
  if (line[n - 1] != '\n' || 12 + text > BSC_BB_ITEM_MAX || 12 + text < BSC_BB_ITEM_MIN) return -1;
  put32(item, chrom_id);
  put32(item + 4, r->core.pos - 1u);
  put32(item + 8, r->core.pos);
  memcpy(item + 12, q, text - 1);
  item[12 + text - 1] = 0;
  return (long)(12 + text);
}

int bsc_bigbed_blocks_recs(const bsc_vcf_rec *recs, size_t n, uint32_t chrom_id, const bsc_meth_params *params, const bsc_bb_params *bb_params,
                           void *out, uint64_t cap, uint64_t *n_bytes, bsc_bb_sum *blocks, uint64_t *n_blocks, bsc_bb_sum *zoom0, uint64_t *n_zoom0) {
  if ((!recs && n) || !params || !bb_params || !n_bytes || !n_blocks || !n_zoom0 || (!out && cap)) return BSC_ERR_ARG;
  if (params->contexts != BSC_METH_CPG && params->contexts != BSC_METH_ALL) return BSC_ERR_ARG;
  const uint64_t B = bb_params->items_per_block, red = bb_params->reduction;
  if (B < 1 || B > 65535 || red < 1) return BSC_ERR_ARG;
  const uint64_t blk_room = *n_blocks, zoom_room = *n_zoom0;
  if ((blk_room && !blocks) || (zoom_room && !zoom0)) return BSC_ERR_ARG;
  uint8_t item[BSC_BB_ITEM_MAX];
  /* the needs first: nothing is written into a room too small */
  uint64_t bytes = 0, sites = 0, wins = 0, last_w = 0;
  for (size_t i = 0; i < n; i++) {
    const long len = bb_item_of(&recs[i], chrom_id, params, item);
    if (len < 0) return BSC_ERR_ARG;
    if (!len) continue;
    const uint64_t w = (uint64_t)(recs[i].core.pos - 1u) / red;
    if (!sites || w != last_w) wins++;
    last_w = w;
    sites++;
    bytes += (uint64_t)len;
  }
  const uint64_t blks = (sites + B - 1) / B;
  *n_bytes = bytes;
  *n_blocks = blks;
  *n_zoom0 = wins;
  if (bytes > cap || blks > blk_room || wins > zoom_room) return BSC_ERR_ARG;
  uint64_t at = 0, rank = 0, nw = 0;
  for (size_t i = 0; i < n; i++) {
    const long len = bb_item_of(&recs[i], chrom_id, params, item);
    if (len <= 0) continue;
    const uint32_t start = recs[i].core.pos - 1u;
    bsc_bb_sum *b = &blocks[rank / B];
    if (rank % B == 0) {
      b->start = start;
      b->count = 0;
      b->_pad = 0;
      b->off = at;
    }
    b->end = start + 1u;
    b->count++;
    if (!nw || (uint64_t)start / red != (uint64_t)zoom0[nw - 1].start / red) {
      bsc_bb_sum *z = &zoom0[nw++];
      z->start = start;
      z->count = 0;
      z->_pad = 0;
      z->off = 0;
    }
    zoom0[nw - 1].end = start + 1u;
    zoom0[nw - 1].count++;
    memcpy((uint8_t *)out + at, item, (size_t)len);
    at += (uint64_t)len;
    rank++;
  }
  return BSC_OK;
}

/* ---- the writer ------------------------------------------------------------------------------------------------------------------------- */
/* the autoSql text of the file, as include/bscall_amd.h fixes it */
static const char BB_AUTOSQL[] =
    "table bedMethyl\n"
    "\"Methylation level per cytosine\"\n"
    "(\n"
    "string chrom; \"Reference sequence\"\n"
    "uint chromStart; \"Start, 0-based\"\n"
    "uint chromEnd; \"End\"\n"
    "string name; \"Context: CG, CHG, CHH or CHN\"\n"
    "uint score; \"Coverage, capped at 1000\"\n"
    "char[1] strand; \"+ or -\"\n"
    "uint thickStart; \"Start\"\n"
    "uint thickEnd; \"End\"\n"
    "uint reserved; \"Colour by level (itemRgb)\"\n"
    "bigint coverage; \"Informative reads: non-converted + converted\"\n"
    "uint percent; \"Methylation level, percent, rounded half up\"\n"
    "uint nonConverted; \"Non-converted reads\"\n"
    "uint converted; \"Converted reads\"\n"
    "uint gq; \"Phred-scaled genotype quality\"\n"
    "string filter; \"FILTER of the call\"\n"
    ")\n";
#define BB_TREE_AT (296u + (uint32_t)sizeof BB_AUTOSQL) /* the chromosome tree: behind the text and its NUL */

typedef struct {
  uint32_t tid, start, end, count;
  uint64_t off, size, raw; /* a block's place in the file, its bytes there, its raw bytes (not used by a zoom record) */
} bb_rec;

struct bsc_bigbed {
  int fd;
  uint32_t n_refs, key_size;
  char **names;
  uint32_t *lens;
  bsc_bb_params par;
  uint64_t data_start; /* fullDataOffset: the item count, the blocks behind it */
  uint64_t data_bytes, n_items;
  bb_rec *blk;
  uint64_t n_blk, cap_blk;
  bb_rec *z0;
  uint64_t n_z0, cap_z0;
  int have_last, finished;
  int mode; /* 0 until the first non-empty add; then BB_PLAIN or BB_Z */
  uint32_t last_tid, last_end;
};
enum { BB_PLAIN = 1, BB_Z = 2 };

static int bb_params_ok(const bsc_bb_params *p) { return p && p->items_per_block >= 1 && p->items_per_block <= 65535 && p->reduction >= 1; }

int bsc_bigbed_open(int fd, uint32_t n_refs, const char *const *names, const uint32_t *lens, const bsc_bb_params *bb_params, bsc_bigbed **out) {
  static const char who[] = "bsc_bigbed_open";
  if (out) *out = NULL;
  if (!out || fd < 0 || (n_refs && (!names || !lens))) return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (!bb_params_ok(bb_params)) return bsc_set_error(BSC_ERR_ARG, "%s: items_per_block is 1 .. 65535, reduction 1 or more", who);
  bsc_bigbed *bb = calloc(1, sizeof *bb);
  if (!bb) return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  bb->fd = fd;
  bb->par = *bb_params;
  bb->names = calloc(n_refs ? n_refs : 1, sizeof *bb->names);
  bb->lens = calloc(n_refs ? n_refs : 1, sizeof *bb->lens);
  int bad = !bb->names || !bb->lens;
  for (uint32_t k = 0; k < n_refs && !bad; k++) {
    const size_t len = names[k] ? strlen(names[k]) : 0;
    if (!names[k] || len > 65535) {
      bsc_bigbed_close(bb);
      return bsc_set_error(BSC_ERR_ARG, "%s: contig %u has no name, or one of more than 65535 bytes", who, k);
    }
    bb->names[k] = malloc(len + 1);
    if (!bb->names[k]) {
      bad = 1;
      break;
    }
    memcpy(bb->names[k], names[k], len + 1);
    bb->lens[k] = lens[k];
    bb->n_refs = k + 1;
    if (len > bb->key_size) bb->key_size = (uint32_t)len;
  }
  if (bad) {
    bsc_bigbed_close(bb);
    return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  }
  bb->data_start = BB_TREE_AT + chrom_tree_bytes(n_refs, bb->key_size);
  *out = bb;
  return BSC_OK;
}

void bsc_bigbed_close(bsc_bigbed *bb) {
  if (!bb) return;
  for (uint32_t k = 0; bb->names && k < bb->n_refs; k++) free(bb->names[k]);
  free(bb->names);
  free(bb->lens);
  free(bb->blk);
  free(bb->z0);
  free(bb);
}

/* bsc_bigbed_add (z_sizes NULL: data is the plain stream of raw_bytes bytes) and bsc_bigbed_add_z (data is the blocks' zlib streams, z_sizes
 * their lengths, raw_bytes the length of the stream they were made from).  Every check comes before the one write. */
static int bb_add(bsc_bigbed *bb, const char *who, uint32_t tid, const void *data, uint64_t n_bytes, const uint32_t *z_sizes, int z, uint64_t raw_bytes,
                  const bsc_bb_sum *blocks, uint64_t n_blocks, const bsc_bb_sum *zoom0, uint64_t n_zoom0) {
  if (!bb || (n_bytes && !data) || (n_blocks && !blocks) || (n_zoom0 && !zoom0) || (z && n_blocks && !z_sizes))
    return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (bb->finished) return bsc_set_error(BSC_ERR_ARG, "%s: the file is finished", who);
  if (tid >= bb->n_refs) return bsc_set_error(BSC_ERR_ARG, "%s: contig %u of %u", who, tid, bb->n_refs);
  if (bb->have_last && tid < bb->last_tid) return bsc_set_error(BSC_ERR_ARG, "%s: contig %u behind contig %u", who, tid, bb->last_tid);
  if (!n_blocks) {
    if (n_bytes || raw_bytes || n_zoom0) return bsc_set_error(BSC_ERR_ARG, "%s: bytes or windows without a block", who);
    return BSC_OK;
  }
  if (!n_zoom0) return bsc_set_error(BSC_ERR_ARG, "%s: blocks without a window", who);
  if (bb->mode && bb->mode != (z ? BB_Z : BB_PLAIN))
    return bsc_set_error(BSC_ERR_ARG, "%s: the file's blocks are %s", who, bb->mode == BB_Z ? "compressed: bsc_bigbed_add_z adds to it" : "plain: bsc_bigbed_add adds to it");
  const uint64_t B = bb->par.items_per_block, red = bb->par.reduction;
  if (z && B > BSC_BB_Z_ITEMS_MAX) return bsc_set_error(BSC_ERR_ARG, "%s: a compressed file's blocks hold at most %u items, not %llu", who, BSC_BB_Z_ITEMS_MAX, (unsigned long long)B);
  uint64_t sites = 0, zsites = 0, zsum = 0;
  uint32_t end = bb->have_last && tid == bb->last_tid ? bb->last_end : 0;
  if (blocks[0].start < end)
    return bsc_set_error(BSC_ERR_ARG, "%s: contig %u: start %u lies below the previous end %u", who, tid, blocks[0].start, end);
  if (blocks[0].off) return bsc_set_error(BSC_ERR_ARG, "%s: the first block's offset is %llu, not 0", who, (unsigned long long)blocks[0].off);
  for (uint64_t k = 0; k < n_blocks; k++) {
    const bsc_bb_sum *s = &blocks[k];
    if (!s->count || s->count > B || (k + 1 < n_blocks && s->count != B) || s->start < end || s->end <= s->start || s->end - s->start < s->count)
      return bsc_set_error(BSC_ERR_ARG, "%s: block %llu is not one of %llu sites in order", who, (unsigned long long)k, (unsigned long long)B);
    const uint64_t next = k + 1 < n_blocks ? blocks[k + 1].off : raw_bytes;
    if (next <= s->off) return bsc_set_error(BSC_ERR_ARG, "%s: block %llu: the offsets do not ascend to the stream's %llu bytes", who, (unsigned long long)k, (unsigned long long)raw_bytes);
    const uint64_t len = next - s->off;
    if (len < (uint64_t)s->count * BSC_BB_ITEM_MIN || len > (uint64_t)s->count * BSC_BB_ITEM_MAX)
      return bsc_set_error(BSC_ERR_ARG, "%s: block %llu of %u items has %llu bytes", who, (unsigned long long)k, s->count, (unsigned long long)len);
    if (z) {
      if (!z_sizes[k] || z_sizes[k] > len + 11)
        return bsc_set_error(BSC_ERR_ARG, "%s: block %llu of %llu bytes has a stream of %u bytes", who, (unsigned long long)k, (unsigned long long)len, z_sizes[k]);
      zsum += z_sizes[k];
    }
    end = s->end;
    sites += s->count;
  }
  if (z ? zsum != n_bytes : raw_bytes != n_bytes)
    return bsc_set_error(BSC_ERR_ARG, "%s: the blocks add up to %llu bytes, not %llu", who, (unsigned long long)(z ? zsum : raw_bytes), (unsigned long long)n_bytes);
  for (uint64_t k = 0; k < n_zoom0; k++) {
    const bsc_bb_sum *w = &zoom0[k];
    if (!w->count || w->end <= w->start || (w->end - 1u) / red != w->start / red || (k && w->start / red <= zoom0[k - 1].start / red))
      return bsc_set_error(BSC_ERR_ARG, "%s: window %llu is not one window of %llu bases in order", who, (unsigned long long)k, (unsigned long long)red);
    zsites += w->count;
  }
  if (zsites != sites || zoom0[0].start != blocks[0].start || zoom0[n_zoom0 - 1].end != end)
    return bsc_set_error(BSC_ERR_ARG, "%s: the windows do not hold the blocks' sites", who);
  if (grow((void **)&bb->blk, &bb->cap_blk, bb->n_blk + n_blocks, sizeof *bb->blk)) return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  if (grow((void **)&bb->z0, &bb->cap_z0, bb->n_z0 + n_zoom0, sizeof *bb->z0)) return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  const uint64_t base = bb->data_start + 8 + bb->data_bytes;
  if (write_all(bb->fd, data, n_bytes, base)) return bsc_set_error(BSC_ERR_ARG, "%s: write failed: %s", who, strerror(errno));
  uint64_t at = base;
  for (uint64_t k = 0; k < n_blocks; k++) {
    bb_rec *r = &bb->blk[bb->n_blk++];
    r->tid = tid;
    r->start = blocks[k].start;
    r->end = blocks[k].end;
    r->count = blocks[k].count;
    r->raw = (k + 1 < n_blocks ? blocks[k + 1].off : raw_bytes) - blocks[k].off;
    r->off = at;
    r->size = z ? z_sizes[k] : r->raw;
    at += r->size;
  }
  for (uint64_t k = 0; k < n_zoom0; k++) {
    bb_rec *prev = bb->n_z0 ? &bb->z0[bb->n_z0 - 1] : NULL;
    if (!k && prev && prev->tid == tid && prev->start / red == zoom0[0].start / red) { /* a window two adds share: the counts add */
      prev->count += zoom0[0].count;
      prev->end = zoom0[0].end;
      continue;
    }
    bb_rec *r = &bb->z0[bb->n_z0++];
    memset(r, 0, sizeof *r);
    r->tid = tid;
    r->start = zoom0[k].start;
    r->end = zoom0[k].end;
    r->count = zoom0[k].count;
  }
  bb->data_bytes += n_bytes;
  bb->n_items += sites;
  bb->have_last = 1;
  bb->mode = z ? BB_Z : BB_PLAIN;
  bb->last_tid = tid;
  bb->last_end = end;
  return BSC_OK;
}

int bsc_bigbed_add(bsc_bigbed *bb, uint32_t tid, const void *data, uint64_t n_bytes, const bsc_bb_sum *blocks, uint64_t n_blocks,
                   const bsc_bb_sum *zoom0, uint64_t n_zoom0) {
  return bb_add(bb, "bsc_bigbed_add", tid, data, n_bytes, NULL, 0, n_bytes, blocks, n_blocks, zoom0, n_zoom0);
}

int bsc_bigbed_add_z(bsc_bigbed *bb, uint32_t tid, const void *zdata, uint64_t z_bytes, const uint32_t *z_sizes, uint64_t raw_bytes,
                     const bsc_bb_sum *blocks, uint64_t n_blocks, const bsc_bb_sum *zoom0, uint64_t n_zoom0) {
  return bb_add(bb, "bsc_bigbed_add_z", tid, zdata, z_bytes, z_sizes, 1, raw_bytes, blocks, n_blocks, zoom0, n_zoom0);
}

/* a zoom level's records at file offset `at`: the count, the blocks — each deflated (compress2, the default level) where z —, the R-tree
 * over the blocks; *index = the tree's offset; *max_raw: raised to the largest block's raw bytes */
static int bb_zoom_level_put(bw_buf *b, const bb_rec *r, uint64_t n, uint64_t at, uint64_t *index, int z, uint64_t *max_raw) {
  const uint64_t b0 = b->n;
  rt_item *it = malloc((size_t)(n ? n : 1) * sizeof *it); /* (at most one block per record) */
  if (!it) return -1;
  uint64_t n_it = 0;
  buf_u32(b, (uint32_t)n);
  for (uint64_t i = 0; i < n;) {
    uint64_t j = i;
    while (j < n && j - i < BB_ZBLOCK && r[j].tid == r[i].tid) j++;
    rt_item v = {r[i].tid, r[i].start, r[i].tid, r[j - 1].end, at + (b->n - b0), 32 * (j - i)};
    const size_t raw_at = b->n;
    if (v.size > *max_raw) *max_raw = v.size;
    for (; i < j; i++) { /* the depth is 1 wherever it is not 0 */
      buf_u32(b, r[i].tid);
      buf_u32(b, r[i].start);
      buf_u32(b, r[i].end);
      buf_u32(b, r[i].count);
      buf_f32(b, 1.0f);
      buf_f32(b, 1.0f);
      buf_f32(b, (float)r[i].count);
      buf_f32(b, (float)r[i].count);
    }
    if (z && !b->oom) { /* the block's raw bytes, just written, give way to their stream */
      uLongf zn = (uLongf)(v.size + v.size / 512 + 64); /* (above compressBound: at most 16 KiB in) */
      Bytef *zb = malloc(zn);
      if (!zb || compress2(zb, &zn, b->p + raw_at, (uLong)v.size, Z_DEFAULT_COMPRESSION) != Z_OK) {
        free(zb);
        free(it);
        return -1;
      }
      b->n = raw_at;
      uint8_t *q = buf_room(b, zn);
      if (q) memcpy(q, zb, zn);
      free(zb);
      v.size = zn;
    }
    it[n_it++] = v;
  }
  *index = at + (b->n - b0);
  const int rc = rtree_put(b, it, n_it, *index, *index, 1);
  free(it);
  return rc;
}

int bsc_bigbed_finish(bsc_bigbed *bb) {
  static const char who[] = "bsc_bigbed_finish";
  if (!bb) return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  if (bb->finished) return bsc_set_error(BSC_ERR_ARG, "%s: the file is finished", who);
  if (bb->n_z0 > 0xffffffffull) return bsc_set_error(BSC_ERR_ARG, "%s: more than 2^32 - 1 zoom records", who);
  if (bb->mode == BB_Z && !compress2) return bsc_set_error(BSC_ERR_ARG, "%s: a compressed file needs libz, which this program does not link", who);
  bw_buf head = {0}, tail = {0};
  int rc = 0, levels = 0;
  uint64_t z_red[BB_LEVELS] = {0}, z_data[BB_LEVELS] = {0}, z_index[BB_LEVELS] = {0};
  const uint64_t index_at = bb->data_start + 8 + bb->data_bytes;
  const int z = bb->mode == BB_Z;
  uint64_t max_raw = 0;
  /* the blocks' index */
  rt_item *it = malloc((size_t)(bb->n_blk ? bb->n_blk : 1) * sizeof *it);
  if (!it) rc = -1;
  for (uint64_t k = 0; k < bb->n_blk && !rc; k++) {
    const bb_rec *s = &bb->blk[k];
    const rt_item v = {s->tid, s->start, s->tid, s->end, s->off, s->size};
    it[k] = v;
    if (z && s->raw > max_raw) max_raw = s->raw;
  }
  if (!rc) rc = rtree_put(&tail, it, bb->n_blk, index_at, index_at, bb->par.items_per_block);
  free(it);
  /* the pyramid */
  bb_rec *cur = bb->z0, *own = NULL;
  uint64_t n_cur = bb->n_z0, width = bb->par.reduction;
  for (int l = 0; l < BB_LEVELS && !rc; l++) {
    if (l) {
      if (n_cur <= 256) break;
      width *= 4; /* (reduction < 2^32, 4^7 = 2^14: 64 bits hold it) */
      bb_rec *next = malloc((size_t)n_cur * sizeof *next);
      if (!next) {
        rc = -1;
        break;
      }
      uint64_t m = 0;
      for (uint64_t i = 0; i < n_cur; i++) {
        if (m && next[m - 1].tid == cur[i].tid && next[m - 1].start / width == cur[i].start / width) {
          next[m - 1].count += cur[i].count;
          next[m - 1].end = cur[i].end;
        } else {
          next[m++] = cur[i];
        }
      }
      free(own);
      cur = own = next;
      n_cur = m;
    }
    z_red[l] = width < 0xffffffffull ? width : 0xffffffffull;
    z_data[l] = index_at + tail.n;
    rc = bb_zoom_level_put(&tail, cur, n_cur, z_data[l], &z_index[l], z, &max_raw);
    levels = l + 1;
  }
  free(own);
  buf_u32(&tail, BB_MAGIC);
  /* the header, the zoom headers, the total summary, the autoSql text, the chromosome tree, the item count */
  buf_u32(&head, BB_MAGIC);
  buf_u16(&head, 4);
  buf_u16(&head, (uint16_t)levels);
  buf_u64(&head, BB_TREE_AT);
  buf_u64(&head, bb->data_start);
  buf_u64(&head, index_at);
  buf_u16(&head, 15);
  buf_u16(&head, 9);
  buf_u64(&head, 296);
  buf_u64(&head, 256);
  buf_u32(&head, z ? (uint32_t)max_raw : 0); /* uncompressBufSize: at most 0xFF00 or 32 * 512 */
  buf_u64(&head, 0);
  for (int l = 0; l < BB_LEVELS; l++) {
    buf_u32(&head, l < levels ? (uint32_t)z_red[l] : 0);
    buf_u32(&head, 0);
    buf_u64(&head, l < levels ? z_data[l] : 0);
    buf_u64(&head, l < levels ? z_index[l] : 0);
  }
  buf_u64(&head, bb->n_items);
  buf_f64(&head, bb->n_items ? 1.0 : 0.0);
  buf_f64(&head, bb->n_items ? 1.0 : 0.0);
  buf_f64(&head, (double)bb->n_items);
  buf_f64(&head, (double)bb->n_items);
  {
    uint8_t *q = buf_room(&head, sizeof BB_AUTOSQL); /* the NUL included */
    if (q) memcpy(q, BB_AUTOSQL, sizeof BB_AUTOSQL);
  }
  if (!rc) rc = chrom_tree_put(&head, bb->n_refs, bb->key_size, bb->names, bb->lens, BB_TREE_AT);
  buf_u64(&head, bb->n_items);
  if (!rc && (head.oom || tail.oom)) rc = -1;
  if (rc) {
    free(head.p);
    free(tail.p);
    return bsc_set_error(BSC_ERR_NOMEM, "%s: out of memory", who);
  }
  if (head.n != bb->data_start + 8) {
    free(head.p);
    free(tail.p);
    return bsc_set_error(BSC_ERR_ARG, "%s: the head is %zu bytes, not %llu", who, head.n, (unsigned long long)bb->data_start + 8);
  }
  if (write_all(bb->fd, tail.p, tail.n, index_at) || write_all(bb->fd, head.p, head.n, 0))
    rc = bsc_set_error(BSC_ERR_ARG, "%s: write failed: %s", who, strerror(errno));
  free(head.p);
  free(tail.p);
  if (!rc) bb->finished = 1;
  return rc;
}
