/*
 * bbi_trees.h — what the two bbiFile writers (csrc/bigwig.c, csrc/bigbed.c) have in common, private to them: a growing byte buffer with
 * little-endian stores, the checked pwrite, the chromosome B+ tree, the R-tree and the arithmetic of their levels (include/bscall_amd.h
 * has the layouts).  Moved out of bigwig.c as it stood: the bigWig file's bytes are what they were.
 */
#ifndef BSC_BBI_TREES_H
#define BSC_BBI_TREES_H
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define BW_NODE 256u /* items a tree node */

static inline void put32(uint8_t *q, uint32_t v) {
  q[0] = (uint8_t)v;
  q[1] = (uint8_t)(v >> 8);
  q[2] = (uint8_t)(v >> 16);
  q[3] = (uint8_t)(v >> 24);
}

typedef struct { /* a leaf item of an R-tree */
  uint32_t c0, s0, c1, e1;
  uint64_t off, size;
} rt_item;

typedef struct {
  uint8_t *p;
  size_t n, cap;
  int oom;
} bw_buf;

static inline void *buf_room(bw_buf *b, size_t k) {
  if (b->oom) return NULL;
  if (b->n + k > b->cap) {
    size_t cap = b->cap ? b->cap : 4096;
    while (cap < b->n + k) cap *= 2;
    uint8_t *q = realloc(b->p, cap);
    if (!q) {
      b->oom = 1;
      return NULL;
    }
    b->p = q;
    b->cap = cap;
  }
  b->n += k;
  return b->p + b->n - k;
}
static inline void buf_u8(bw_buf *b, uint8_t v) {
  uint8_t *q = buf_room(b, 1);
  if (q) q[0] = v;
}
static inline void buf_u16(bw_buf *b, uint16_t v) {
  uint8_t *q = buf_room(b, 2);
  if (q) q[0] = (uint8_t)v, q[1] = (uint8_t)(v >> 8);
}
static inline void buf_u32(bw_buf *b, uint32_t v) {
  uint8_t *q = buf_room(b, 4);
  if (q) put32(q, v);
}
static inline void buf_u64(bw_buf *b, uint64_t v) {
  buf_u32(b, (uint32_t)v);
  buf_u32(b, (uint32_t)(v >> 32));
}
static inline void buf_f32(bw_buf *b, float f) {
  uint32_t v;
  memcpy(&v, &f, 4);
  buf_u32(b, v);
}
static inline void buf_f64(bw_buf *b, double f) {
  uint64_t v;
  memcpy(&v, &f, 8);
  buf_u64(b, v);
}

/* every byte of p[0 .. n) at file offset off, or -1 with errno */
static inline int write_all(int fd, const void *p, uint64_t n, uint64_t off) {
  const uint8_t *q = p;
  while (n) {
    const ssize_t w = pwrite(fd, q, n > (1u << 30) ? (1u << 30) : (size_t)n, (off_t)off);
    if (w < 0) {
      if (errno == EINTR) continue;
      return -1;
    }
    if (w == 0) {
      errno = EIO;
      return -1;
    }
    q += w;
    off += (uint64_t)w;
    n -= (uint64_t)w;
  }
  return 0;
}

/* the levels of a tree over n items with BW_NODE a node, bottom-up: cnt[l] items in nodes[l] nodes; returns the level count */
static inline int tree_levels(uint64_t n, uint64_t cnt[12], uint64_t nodes[12]) {
  int l = 0;
  cnt[0] = n;
  nodes[0] = n ? (n + BW_NODE - 1) / BW_NODE : 1;
  while (nodes[l] > 1) {
    cnt[l + 1] = nodes[l];
    nodes[l + 1] = (cnt[l + 1] + BW_NODE - 1) / BW_NODE;
    l++;
  }
  return l + 1;
}

static inline uint64_t chrom_tree_bytes(uint32_t n_refs, uint32_t key_size) {
  uint64_t cnt[12], nodes[12], bytes = 32;
  const int levels = tree_levels(n_refs, cnt, nodes);
  for (int l = 0; l < levels; l++) bytes += 4 * nodes[l] + cnt[l] * ((uint64_t)key_size + 8);
  return bytes;
}

typedef struct {
  const char *name;
  uint32_t id;
} bw_name;
static inline int by_name(const void *x, const void *y) { /* memcmp order of the zero-padded keys = the names as unsigned byte strings */
  const bw_name *a = x, *b = y;
  const int c = strcmp(a->name, b->name);
  return c ? c : (a->id > b->id) - (a->id < b->id);
}

/* the chromosome B+ tree at file offset `at` */
static inline int chrom_tree_put(bw_buf *b, uint32_t n_refs, uint32_t key_size, char *const *names, const uint32_t *lens, uint64_t at) {
  const uint32_t n = n_refs, key = key_size;
  const uint64_t item = (uint64_t)key + 8;
  uint64_t cnt[12], nodes[12], start[12];
  const int levels = tree_levels(n, cnt, nodes);
  bw_name *order = malloc((n ? n : 1) * sizeof *order);
  if (!order) return -1;
  for (uint32_t k = 0; k < n; k++) {
    order[k].name = names[k];
    order[k].id = k;
  }
  qsort(order, n, sizeof *order, by_name);
  buf_u32(b, 0x78CA8C91u);
  buf_u32(b, BW_NODE);
  buf_u32(b, key);
  buf_u32(b, 8);
  buf_u64(b, n);
  buf_u64(b, 0);
  start[levels - 1] = at + 32;
  for (int l = levels - 1; l > 0; l--) start[l - 1] = start[l] + 4 * nodes[l] + cnt[l] * item;
  for (int l = levels - 1; l >= 0; l--) {
    uint64_t span = 1; /* leaf items under one item of this level */
    for (int k = 0; k < l; k++) span *= BW_NODE;
    for (uint64_t j = 0; j < nodes[l]; j++) {
      const uint64_t lo = j * BW_NODE, hi = lo + BW_NODE < cnt[l] ? lo + BW_NODE : cnt[l];
      buf_u8(b, l == 0);
      buf_u8(b, 0);
      buf_u16(b, (uint16_t)(hi - lo));
      for (uint64_t i = lo; i < hi; i++) {
        const uint32_t id = order[i * span].id; /* the item's — or its subtree's first — contig */
        const size_t len = strlen(names[id]);
        uint8_t *q = buf_room(b, key);
        if (q) {
          memset(q, 0, key);
          memcpy(q, names[id], len);
        }
        if (l == 0) {
          buf_u32(b, id);
          buf_u32(b, lens[id]);
        } else {
          buf_u64(b, start[l - 1] + i * 4 + i * BW_NODE * item); /* child i: every node before it is full */
        }
      }
    }
  }
  free(order);
  return b->oom ? -1 : 0;
}

static inline int lex_less(uint32_t c, uint32_t p, uint32_t c2, uint32_t p2) { return c < c2 || (c == c2 && p < p2); }

/* an R-tree over it[0 .. n) at file offset `at`; end_off: where the data it indexes end; items_per_slot: the header's itemsPerSlot */
static inline int rtree_put(bw_buf *b, const rt_item *it, uint64_t n, uint64_t at, uint64_t end_off, uint32_t items_per_slot) {
  uint64_t cnt[12], nodes[12], start[12];
  const int levels = tree_levels(n, cnt, nodes);
  rt_item *bound[12] = {0}; /* per level, per node: its bounds (off, size unused) */
  int rc = 0;
  for (int l = 0; l < levels && !rc; l++) {
    bound[l] = malloc((size_t)nodes[l] * sizeof **bound);
    if (!bound[l]) {
      rc = -1;
      break;
    }
    const rt_item *src = l ? bound[l - 1] : it;
    for (uint64_t j = 0; j < nodes[l]; j++) {
      const uint64_t lo = j * BW_NODE, hi = lo + BW_NODE < cnt[l] ? lo + BW_NODE : cnt[l];
      rt_item v = {0, 0, 0, 0, 0, 0};
      for (uint64_t i = lo; i < hi; i++) {
        if (i == lo || lex_less(src[i].c0, src[i].s0, v.c0, v.s0)) v.c0 = src[i].c0, v.s0 = src[i].s0;
        if (i == lo || lex_less(v.c1, v.e1, src[i].c1, src[i].e1)) v.c1 = src[i].c1, v.e1 = src[i].e1;
      }
      bound[l][j] = v;
    }
  }
  if (!rc) {
    const rt_item all = bound[levels - 1][0];
    buf_u32(b, 0x2468ACE0u);
    buf_u32(b, BW_NODE);
    buf_u64(b, n);
    buf_u32(b, all.c0);
    buf_u32(b, all.s0);
    buf_u32(b, all.c1);
    buf_u32(b, all.e1);
    buf_u64(b, end_off);
    buf_u32(b, items_per_slot);
    buf_u32(b, 0);
    start[levels - 1] = at + 48;
    for (int l = levels - 1; l > 0; l--) start[l - 1] = start[l] + 4 * nodes[l] + 24 * cnt[l];
    for (int l = levels - 1; l >= 0; l--) {
      const rt_item *src = l ? bound[l - 1] : it;
      const uint64_t below = l > 1 ? 24 : 32; /* an item's size one level down */
      for (uint64_t j = 0; j < nodes[l]; j++) {
        const uint64_t lo = j * BW_NODE, hi = lo + BW_NODE < cnt[l] ? lo + BW_NODE : cnt[l];
        buf_u8(b, l == 0);
        buf_u8(b, 0);
        buf_u16(b, (uint16_t)(hi - lo));
        for (uint64_t i = lo; i < hi; i++) {
          buf_u32(b, src[i].c0);
          buf_u32(b, src[i].s0);
          buf_u32(b, src[i].c1);
          buf_u32(b, src[i].e1);
          if (l == 0) {
            buf_u64(b, src[i].off);
            buf_u64(b, src[i].size);
          } else {
            buf_u64(b, start[l - 1] + i * 4 + i * BW_NODE * below);
          }
        }
      }
    }
  }
  for (int l = 0; l < levels; l++) free(bound[l]);
  return rc || b->oom ? -1 : 0;
}

static inline int grow(void **p, uint64_t *cap, uint64_t need, size_t item) {
  if (need <= *cap) return 0;
  uint64_t c = *cap ? *cap : 1024;
  while (c < need) c *= 2;
  void *q = realloc(*p, (size_t)c * item);
  if (!q) return -1;
  *p = q;
  *cap = c;
  return 0;
}

#endif
