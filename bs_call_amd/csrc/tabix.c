/*
 * tabix.c — the index of a BGZF-compressed methylation table (BED text), a .tbi or a .csi file, made while the table is written: the host
 * half of bsc_tbx_* and the host form of the device scan (bsc_bed_entries_host over bedidx_core.h, the checker of beddev.hip).  Host code
 * only: the part that needs the BGZF writer's fields (bsc_tbx_open) is in bscall_api.c and reaches this file through tabix_int.h.
 * include/bscall_amd.h has the rule — entries, bins, chunks, the linear index, both files' layouts.
 *
 * What is kept per contig: every entry's extent in the logical stream with its bin, in file order (an extent that goes on in the bin of the
 * one before it extends that one at once: a contig of one window costs one extent), the first offset of every window, the first and the
 * last offset and the lines.  bsc_tbx_finish orders the extents by bin, joins what touches, fills the windows no line overlaps and turns
 * offsets into virtual offsets.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bedidx_core.h"
#include "../../include/bscall_amd.h"
#include "tabix_int.h"

int bsc_set_error(int code, const char *fmt, ...); /* bscall_api.c: the message bsc_last_error returns */

_Static_assert(sizeof(bed_run) == 24 && sizeof(bsc_bed_entry) == 24, "bsc_bed_entry is the walk's bed_run: 24 bytes");

#define TBX_MEMBER 0xFF00u
#define TBX_SLOT 0x10000u
#define TBX_UNSET UINT64_MAX

typedef struct {
  uint32_t bin;
  uint64_t u_beg, u_end;
} tbx_extent;
typedef struct {
  tbx_extent *x;
  uint64_t n, cap;
  uint64_t *lin; /* the first offset of a line that overlaps window w, TBX_UNSET where there is none (yet) */
  uint64_t n_lin, cap_lin;
  uint64_t first, last_end, n_lines;
  uint32_t last_wb;
} tbx_ref;
struct bsc_tbx {
  int kind, detached, have_members, min_shift, depth, n_refs;
  char *names; /* NUL-terminated, one after the other */
  size_t l_names;
  tbx_ref *ref;
  int32_t last_tid;
  uint64_t logical; /* detached: the stream's length so far; with a writer: its length at close */
  uint64_t *msize, n_msize;
  void *writer; /* the BGZF writer, while it is open */
  uint64_t (*w_logical)(void *);
  void (*w_unbind)(void *);
  struct bsc_tbx *next_open;
};
static pthread_mutex_t tbx_mu = PTHREAD_MUTEX_INITIALIZER;
static struct bsc_tbx *tbx_open_list;
static int tbx_is_open(const bsc_tbx *ix) {
  int found = 0;
  pthread_mutex_lock(&tbx_mu);
  for (const struct bsc_tbx *q = tbx_open_list; q && !found; q = q->next_open) found = q == ix;
  pthread_mutex_unlock(&tbx_mu);
  return found;
}

/* ---- the host form of the scan ------------------------------------------------------------------------------------------------------- */
int bsc_bed_entries_host(const void *stream, uint64_t n_bytes, const uint64_t *sync, uint32_t n_sync, int min_shift, bsc_bed_entry *entries,
                         uint64_t cap_entries, uint64_t totals[3]) {
  if (!totals || (!stream && n_bytes) || (!entries && cap_entries)) return bsc_set_error(BSC_ERR_ARG, "bsc_bed_entries_host: NULL argument");
  totals[0] = totals[1] = totals[2] = 0;
  if (min_shift < 0 || min_shift > 31) return bsc_set_error(BSC_ERR_ARG, "bsc_bed_entries_host: min_shift %d is not 0 .. 31", min_shift);
  if (!sync) n_sync = 1;
  uint32_t err = 0;
  uint64_t at = 0;
  for (uint32_t i = 0; i < n_sync; i++) {
    const uint64_t beg = sync ? sync[i] : 0, end = sync ? sync[i + 1u] : n_bytes;
    if (!(beg <= end && end <= n_bytes)) {
      err |= BED_ERR_INTERVAL;
      continue;
    }
    uint32_t l = 0;
    at += bed_walk((const uint8_t *)stream, beg, end, min_shift, (bed_run *)entries, at, cap_entries, &l, &err);
    totals[1] += l;
  }
  totals[0] = at;
  totals[2] = err;
  return BSC_OK;
}

/* ---- the writer ------------------------------------------------------------------------------------------------------------------------ */
int bsc_tbx_make_(const char *who, int kind, int min_shift, int n_refs, const char *const *names, const uint32_t *lens, bsc_tbx **out) {
  if (!out) return bsc_set_error(BSC_ERR_ARG, "%s: out is NULL", who);
  *out = NULL;
  if (kind != BSC_TBX_TBI && kind != BSC_TBX_CSI) return bsc_set_error(BSC_ERR_ARG, "%s: kind %d is neither BSC_TBX_TBI nor BSC_TBX_CSI", who, kind);
  if (kind == BSC_TBX_TBI && min_shift != 14) return bsc_set_error(BSC_ERR_ARG, "%s: a .tbi has min_shift 14 (and five levels), not %d: the csi kind takes others", who, min_shift);
  if (min_shift < 1 || min_shift > 31) return bsc_set_error(BSC_ERR_ARG, "%s: min_shift %d is not 1 .. 31", who, min_shift);
  if (n_refs < 0 || (n_refs && (!names || !lens))) return bsc_set_error(BSC_ERR_ARG, "%s: NULL argument", who);
  uint64_t longest = 0;
  size_t l_names = 0;
  for (int i = 0; i < n_refs; i++) {
    if (!names[i]) return bsc_set_error(BSC_ERR_ARG, "%s: contig %d has no name", who, i);
    l_names += strlen(names[i]) + 1;
    if (lens[i] > longest) longest = lens[i];
    if (kind == BSC_TBX_TBI && lens[i] > ((uint32_t)1 << 29))
      return bsc_set_error(BSC_ERR_ARG, "%s: contig %s has %u bases, a .tbi reaches 2^29: ask for a csi index", who, names[i], lens[i]);
  }
  bsc_tbx *ix = calloc(1, sizeof *ix);
  if (ix) ix->names = malloc(l_names ? l_names : 1);
  if (ix && ix->names) ix->ref = calloc((size_t)n_refs + 1, sizeof *ix->ref);
  if (!ix || !ix->names || !ix->ref) {
    if (ix) free(ix->names);
    free(ix);
    return bsc_set_error(BSC_ERR_NOMEM, "%s: out of host memory", who);
  }
  size_t at = 0;
  for (int i = 0; i < n_refs; i++) {
    const size_t l = strlen(names[i]) + 1;
    memcpy(ix->names + at, names[i], l);
    at += l;
  }
  ix->l_names = l_names;
  ix->kind = kind;
  ix->min_shift = min_shift;
  ix->n_refs = n_refs;
  ix->last_tid = -1;
  int depth = 5;
  if (kind == BSC_TBX_CSI) { /* the rule of bsc_csi_open: the levels that cover the longest contig + 256 */
    depth = 0;
    for (uint64_t s = (uint64_t)1 << min_shift; s < longest + 256u; s <<= 3) depth++;
  }
  ix->depth = depth;
  pthread_mutex_lock(&tbx_mu);
  ix->next_open = tbx_open_list;
  tbx_open_list = ix;
  pthread_mutex_unlock(&tbx_mu);
  *out = ix;
  return BSC_OK;
}

void bsc_tbx_bind_(bsc_tbx *ix, void *writer, uint64_t (*logical)(void *), void (*unbind)(void *)) {
  ix->writer = writer;
  ix->w_logical = logical;
  ix->w_unbind = unbind;
}

/* the writer's close: the index takes a copy of the members' sizes (a failed close leaves it without: bsc_tbx_finish refuses) */
void bsc_tbx_writer_closed_(bsc_tbx *ix, int rc, const uint64_t *msize, uint64_t n_msize, uint64_t logical) {
  if (!tbx_is_open(ix)) return;
  ix->writer = NULL;
  if (rc) return;
  ix->msize = malloc((size_t)(n_msize ? n_msize : 1) * 8);
  if (!ix->msize) return;
  if (n_msize) memcpy(ix->msize, msize, (size_t)n_msize * 8);
  ix->n_msize = n_msize;
  ix->logical = logical;
  ix->have_members = 1;
}

int bsc_tbx_open_detached(int kind, int min_shift, int n_refs, const char *const *names, const uint32_t *lens, uint64_t header_bytes, bsc_tbx **out) {
  const int rc = bsc_tbx_make_("bsc_tbx_open_detached", kind, min_shift, n_refs, names, lens, out);
  if (rc) return rc;
  (*out)->detached = 1;
  (*out)->logical = header_bytes;
  return BSC_OK;
}

int bsc_tbx_members(bsc_tbx *ix, const uint64_t *sizes, uint64_t n_members) {
  if (!tbx_is_open(ix)) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_members: not an open index (NULL, or closed)");
  if (!ix->detached || ix->have_members) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_members: the members' sizes come from the index's writer, or are here already");
  if (!sizes && n_members) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_members: sizes is NULL");
  if (n_members != (ix->logical + TBX_MEMBER - 1) / TBX_MEMBER)
    return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_members: %llu members, the stream's %llu bytes make %llu", (unsigned long long)n_members,
                         (unsigned long long)ix->logical, (unsigned long long)((ix->logical + TBX_MEMBER - 1) / TBX_MEMBER));
  for (uint64_t k = 0; k < n_members; k++)
    if (sizes[k] < 28 || sizes[k] > TBX_SLOT) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_members: member %llu has %llu bytes", (unsigned long long)k, (unsigned long long)sizes[k]);
  ix->msize = malloc((size_t)(n_members ? n_members : 1) * 8);
  if (!ix->msize) return bsc_set_error(BSC_ERR_NOMEM, "bsc_tbx_members: out of host memory");
  if (n_members) memcpy(ix->msize, sizes, (size_t)n_members * 8);
  ix->n_msize = n_members;
  ix->have_members = 1;
  return BSC_OK;
}

/* the bin of the windows wb .. wl under `depth` levels: the smallest level that holds both; -1: beyond the levels */
static int64_t tbx_bin(uint32_t wb, uint32_t wl, int depth) {
  if (3 * depth < 32 && wl >= ((uint32_t)1 << (3 * depth))) return -1;
  int k = 0;
  while (k <= depth && 3 * k < 32 && (wb >> (3 * k)) != (wl >> (3 * k))) k++;
  if (k > depth) return -1;
  if (3 * k >= 32) return depth == k ? 0 : -1;
  return (int64_t)((((uint64_t)1 << (3 * (depth - k))) - 1) / 7 + (wb >> (3 * k)));
}

int bsc_tbx_add(bsc_tbx *ix, int32_t tid, const bsc_bed_entry *entries, uint64_t n, uint64_t n_bytes) {
  if (!tbx_is_open(ix)) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: not an open index (NULL, or closed)");
  if (ix->have_members || (!ix->detached && !ix->writer)) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: the index's writer is closed");
  if (!entries && n) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: entries is NULL");
  if (tid < 0 || tid >= ix->n_refs) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: contig %d of %d", tid, ix->n_refs);
  if (tid < ix->last_tid) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: entries out of order: contig %d behind contig %d", tid, ix->last_tid);
  if ((n == 0) != (n_bytes == 0)) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: %llu entries for a table of %llu bytes", (unsigned long long)n, (unsigned long long)n_bytes);
  tbx_ref *r = &ix->ref[tid];
  uint32_t max_wl = 0;
  for (uint64_t i = 0; i < n; i++) { /* everything is checked before anything is added */
    const bsc_bed_entry *e = &entries[i];
    const uint32_t prev_wb = i ? entries[i - 1].win_beg : (r->n_lines ? r->last_wb : 0);
    if (!e->n_lines) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: entry %llu has no lines", (unsigned long long)i);
    if (e->win_last < e->win_beg) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: entry %llu ends in window %u, before its first, %u", (unsigned long long)i, e->win_last, e->win_beg);
    if (e->win_beg < prev_wb) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: entries out of order: window %u behind window %u", e->win_beg, prev_wb);
    if (tbx_bin(e->win_beg, e->win_last, ix->depth) < 0)
      return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: windows %u .. %u lie beyond the index's %d levels", e->win_beg, e->win_last, ix->depth);
    if (i ? e->u_beg <= entries[i - 1].u_beg : e->u_beg != 0)
      return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: entries out of order: entry %llu begins at %llu", (unsigned long long)i, (unsigned long long)e->u_beg);
    if (e->u_beg >= n_bytes) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_add: entry %llu begins at %llu of %llu bytes", (unsigned long long)i, (unsigned long long)e->u_beg, (unsigned long long)n_bytes);
    if (e->win_last > max_wl) max_wl = e->win_last;
  }
  if (r->n + n > r->cap) { /* all the room before anything changes */
    const uint64_t cap = (r->n + n) * 2 + 16;
    tbx_extent *q = realloc(r->x, (size_t)cap * sizeof *q);
    if (!q) return bsc_set_error(BSC_ERR_NOMEM, "bsc_tbx_add: out of host memory");
    r->x = q;
    r->cap = cap;
  }
  if (n && (uint64_t)max_wl + 1 > r->cap_lin) {
    const uint64_t cap = ((uint64_t)max_wl + 1) * 2;
    uint64_t *q = realloc(r->lin, (size_t)cap * 8);
    if (!q) return bsc_set_error(BSC_ERR_NOMEM, "bsc_tbx_add: out of host memory");
    r->lin = q;
    r->cap_lin = cap;
  }
  const uint64_t base = ix->detached ? ix->logical : ix->w_logical(ix->writer);
  for (uint64_t i = 0; i < n; i++) {
    const bsc_bed_entry *e = &entries[i];
    const uint64_t u_beg = base + e->u_beg, u_end = base + (i + 1 < n ? entries[i + 1].u_beg : n_bytes);
    const uint32_t bin = (uint32_t)tbx_bin(e->win_beg, e->win_last, ix->depth);
    if (r->n && r->x[r->n - 1].bin == bin && r->x[r->n - 1].u_end == u_beg) r->x[r->n - 1].u_end = u_end;
    else {
      const tbx_extent x = {bin, u_beg, u_end};
      r->x[r->n++] = x;
    }
    /* windows below n_lin that an earlier line reached are set; the starts do not descend, so the others below win_beg stay without */
    while (r->n_lin < (uint64_t)e->win_last + 1) r->lin[r->n_lin++] = TBX_UNSET;
    for (uint64_t w = e->win_last;; w--) { /* from the back: a window that is set ends it, everything before is set or out of reach */
      if (r->lin[w] != TBX_UNSET) break;
      r->lin[w] = u_beg;
      if (w == e->win_beg) break;
    }
    if (!r->n_lines) r->first = u_beg;
    r->n_lines += e->n_lines;
    r->last_end = u_end;
    r->last_wb = e->win_beg;
  }
  ix->last_tid = tid;
  if (ix->detached) ix->logical += n_bytes;
  return BSC_OK;
}

typedef struct {
  uint8_t *p;
  size_t n, cap;
  int bad;
} tbx_buf;
static void tbx_put(tbx_buf *b, const void *src, size_t n) {
  if (b->bad) return;
  if (b->n + n > b->cap) {
    const size_t cap = (b->n + n) * 2 + 256;
    uint8_t *q = realloc(b->p, cap);
    if (!q) {
      b->bad = 1;
      return;
    }
    b->p = q;
    b->cap = cap;
  }
  if (n) memcpy(b->p + b->n, src, n);
  b->n += n;
}
static void tbx_put32(tbx_buf *b, uint32_t v) {
  const uint8_t x[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
  tbx_put(b, x, 4);
}
static void tbx_put64(tbx_buf *b, uint64_t v) {
  tbx_put32(b, (uint32_t)v);
  tbx_put32(b, (uint32_t)(v >> 32));
}
static uint32_t tbx_crc32(const uint8_t *p, size_t n) { /* the gzip CRC, a bit at a time: an index is kilobytes */
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return c ^ 0xFFFFFFFFu;
}
static int tbx_by_bin(const void *a, const void *b) { /* by bin, then in file order */
  const tbx_extent *x = a, *y = b;
  if (x->bin != y->bin) return x->bin < y->bin ? -1 : 1;
  return x->u_beg < y->u_beg ? -1 : x->u_beg > y->u_beg;
}

long bsc_tbx_finish(bsc_tbx *ix, void *buf, uint64_t cap) {
  if (!tbx_is_open(ix)) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_finish: not an open index (NULL, or closed)");
  if (!ix->have_members) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_finish: the file is not closed yet (bsc_bgzf_close, or bsc_tbx_members, comes first)");
  if (!buf && cap) return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_finish: buf is NULL");
  if (ix->n_msize != (ix->logical + TBX_MEMBER - 1) / TBX_MEMBER)
    return bsc_set_error(BSC_ERR_ARG, "bsc_tbx_finish: %llu members for a stream of %llu bytes", (unsigned long long)ix->n_msize, (unsigned long long)ix->logical);
  uint64_t *coff = malloc((size_t)(ix->n_msize + 1) * 8);
  if (!coff) return bsc_set_error(BSC_ERR_NOMEM, "bsc_tbx_finish: out of host memory");
  coff[0] = 0;
  for (uint64_t k = 0; k < ix->n_msize; k++) coff[k + 1] = coff[k] + ix->msize[k];
#define VOFF(u) (coff[(u) / TBX_MEMBER] << 16 | (u) % TBX_MEMBER)
  const int csi = ix->kind == BSC_TBX_CSI;
  tbx_buf b = {NULL, 0, 0, 0};
  const uint32_t aux[7] = {0x10000, 1, 2, 3, '#', 0, (uint32_t)ix->l_names};
  if (csi) {
    tbx_put(&b, "CSI\1", 4);
    tbx_put32(&b, (uint32_t)ix->min_shift);
    tbx_put32(&b, (uint32_t)ix->depth);
    tbx_put32(&b, (uint32_t)(28 + ix->l_names));
    for (int k = 0; k < 7; k++) tbx_put32(&b, aux[k]);
    tbx_put(&b, ix->names, ix->l_names);
    tbx_put32(&b, (uint32_t)ix->n_refs);
  } else {
    tbx_put(&b, "TBI\1", 4);
    tbx_put32(&b, (uint32_t)ix->n_refs);
    for (int k = 0; k < 7; k++) tbx_put32(&b, aux[k]);
    tbx_put(&b, ix->names, ix->l_names);
  }
  const uint64_t pseudo = (((uint64_t)1 << (3 * (ix->depth + 1))) - 1) / 7 + 1;
  int rc = BSC_OK;
  for (int t = 0; t < ix->n_refs && !rc; t++) {
    const tbx_ref *r = &ix->ref[t];
    if (!r->n) {
      tbx_put32(&b, 0);
      if (!csi) tbx_put32(&b, 0);
      continue;
    }
    if (r->last_end > ix->logical) {
      rc = bsc_set_error(BSC_ERR_ARG, "bsc_tbx_finish: a block that ends at %llu was added, the file's stream has %llu bytes", (unsigned long long)r->last_end,
                         (unsigned long long)ix->logical);
      break;
    }
    /* the extents by bin, in file order inside a bin; what begins where the bin's last chunk ends extends it */
    tbx_extent *x = malloc((size_t)r->n * sizeof *x);
    uint64_t *lin = malloc((size_t)r->n_lin * 8);
    if (!x || !lin) {
      free(x);
      free(lin);
      rc = bsc_set_error(BSC_ERR_NOMEM, "bsc_tbx_finish: out of host memory");
      break;
    }
    memcpy(x, r->x, (size_t)r->n * sizeof *x);
    qsort(x, (size_t)r->n, sizeof *x, tbx_by_bin);
    uint64_t m = 0, n_bin = 0;
    for (uint64_t k = 0; k < r->n; k++) {
      if (m && x[m - 1].bin == x[k].bin && x[m - 1].u_end == x[k].u_beg) x[m - 1].u_end = x[k].u_end;
      else x[m++] = x[k];
    }
    for (uint64_t k = 0; k < m; k++) n_bin += !k || x[k].bin != x[k - 1].bin;
    /* the linear index: a window no line overlaps takes the next one's offset (the last window has a line) */
    memcpy(lin, r->lin, (size_t)r->n_lin * 8);
    for (uint64_t w = r->n_lin - 1; w-- > 0;)
      if (lin[w] == TBX_UNSET) lin[w] = lin[w + 1];
    tbx_put32(&b, (uint32_t)(n_bin + 1));
    for (uint64_t k = 0; k < m;) {
      uint64_t e = k;
      while (e < m && x[e].bin == x[k].bin) e++;
      tbx_put32(&b, x[k].bin);
      if (csi) { /* loffset: the linear rule at the bin's first window */
        uint64_t first = 0;
        for (int l = 0; l <= ix->depth; l++) {
          const uint64_t at0 = (((uint64_t)1 << (3 * l)) - 1) / 7;
          if (x[k].bin >= at0) first = (x[k].bin - at0) << (3 * (ix->depth - l));
        }
        tbx_put64(&b, VOFF(lin[first]));
      }
      tbx_put32(&b, (uint32_t)(e - k));
      for (; k < e; k++) {
        tbx_put64(&b, VOFF(x[k].u_beg));
        tbx_put64(&b, VOFF(x[k].u_end));
      }
    }
    tbx_put32(&b, (uint32_t)pseudo);
    if (csi) tbx_put64(&b, 0);
    tbx_put32(&b, 2);
    tbx_put64(&b, VOFF(r->first));
    tbx_put64(&b, VOFF(r->last_end));
    tbx_put64(&b, r->n_lines);
    tbx_put64(&b, 0);
    if (!csi) {
      tbx_put32(&b, (uint32_t)r->n_lin);
      for (uint64_t w = 0; w < r->n_lin; w++) tbx_put64(&b, VOFF(lin[w]));
    }
    free(x);
    free(lin);
  }
#undef VOFF
  tbx_put64(&b, 0); /* n_no_coor */
  free(coff);
  if (!rc && b.bad) rc = bsc_set_error(BSC_ERR_NOMEM, "bsc_tbx_finish: out of host memory");
  if (rc) {
    free(b.p);
    return rc;
  }
  /* the file: stored members of 0xFF00 bytes, the end-of-file marker */
  static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t nm = (b.n + TBX_MEMBER - 1) / TBX_MEMBER, need = b.n + nm * 31 + sizeof eof;
  if (buf && cap >= need) {
    uint8_t *o = buf;
    for (uint64_t k = 0; k < nm; k++) {
      const uint8_t *src = b.p + k * TBX_MEMBER;
      const uint32_t len = (uint32_t)(b.n - k * TBX_MEMBER < TBX_MEMBER ? b.n - k * TBX_MEMBER : TBX_MEMBER), size = 31 + len, crc = tbx_crc32(src, len);
      const uint8_t h[23] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(size - 1), (uint8_t)((size - 1) >> 8), 1,
                             (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)~len, (uint8_t)(~len >> 8)};
      memcpy(o, h, 23);
      memcpy(o + 23, src, len);
      const uint8_t tl[8] = {(uint8_t)crc, (uint8_t)(crc >> 8), (uint8_t)(crc >> 16), (uint8_t)(crc >> 24), (uint8_t)len, (uint8_t)(len >> 8), 0, 0};
      memcpy(o + 23 + len, tl, 8);
      o += size;
    }
    memcpy(o, eof, sizeof eof);
  }
  free(b.p);
  return (long)need;
}

void bsc_tbx_close(bsc_tbx *ix) {
  if (!tbx_is_open(ix)) return;
  pthread_mutex_lock(&tbx_mu);
  for (struct bsc_tbx **q = &tbx_open_list; *q; q = &(*q)->next_open)
    if (*q == ix) {
      *q = ix->next_open;
      break;
    }
  pthread_mutex_unlock(&tbx_mu);
  if (ix->writer && ix->w_unbind) ix->w_unbind(ix->writer);
  for (int t = 0; t < ix->n_refs; t++) {
    free(ix->ref[t].x);
    free(ix->ref[t].lin);
  }
  free(ix->ref);
  free(ix->names);
  free(ix->msize);
  free(ix);
}
