/*
 * patdev.hip — the per-read CpG pattern table (PAT) of a block (include/bscall_amd.h has the rule: COUNTS, SITE, BYTE, STATE of the read-level
 * CpG table; ORDINAL, PATTERN, PIECES, RECORD, TOTALS, LINE; csrc/pat.c the host form, which is the checker): per template the string of
 * methylated / unmethylated calls over the reference CpGs it covers, identical strings collapsed and counted — from the prepared templates,
 * their read bytes and the block's reference codes, while they are in HBM.
 *
 *   (the site pass and the exclusive scan are the read-level table's: bsc_dev_launch_cr_sites, cpgreadsdev.hip -> tile_mask[k], a bit per SITE
 *   of tile k = positions x + 64 k .., and tile_off[k] = the rank of the tile's first site = its ORDINAL)
 *   bsc_pat_slots_kernel  a lane per template, no read byte touched: the sites of its span, rank(end) - rank(start) from the masks, hold at
 *                         most ceil(sites / 64) pieces: the template's slots.  An exclusive scan (sort.hip) places them.
 *   bsc_pat_walk_kernel   one wave per template, its rounds the tiles its span touches in ascending order, through cr_round
 *                         (cpgreads_dev.h): ballots give the round's M and U masks by position.  One ds_permute moves every site's state
 *                         to the lane of its rank within the tile, two more ballots give the masks by ORDINAL, and the rest is the wave's
 *                         scalar arithmetic: the masks are shifted to their place behind f, the template's first state, and OR-ed into the
 *                         current piece's 64 C and 64 T bits; a round that starts the next piece flushes the one before.  A flush trims
 *                         (ctz / clz), interleaves the two masks into the record's 2-bit codes and writes one slot; '.' is what lies
 *                         between without a bit, so mate gaps cost nothing.  Unused slots get idx = 0xFFFFFFFF, which sorts last.  The
 *                         totals are wave-uniform counts that meet in the workgroup's LDS and leave it as integer atomic adds.
 *   (the sort by (idx, hi, lo) is rocPRIM's radix sort over the 24-byte slots: bsc_dev_sort_pat, sort.hip)
 *   bsc_pat_flags_kernel  a slot is a head where its key differs from the slot before it; an exclusive scan numbers the heads
 *   bsc_pat_heads_kernel  head r's slot index -> first[r]; first[heads] = the slots
 *   bsc_pat_recs_kernel   record r = the head's key with count = first[r + 1] - first[r], compacted into d_rec[< cap]; the run of unused
 *                         slots, the last, is no record; the record count and totals [0], [1]
 *   bsc_pat_size_kernel / the table's lines: the size pass, the scan and the write pass of epidev.hip over the 24-byte records, with the decimal
 *   bsc_pat_write_kernel  forms of methtext_dev.h and the placement of recstream_dev.h.
 *
 * Longest line: the contig's name (<= 255 bytes) + 98: tab, index <= 2^63 + 2^32 (19 digits; room for 20), tab, 64 characters, tab, count
 * (10 digits), '\n'.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "recstream_dev.h"
#include "methtext_dev.h"
#include "cpgreads_dev.h"

static_assert(sizeof(bsc_pat_rec) == 24, "bsc_pat_rec is 24 bytes");
static_assert(sizeof(bsc_template) == 40, "bsc_template is 40 bytes");
static_assert(BSC_PAT_MAX_SITES == 64, "a piece is the two 64-bit masks of a wave");

#define PT_WAVES 4u
#define PT_UNUSED 0xffffffffu

/* the template's fields and the positions [a, b) whose sites can have a state: p in [lo, hi) for C2T, [lo - 1, hi - 1) for G2A, within x .. y;
 * false: none (not converted, no read inside the buffer, outside the block) */
__device__ __forceinline__ bool pt_span(const bsc_template *tp, uint64_t seq_bytes, uint32_t x, uint32_t y, cr_tpl &t, uint64_t &a, uint64_t &b) {
  t.bs = tp->bs_strand;
  if (t.bs != 1u && t.bs != 2u) return false;
  uint64_t lo = ~0ull, hi = 0ull;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint64_t len = tp->len[k], off = tp->off[k];
    const bool have = len != 0u && off <= seq_bytes && len <= seq_bytes - off;
    t.pos[k] = tp->pos[k];
    t.end[k] = have ? t.pos[k] + len : t.pos[k]; /* (empty: no q lies in it) */
    t.off[k] = off;
    if (have) {
      lo = t.pos[k] < lo ? t.pos[k] : lo;
      hi = t.end[k] > hi ? t.end[k] : hi;
    }
  }
  if (hi == 0ull) return false;
  const uint64_t sh = t.bs == 2u ? 1u : 0u;
  a = lo >= sh ? lo - sh : 0ull;
  b = hi - sh;
  if (a < x) a = x;
  if (b > (uint64_t)y + 1u) b = (uint64_t)y + 1u;
  return a < b;
}

/* cnt[i] = the slots of template i (u64, for the scan); cnt[nr] = 0, so that the scan's last output is their sum; *n_sites = S */
extern "C" __global__ __launch_bounds__(256) void bsc_pat_slots_kernel(const bsc_template *__restrict__ tpl, uint32_t nr, uint64_t seq_bytes, uint32_t x,
                                                                       uint32_t y, uint32_t n_tiles, const uint32_t *__restrict__ tile_off,
                                                                       const unsigned long long *__restrict__ tile_mask,
                                                                       unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ n_sites) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cnt[nr] = 0ull;
    *n_sites = (uint64_t)tile_off[n_tiles - 1u] + (unsigned)__popcll(tile_mask[n_tiles - 1u]);
  }
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nr; i += (uint64_t)gridDim.x * 256u) {
    cr_tpl t;
    uint64_t a, b;
    unsigned long long slots = 0ull;
    if (pt_span(tpl + i, seq_bytes, x, y, t, a, b)) {
      const uint32_t oa = (uint32_t)(a - x), ob = (uint32_t)(b - 1u - x); /* both within the block: tiles < n_tiles */
      const unsigned ba = oa & 63u, bb = ob & 63u;
      const uint64_t ra = (uint64_t)tile_off[oa >> 6] + (unsigned)__popcll(tile_mask[oa >> 6] & ((1ull << ba) - 1ull));
      const uint64_t rb = (uint64_t)tile_off[ob >> 6] + (unsigned)__popcll(tile_mask[ob >> 6] & (bb == 63u ? ~0ull : (2ull << bb) - 1ull));
      slots = (rb - ra + (BSC_PAT_MAX_SITES - 1u)) / BSC_PAT_MAX_SITES;
    }
    cnt[i] = slots;
  }
}

/* bit k of v -> bit 2 k */
__device__ __forceinline__ unsigned long long pt_spread(uint32_t v) {
  unsigned long long s = v;
  s = (s | s << 16) & 0x0000ffff0000ffffull;
  s = (s | s << 8) & 0x00ff00ff00ff00ffull;
  s = (s | s << 4) & 0x0f0f0f0f0f0f0f0full;
  s = (s | s << 2) & 0x3333333333333333ull;
  s = (s | s << 1) & 0x5555555555555555ull;
  return s;
}

/* 32 sites' codes: bit j of h / l = the high / low bit of site j's code -> site j in bits 63 - 2 j, 62 - 2 j */
__device__ __forceinline__ unsigned long long pt_codes(uint32_t h, uint32_t l) { return pt_spread(__brev(h)) << 1 | pt_spread(__brev(l)); }

/* one 24-byte slot, as three 8-byte stores */
__device__ __forceinline__ void pt_store(bsc_pat_rec *__restrict__ o, uint32_t idx, uint32_t count, unsigned long long hi, unsigned long long lo) {
  unsigned long long *w = reinterpret_cast<unsigned long long *>(o);
  w[0] = (unsigned long long)idx | (unsigned long long)count << 32;
  w[1] = hi;
  w[2] = lo;
}

/* the piece's own counts, wave-uniform */
struct pt_acc {
  unsigned long long c, t, dot;
  unsigned n_out; /* slots written */
};

/* the piece `piece` (C and T bits by ordinal - f - 64 piece) into the template's next slot; nothing for a piece without a state */
__device__ __forceinline__ void pt_flush(unsigned long long C, unsigned long long T, uint32_t f, uint32_t piece, bsc_pat_rec *__restrict__ slots, uint64_t s0,
                                         uint64_t s1, unsigned lane, pt_acc &acc) {
  const unsigned long long any = C | T;
  if (!any) return;
  const unsigned first = (unsigned)__builtin_ctzll(any), n = 64u - (unsigned)__builtin_clzll(any) - first;
  const unsigned long long c = C >> first, t = T >> first, valid = n == 64u ? ~0ull : (1ull << n) - 1ull;
  /* codes: '.' 01, 'C' 10, 'T' 11 — the high bit is C | T, the low bit is not C */
  const unsigned long long h = c | t, l = ~c & valid;
  const uint64_t at = s0 + acc.n_out;
  if (lane == 0u && at < s1)
    pt_store(slots + at, f + piece * 64u + first, 1u, pt_codes((uint32_t)h, (uint32_t)l), pt_codes((uint32_t)(h >> 32), (uint32_t)(l >> 32)));
  acc.n_out++;
  acc.c += (unsigned)__popcll(C);
  acc.t += (unsigned)__popcll(T);
  acc.dot += n - (unsigned)__popcll(any);
}

extern "C" __global__ __launch_bounds__(256) void bsc_pat_walk_kernel(const bsc_template *__restrict__ tpl, uint32_t nr, const uint8_t *__restrict__ seq,
                                                                      uint64_t seq_bytes, uint32_t x, uint32_t y, unsigned min_qual, unsigned min_sites,
                                                                      const uint32_t *__restrict__ tile_off,
                                                                      const unsigned long long *__restrict__ tile_mask,
                                                                      const unsigned long long *__restrict__ slot_off, bsc_pat_rec *__restrict__ slots,
                                                                      unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long s_tot[5];
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  if (threadIdx.x < 5u) s_tot[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long w_tpl = 0, w_c = 0, w_t = 0, w_dot = 0, w_cut = 0; /* wave-uniform */
  for (uint64_t i = (uint64_t)blockIdx.x * PT_WAVES + wid; i < nr; i += (uint64_t)gridDim.x * PT_WAVES) {
    cr_tpl t;
    uint64_t a, b;
    if (!pt_span(tpl + i, seq_bytes, x, y, t, a, b)) continue; /* wave-uniform: one address a wave; such a template has no slot */
    const uint64_t s0 = slot_off[i], s1 = slot_off[i + 1u];
    const uint32_t tile_a = (uint32_t)((a - x) >> 6), tile_b = (uint32_t)((b - 1u - x) >> 6);
    pt_acc acc = {0ull, 0ull, 0ull, 0u};
    unsigned kt = 0u;
    bool have_f = false;
    uint32_t f = 0u, cur = 0u; /* the first state's ordinal; the current piece */
    unsigned long long C = 0ull, T = 0ull;
    for (uint32_t tile = tile_a; tile <= tile_b; tile++) {
      const unsigned long long m = tile_mask[tile];
      if (!m) continue;
      unsigned long long mm, mu;
      cr_round(t, seq, x, y, tile, m, lane, min_qual, mm, mu);
      if (!(mm | mu)) continue; /* no state in this round: dots, which are what no bit says */
      kt += (unsigned)__popcll(mm | mu);
      /* by position -> by rank within the tile: the sites' lanes to lanes 0 .. c - 1 in order, the others behind them (a permutation) */
      const unsigned r = (unsigned)__popcll(m & ((1ull << lane) - 1ull)), c = (unsigned)__popcll(m);
      const unsigned dest = ((m >> lane) & 1ull) ? r : c + (lane - r);
      const int got = __builtin_amdgcn_ds_permute((int)(dest << 2), (int)cr_state_at(mm, mu, lane));
      unsigned long long rm = __ballot(got & 1), ru = __ballot(got & 2);
      const uint32_t off = tile_off[tile];
      if (!have_f) {
        f = off + (unsigned)__builtin_ctzll(rm | ru);
        have_f = true;
      }
      uint32_t base; /* rank 0 of this tile lies at ordinal f + base */
      if (off < f) { /* the first round: the sites in front of f have no bit */
        rm >>= f - off;
        ru >>= f - off;
        base = 0u;
      } else base = off - f;
      const uint32_t piece = base >> 6;
      const unsigned sh = base & 63u;
      if (piece != cur) {
        pt_flush(C, T, f, cur, slots, s0, s1, lane, acc);
        cur = piece;
        C = T = 0ull;
      }
      C |= rm << sh;
      T |= ru << sh;
      const unsigned long long c2 = sh ? rm >> (64u - sh) : 0ull, t2 = sh ? ru >> (64u - sh) : 0ull; /* the tile's sites beyond the piece */
      if (c2 | t2) {
        pt_flush(C, T, f, cur, slots, s0, s1, lane, acc);
        cur = piece + 1u;
        C = c2;
        T = t2;
      }
    }
    pt_flush(C, T, f, cur, slots, s0, s1, lane, acc); /* (the last piece holds l: it has a state) */
    const bool gives = kt >= min_sites; /* min_sites >= 1: the launcher's */
    if (gives) {
      w_tpl++;
      w_c += acc.c;
      w_t += acc.t;
      w_dot += acc.dot;
      w_cut += cur > 0u;
    }
    /* the slots that hold no piece; those of a template below min_sites are taken back by the lane that wrote them */
    uint64_t used = s0 + acc.n_out < s1 ? s0 + acc.n_out : s1;
    if (!gives) {
      if (lane == 0u)
        for (uint64_t j = s0; j < used; j++) pt_store(slots + j, PT_UNUSED, 0u, 0ull, 0ull);
    }
    for (uint64_t j = used + lane; j < s1; j += 64u) pt_store(slots + j, PT_UNUSED, 0u, 0ull, 0ull);
  }
  if (lane == 0) {
    if (w_tpl) atomicAdd(&s_tot[0], w_tpl);
    if (w_c) atomicAdd(&s_tot[1], w_c);
    if (w_t) atomicAdd(&s_tot[2], w_t);
    if (w_dot) atomicAdd(&s_tot[3], w_dot);
    if (w_cut) atomicAdd(&s_tot[4], w_cut);
  }
  __syncthreads();
  if (threadIdx.x < 5u && s_tot[threadIdx.x]) atomicAdd(totals + 2u + threadIdx.x, s_tot[threadIdx.x]);
}

/* ---- heads and run lengths over the sorted slots ------------------------------------------------------------------------------------------------ */
__device__ __forceinline__ bool pt_same(const bsc_pat_rec *__restrict__ a, const bsc_pat_rec *__restrict__ b) {
  return a->idx == b->idx && a->hi == b->hi && a->lo == b->lo;
}

extern "C" __global__ __launch_bounds__(256) void bsc_pat_flags_kernel(const bsc_pat_rec *__restrict__ sorted, uint32_t n, uint32_t *__restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
    flag[i] = i == 0u || !pt_same(sorted + i, sorted + i - 1u) ? 1u : 0u;
}

/* first[r] = the slot of head r; first[heads] = n */
extern "C" __global__ __launch_bounds__(256) void bsc_pat_heads_kernel(uint32_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ num,
                                                                       uint32_t *__restrict__ first) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    if (flag[i]) first[num[i]] = (uint32_t)i;
    if (i == n - 1u) first[(uint64_t)num[i] + flag[i]] = n;
  }
}

extern "C" __global__ __launch_bounds__(256) void bsc_pat_recs_kernel(const bsc_pat_rec *__restrict__ sorted, uint32_t n, const uint32_t *__restrict__ flag,
                                                                      const uint32_t *__restrict__ num, const uint32_t *__restrict__ first,
                                                                      bsc_pat_rec *__restrict__ rec, uint64_t cap, unsigned long long *__restrict__ n_rec,
                                                                      unsigned long long *__restrict__ totals) {
  const uint64_t heads = (uint64_t)num[n - 1u] + flag[n - 1u];
  const bool tail = sorted[n - 1u].idx == PT_UNUSED; /* the last run is that of the unused slots */
  const uint64_t recs = heads - (tail ? 1u : 0u);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *n_rec = recs;
    totals[0] = recs;
    totals[1] = tail ? first[heads - 1u] : n;
  }
  const uint64_t room = recs < cap ? recs : cap;
  for (uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < room; r += (uint64_t)gridDim.x * 256u) {
    const uint32_t i = first[r];
    const bsc_pat_rec *k = sorted + i;
    pt_store(rec + r, k->idx, first[r + 1u] - i, k->hi, k->lo);
  }
}

/* ---- the table's lines ----------------------------------------------------------------------------------------------------------------------- */
#define PT_CONTIG_MAX 255u
#define PT_LINE_MAX (PT_CONTIG_MAX + 1u + 21u + 65u + 11u) /* the name, its tab, the index, the pattern, the count, each with its separator */
#define PT_IMG 4096u
#define PT_PARTS 8u
static_assert(PT_LINE_MAX == PT_CONTIG_MAX + 98u, "the longest line is the contig's name + 98");
static_assert(PT_IMG >= (RS_LANES / PT_PARTS) * PT_LINE_MAX && PT_IMG % 16u == 0u, "an eighth of a tile of the longest lines must fit the wave's image");
static_assert(PT_LINE_MAX <= 0xffffu, "a line's length is kept in 16 bits");

struct pt_text_args {
  const bsc_pat_rec *rec;
  const unsigned long long *n_rec;
  uint64_t max_rec;
  uint64_t index_base1;  /* index_base + 1 */
  uint32_t clen1;        /* the contig's name and the tab behind it, bytes */
  uint32_t contig_w[64]; /* those bytes, zero padded */
};

__device__ __forceinline__ uint64_t pt_clamp_n(const pt_text_args &a) {
  const unsigned long long n = *a.n_rec;
  return n < a.max_rec ? n : a.max_rec;
}

struct pt_line {
  uint32_t idx, count;
  unsigned long long hi, lo;
};

__device__ __forceinline__ void pt_load(pt_line &h, const pt_text_args &a, uint64_t i) {
  const unsigned long long *p = reinterpret_cast<const unsigned long long *>(a.rec + i); /* 24-byte records, 8-byte aligned */
  const unsigned long long w = p[0];
  h.idx = (uint32_t)w;
  h.count = (uint32_t)(w >> 32);
  h.hi = p[1];
  h.lo = p[2];
}

/* eight digits of v < 10^8, zero padded */
template <class S>
__device__ __forceinline__ void pt_put_dec8(S &s, uint32_t v) {
  uint64_t acc = 0ull;
  for (int i = 0; i < 8; i++) {
    const uint32_t q = v / 10u;
    acc = acc << 8 | (uint64_t)('0' + (v - q * 10u));
    v = q;
  }
  s.bytes(acc, 8u);
}

/* any v in decimal and sep behind it (mb_put_dec stops at 10^16; the index reaches 2^63 + 2^32) */
template <class S>
__device__ __forceinline__ void pt_put_dec64(S &s, uint64_t v, unsigned sep) {
  if (v < 10000000000000000ull) {
    mb_put_dec(s, v, sep);
    return;
  }
  const uint64_t top = v / 10000000000000000ull, low = v - top * 10000000000000000ull; /* top <= 1844 */
  unsigned n;
  const uint64_t c = mb_dec8((uint32_t)top, n);
  s.bytes(c, n);
  pt_put_dec8(s, (uint32_t)(low / 100000000ull));
  pt_put_dec8(s, (uint32_t)(low % 100000000ull));
  s.u8(sep);
}

/* the characters of 32 sites' codes, eight at a time; stops at the code 0.  Returns false where it stopped */
template <class S>
__device__ __forceinline__ bool pt_put_sites(S &s, unsigned long long w) {
#pragma unroll 1
  for (int g = 0; g < 4; g++) {
    const unsigned grp = (unsigned)(w >> (48 - 16 * g)) & 0xffffu;
    uint64_t bits = 0ull;
    unsigned n = 0u;
    for (; n < 8u; n++) {
      const unsigned code = (grp >> (14u - 2u * n)) & 3u;
      if (!code) break;
      bits |= (uint64_t)(code == 2u ? 'C' : (code == 3u ? 'T' : '.')) << (8u * n);
    }
    if (n) s.bytes(bits, n);
    if (n < 8u) return false;
  }
  return true;
}

template <class S>
__device__ __forceinline__ void pt_emit_line(S &s, const pt_line &h, uint64_t index_base1, const uint32_t *contig_w, unsigned clen1) {
  s.words(contig_w, clen1);
  pt_put_dec64(s, index_base1 + h.idx, '\t');
  if (pt_put_sites(s, h.hi)) pt_put_sites(s, h.lo);
  s.u8('\t');
  mb_put_dec(s, h.count, '\n');
}

/* tile_bytes[n_tiles] = 0 (so that the scan's last output is the stream's length); *lines += the lines */
extern "C" __global__ __launch_bounds__(256) void bsc_pat_size_kernel(pt_text_args a, uint32_t n_tiles, unsigned long long *__restrict__ tile_bytes,
                                                                      uint16_t *__restrict__ line_len, unsigned long long *__restrict__ lines) {
  __shared__ unsigned long long s_lines;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n = pt_clamp_n(a);
  if (threadIdx.x == 0) s_lines = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  __syncthreads();
  unsigned long long n_lines = 0ull; /* wave-uniform */
  for (uint32_t tile = blockIdx.x * PT_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * PT_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    if (i < n) {
      pt_line h;
      pt_load(h, a, i);
      mb_count_sink c = {0u};
      pt_emit_line(c, h, a.index_base1, a.contig_w, a.clen1);
      len = c.len;
    }
    if (i < a.max_rec) line_len[i] = (uint16_t)len;
    n_lines += (unsigned)__popcll(__ballot(len != 0u));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
  if (lane == 0 && n_lines) atomicAdd(&s_lines, n_lines);
  __syncthreads();
  if (threadIdx.x == 0 && s_lines) atomicAdd(lines, s_lines);
}

extern "C" __global__ __launch_bounds__(256) void bsc_pat_write_kernel(pt_text_args a, uint32_t n_tiles, const unsigned long long *__restrict__ tile_off,
                                                                       const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out, uint64_t out_cap,
                                                                       unsigned long long *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[PT_WAVES][PT_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = pt_clamp_n(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = tile_off[n_tiles];
  for (uint32_t tile = blockIdx.x * PT_WAVES + wid; tile < n_tiles; tile += gridDim.x * PT_WAVES) {
    if ((uint64_t)tile * 64u >= n) break; /* wave-uniform; later tiles of this wave lie further out still */
    const uint64_t g_tile = tile_off[tile], g_end = tile_off[tile + 1u];
    if (g_end == g_tile) continue; /* no line in this tile */
    if (g_end > out_cap) continue; /* the host reports the overflow from *total */
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const unsigned len = i < n ? line_len[i] : 0u;
    pt_line h;
    if (len) pt_load(h, a, i);
    unsigned excl, t_all;
    const unsigned inc = rs_wave_excl_scan(len, excl, t_all);
    const unsigned parts = rs_pick_parts<PT_IMG, PT_PARTS>(inc);
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = rs_lane(inc, step * (ps + 1u) - 1u); /* one past its last */
      const bool mine = len && excl >= b0 && excl < b1;
      const uint64_t g0 = g_tile + b0;
      const unsigned ph = (unsigned)(g0 & 15u);
      if (mine) {
        mb_write_sink w = {img + ph + (excl - b0), 0u};
        pt_emit_line(w, h, a.index_base1, a.contig_w, a.clen1);
      }
      rs_wave_sync();
      rs_copy_out(img, out + (g0 - ph), lane, rs_copy_ranges(ph, b1 - b0));
      rs_wave_sync();
      b0 = b1;
    }
  }
}

extern "C" int bsc_dev_scan_u32(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */
extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream);
extern "C" int bsc_dev_sort_pat(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream);

static unsigned bsc_pat_grid(uint64_t n_items, unsigned per_group, int num_cus) {
  uint64_t grid = (n_items + per_group - 1u) / per_group;
  /* eight workgroups of four waves a CU fill its SIMDs */
  if (grid > (uint64_t)num_cus * 8u) grid = (uint64_t)num_cus * 8u;
  return grid ? (unsigned)grid : 1u;
}

/* the slot pass and its scan behind bsc_dev_launch_cr_sites: slot_off[nr + 1] (u64; [nr] = the block's slots), *n_sites = S.  cnt: nr + 1 u64;
 * scan_tmp: bsc_dev_scan_tmp_bytes_u64 of nr + 1.  n = y - x + 1 > 0, nr < 2^32 - 1 */
extern "C" int bsc_dev_launch_pat_slots(const void *tpl, uint32_t nr, uint64_t seq_bytes, uint32_t x, uint32_t y, const void *tile_off, const void *tile_mask,
                                        void *cnt, void *slot_off, void *scan_tmp, size_t scan_tmp_bytes, void *n_sites, int num_cus, void *stream) {
  const uint32_t n_tiles = (uint32_t)(((uint64_t)(y - x) + 64u) / 64u);
  hipLaunchKernelGGL(bsc_pat_slots_kernel, dim3(bsc_pat_grid(nr, 256u, num_cus)), dim3(256), 0, (hipStream_t)stream, (const bsc_template *)tpl, nr, seq_bytes,
                     x, y, n_tiles, (const uint32_t *)tile_off, (const unsigned long long *)tile_mask, (unsigned long long *)cnt,
                     (unsigned long long *)n_sites);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return bsc_dev_scan_u64(cnt, slot_off, nr + 1u, scan_tmp, scan_tmp_bytes, stream);
}

/* the walk into slots[n_slots] (n_slots = slot_off[nr] > 0, waited for by the caller), the sort into `sorted`, the heads and the records:
 * rec[min(count, cap)], *n_rec, totals[0 .. 6] (the caller zeroes [2 .. 6]).  flag, num: n_slots u32; first: n_slots + 1 u32; scan_tmp:
 * bsc_dev_scan_tmp_bytes of n_slots; sort_tmp: bsc_dev_sort_pat_tmp_bytes of n_slots */
extern "C" int bsc_dev_launch_pat_walk(const void *tpl, uint32_t nr, const void *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, uint32_t min_qual,
                                       uint32_t min_sites, const void *tile_off, const void *tile_mask, const void *slot_off, uint32_t n_slots, void *slots,
                                       void *sorted, void *sort_tmp, size_t sort_tmp_bytes, void *flag, void *num, void *first, void *scan_tmp,
                                       size_t scan_tmp_bytes, void *rec, uint64_t cap, void *n_rec, void *totals, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bsc_pat_walk_kernel, dim3(bsc_pat_grid(nr, PT_WAVES, num_cus)), dim3(256), 0, s, (const bsc_template *)tpl, nr, (const uint8_t *)seq,
                     seq_bytes, x, y, min_qual, min_sites > 1u ? min_sites : 1u, (const uint32_t *)tile_off, (const unsigned long long *)tile_mask,
                     (const unsigned long long *)slot_off, (bsc_pat_rec *)slots, (unsigned long long *)totals);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  int rc = bsc_dev_sort_pat(slots, sorted, n_slots, sort_tmp, sort_tmp_bytes, stream);
  if (rc) return rc;
  const unsigned grid = bsc_pat_grid(n_slots, 256u, num_cus);
  hipLaunchKernelGGL(bsc_pat_flags_kernel, dim3(grid), dim3(256), 0, s, (const bsc_pat_rec *)sorted, n_slots, (uint32_t *)flag);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((rc = bsc_dev_scan_u32(flag, num, n_slots, scan_tmp, scan_tmp_bytes, stream))) return rc;
  hipLaunchKernelGGL(bsc_pat_heads_kernel, dim3(grid), dim3(256), 0, s, n_slots, (const uint32_t *)flag, (const uint32_t *)num, (uint32_t *)first);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bsc_pat_recs_kernel, dim3(grid), dim3(256), 0, s, (const bsc_pat_rec *)sorted, n_slots, (const uint32_t *)flag, (const uint32_t *)num,
                     (const uint32_t *)first, (bsc_pat_rec *)rec, cap, (unsigned long long *)n_rec, (unsigned long long *)totals);
  return (int)hipGetLastError();
}

/*
 * rec[min(*n_rec, max_rec)] -> out[<= out_cap] lines; totals2[0] = the stream's length (also when it exceeds out_cap: then only the tiles that fit
 * whole are written), totals2[1] += lines (the caller zeroes it).  contig: the name, contig_len (1 .. 255) bytes, checked by the caller.
 * tile_bytes / tile_off: max_rec / 64 (rounded up) + 1 u64 each; line_len: max_rec u16; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of the tiles + 1.
 */
extern "C" int bsc_dev_launch_pat_text(const void *rec, const void *n_rec, uint64_t max_rec, const char *contig, uint32_t contig_len, uint64_t index_base,
                                       void *tile_bytes, void *tile_off, void *line_len, void *scan_tmp, size_t scan_tmp_bytes, void *out, uint64_t out_cap,
                                       void *totals2, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!contig_len || contig_len > PT_CONTIG_MAX) return (int)hipErrorInvalidValue;
  pt_text_args a;
  a.rec = (const bsc_pat_rec *)rec;
  a.n_rec = (const unsigned long long *)n_rec;
  a.max_rec = max_rec;
  a.index_base1 = index_base + 1u;
  a.clen1 = contig_len + 1u;
  for (int k = 0; k < 64; k++) a.contig_w[k] = 0u;
  __builtin_memcpy(a.contig_w, contig, contig_len);
  ((char *)a.contig_w)[contig_len] = '\t';
  const uint64_t nt64 = (max_rec + 63u) / 64u;
  if (nt64 > 0x7fffffffull) return (int)hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)nt64;
  const unsigned grid = bsc_pat_grid(n_tiles, PT_WAVES, num_cus);
  hipLaunchKernelGGL(bsc_pat_size_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (unsigned long long *)tile_bytes, (uint16_t *)line_len,
                     (unsigned long long *)totals2 + 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int rc = bsc_dev_scan_u64(tile_bytes, tile_off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_pat_write_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (const unsigned long long *)tile_off, (const uint16_t *)line_len,
                     (uint8_t *)out, out_cap, (unsigned long long *)totals2);
  return (int)hipGetLastError();
}
