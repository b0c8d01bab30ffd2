/*
 * epidev.hip — the epiallele table of a block (include/bscall_amd.h has the rule: COUNTS, SITE, BYTE, STATE of the read-level CpG table; WINDOW,
 * PATTERN, RECORD, TOTALS, LINE; csrc/epi.c the host form, which is the checker): per window of four consecutive reference CpGs the templates
 * that show each of the 16 methylation patterns — from the prepared templates, their read bytes and the block's reference codes, while they
 * are in HBM.
 *
 *   (the site pass and the exclusive scan are the read-level table's: bsc_dev_launch_cr_sites, cpgreadsdev.hip -> tile_mask[k], a bit per SITE
 *   of tile k = positions x + 64 k .., and tile_off[k] = the rank of the tile's first site)
 *   bsc_epi_init_kernel   one wave per tile: a lane per site of rank r <= S - 4 writes its window's record {pos, span, 0 x 16} at r (r < the
 *                         room); span from the third set bit ahead, in the tile's mask or in the masks behind it; the count and totals[0]
 *   bsc_epi_walk_kernel   one wave per template, its rounds the tiles its span touches in ascending order, through cr_round
 *                         (cpgreads_dev.h): ballots give the round's M and U masks.  A lane that holds a site with a state owns the window
 *                         that ENDS there: the three states in front of it are those of the three set bits below its lane in the tile's
 *                         mask, and, where the tile has fewer, of the carry — the states of the last three sites in front of the round,
 *                         wave-uniform, handed on through rounds without a site and "none" in front of the span.  Four states, none of
 *                         them "none": one atomicAdd(&rec[rank - 3].c[code], 1u).  One sweep, every byte read once, no LDS strip and no
 *                         chunk border: a window across two, three or four tiles is the carry's.  Integer adds are exact in any order: the
 *                         output is a function of the input.  Observations and their M bits are counted per lane, the two template counts
 *                         per wave; they meet in the workgroup's LDS and leave it as four 64-bit atomic adds.
 *   bsc_epi_size_kernel / the table's lines: the size pass, the scan and the write pass of cpgreadsdev.hip over the 72-byte records, with the
 *   bsc_epi_write_kernel  decimal forms of methtext_dev.h and the placement of recstream_dev.h.
 *
 * Longest line: the contig's name (<= 255 bytes) + 214: tab, start (<= 10 digits), tab, end = pos + span + 1 <= 2^32 (10), tab, n <= 16 (2^32 - 1)
 * (11), tab, k <= 16 (2), sixteen times a tab and a count of at most ten digits, '\n'.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "recstream_dev.h"
#include "methtext_dev.h"
#include "cpgreads_dev.h"

static_assert(sizeof(bsc_epi_window) == 72, "bsc_epi_window is 72 bytes");
static_assert(sizeof(bsc_template) == 40, "bsc_template is 40 bytes");
static_assert(BSC_EPI_K == 4, "the walk keeps three states in front of a site");

#define EP_WAVES 4u

/* the k-th (k >= 1) set bit of a, counted from bit 0; a has at least k */
__device__ __forceinline__ unsigned ep_kth_bit(unsigned long long a, unsigned k) {
  for (; k > 1u; k--) a &= a - 1ull;
  return (unsigned)__builtin_ctzll(a);
}

extern "C" __global__ __launch_bounds__(256) void bsc_epi_init_kernel(uint32_t x, uint32_t n_tiles, const uint32_t *__restrict__ tile_off,
                                                                      const unsigned long long *__restrict__ tile_mask,
                                                                      bsc_epi_window *__restrict__ win, uint64_t cap,
                                                                      unsigned long long *__restrict__ n_win, unsigned long long *__restrict__ totals) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t S = (uint64_t)tile_off[n_tiles - 1u] + (unsigned)__popcll(tile_mask[n_tiles - 1u]); /* the block's sites */
  const uint64_t nw = S >= BSC_EPI_K ? S - (BSC_EPI_K - 1u) : 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *n_win = nw;
    totals[0] = nw;
  }
  for (uint32_t tile = blockIdx.x * EP_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * EP_WAVES) {
    const unsigned long long m = tile_mask[tile];
    if (!((m >> lane) & 1ull)) continue;
    const uint64_t rank = (uint64_t)tile_off[tile] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (rank >= nw || rank >= cap) continue; /* no window starts at the last three sites; beyond the room: counted, not stored */
    /* the third site ahead: it exists, since rank + 3 < S */
    unsigned need = BSC_EPI_K - 1u;
    uint32_t span = 0u;
    const unsigned long long above = lane == 63u ? 0ull : m >> (lane + 1u);
    const unsigned have = (unsigned)__popcll(above);
    if (have >= need) span = ep_kth_bit(above, need) + 1u;
    else {
      need -= have;
      for (uint32_t t2 = tile + 1u; t2 < n_tiles; t2++) {
        const unsigned long long m2 = tile_mask[t2];
        const unsigned c2 = (unsigned)__popcll(m2);
        if (c2 >= need) {
          span = (t2 - tile) * 64u + ep_kth_bit(m2, need) - lane;
          break;
        }
        need -= c2;
      }
    }
    uint32_t *w = reinterpret_cast<uint32_t *>(win + rank);
    w[0] = x + tile * 64u + lane;
    w[1] = span;
#pragma unroll
    for (int k = 2; k < 18; k++) w[k] = 0u;
  }
}

/* the states of the up to three sites at the highest set bits of `bits`, two bits each, the highest site's in bits 0 .. 1; n: how many */
__device__ __forceinline__ unsigned ep_top3(unsigned long long mm, unsigned long long mu, unsigned long long bits, unsigned &n) {
  unsigned packed = 0u;
  n = 0u;
#pragma unroll
  for (int k = 0; k < 3; k++)
    if (bits) {
      const unsigned j = 63u - (unsigned)__builtin_clzll(bits);
      bits &= ~(1ull << j);
      packed |= cr_state_at(mm, mu, j) << (2 * k);
      n++;
    }
  return packed;
}

/* one round: the adds of the lanes whose window ends in this tile.  carry: the states of the last three sites in front of the round, two bits
 * each, the nearest in bits 0 .. 1, in and out (wave-uniform).  Returns the ballot of the lanes that gave a pattern */
__device__ __forceinline__ unsigned long long ep_add_round(unsigned long long m, unsigned long long mm, unsigned long long mu, uint32_t off, unsigned lane,
                                                           bsc_epi_window *__restrict__ win, uint64_t cap, unsigned &carry, unsigned long long &l_bits) {
  const unsigned st = cr_state_at(mm, mu, lane);
  bool gave = false;
  if (st) { /* (a state only where the mask has a bit) */
    const unsigned long long below = m & ((1ull << lane) - 1ull);
    /* the three states in front: the tile's own sites below the lane, the carry behind them */
    unsigned n_own;
    const unsigned own = ep_top3(mm, mu, below, n_own);
    const unsigned prev = ((carry << (2u * n_own)) | own) & 63u;
    const unsigned s1 = prev & 3u, s2 = (prev >> 2) & 3u, s3 = prev >> 4;
    if (s1 && s2 && s3) { /* (three sites with a state in front: the rank is 3 at least) */
      const unsigned code = (unsigned)(s3 == 1u) | (unsigned)(s2 == 1u) << 1 | (unsigned)(s1 == 1u) << 2 | (unsigned)(st == 1u) << 3;
      const uint64_t rank = (uint64_t)off + (unsigned)__popcll(below) - 3u; /* the window's first site */
      if (rank < cap) atomicAdd(&win[rank].c[code], 1u);
      l_bits += (unsigned)__popc(code);
      gave = true;
    }
  }
  unsigned n_top;
  const unsigned top = ep_top3(mm, mu, m, n_top);
  carry = ((carry << (2u * n_top)) | top) & 63u;
  return __ballot(gave);
}

extern "C" __global__ __launch_bounds__(256) void bsc_epi_walk_kernel(const bsc_template *__restrict__ tpl, uint32_t nr, const uint8_t *__restrict__ seq,
                                                                      uint64_t seq_bytes, uint32_t x, uint32_t y, unsigned min_qual,
                                                                      const uint32_t *__restrict__ tile_off,
                                                                      const unsigned long long *__restrict__ tile_mask,
                                                                      bsc_epi_window *__restrict__ win, uint64_t cap,
                                                                      unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long s_tot[4];
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  if (threadIdx.x < 4u) s_tot[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long l_obs = 0, l_bits = 0; /* per lane */
  unsigned long long t_gave = 0, t_k4 = 0; /* wave-uniform */
  for (uint32_t i = blockIdx.x * EP_WAVES + wid; i < nr; i += gridDim.x * EP_WAVES) {
    const bsc_template *tp = tpl + i; /* one address a wave: the loads are broadcast */
    cr_tpl t;
    t.bs = tp->bs_strand;
    if (t.bs != 1u && t.bs != 2u) continue; /* wave-uniform */
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
    if (hi == 0ull) continue;
    /* the sites that can have a state: p in [lo, hi) for C2T, [lo - 1, hi - 1) for G2A, within x .. y */
    const uint64_t sh = t.bs == 2u ? 1u : 0u;
    uint64_t a = lo >= sh ? lo - sh : 0ull, b = hi - sh; /* [a, b) */
    if (a < x) a = x;
    if (b > (uint64_t)y + 1u) b = (uint64_t)y + 1u;
    if (a >= b) continue;
    const uint32_t tile_a = (uint32_t)((a - x) >> 6), tile_b = (uint32_t)((b - 1u - x) >> 6);
    unsigned kt = 0u, carry = 0u; /* the sites in front of the span have no state */
    bool any = false;
    for (uint32_t tile = tile_a; tile <= tile_b; tile++) {
      const unsigned long long m = tile_mask[tile];
      if (!m) continue; /* (a round without a site hands the carry on) */
      unsigned long long mm, mu;
      cr_round(t, seq, x, y, tile, m, lane, min_qual, mm, mu);
      kt += (unsigned)__popcll(mm | mu);
      const unsigned long long g = ep_add_round(m, mm, mu, tile_off[tile], lane, win, cap, carry, l_bits);
      l_obs += (g >> lane) & 1ull;
      any = any || g != 0ull;
    }
    t_gave += any;
    t_k4 += kt >= BSC_EPI_K;
  }
  /* once a kernel: the lanes' two counts and the wave's two into the workgroup's four (LDS atomics), then four global ones */
  if (l_obs) atomicAdd(&s_tot[0], l_obs);
  if (l_bits) atomicAdd(&s_tot[2], l_bits);
  if (lane == 0) {
    if (t_gave) atomicAdd(&s_tot[1], t_gave);
    if (t_k4) atomicAdd(&s_tot[3], t_k4);
  }
  __syncthreads();
  if (threadIdx.x < 4u && s_tot[threadIdx.x]) atomicAdd(totals + 1u + threadIdx.x, s_tot[threadIdx.x]);
}

/* ---- the table's lines ----------------------------------------------------------------------------------------------------------------------- */
#define EP_CONTIG_MAX 255u
#define EP_LINE_MAX (EP_CONTIG_MAX + 1u + 11u + 11u + 12u + 3u + 16u * 11u) /* the name, its tab, start, end, n, k, sixteen counts; the last separator is '\n' */
#define EP_IMG 4096u
#define EP_PARTS 8u
static_assert(EP_LINE_MAX == EP_CONTIG_MAX + 214u, "the longest line is the contig's name + 214");
static_assert(EP_IMG >= (RS_LANES / EP_PARTS) * EP_LINE_MAX && EP_IMG % 16u == 0u, "an eighth of a tile of the longest lines must fit the wave's image");
static_assert(EP_LINE_MAX <= 0xffffu, "a line's length is kept in 16 bits");

struct ep_text_args {
  const bsc_epi_window *win;
  const unsigned long long *n_win;
  uint64_t max_win;
  uint32_t min_cov;      /* max(1, min_cov) */
  uint32_t clen1;        /* the contig's name and the tab behind it, bytes */
  uint32_t contig_w[64]; /* those bytes, zero padded */
};

__device__ __forceinline__ uint64_t ep_clamp_n(const ep_text_args &a) {
  const unsigned long long n = *a.n_win;
  return n < a.max_win ? n : a.max_win;
}

/* what a line needs of record i beside its counts: pos, span, n = the sum of the sixteen counts, kinds = the counts above 0 */
struct ep_head {
  uint32_t pos, span, kinds;
  uint64_t n;
};

__device__ __forceinline__ void ep_load(ep_head &h, const ep_text_args &a, uint64_t i) {
  const uint2 *p = reinterpret_cast<const uint2 *>(a.win + i); /* 72-byte records, 8-byte aligned */
  const uint2 v0 = p[0];
  h.pos = v0.x;
  h.span = v0.y;
  h.n = 0ull;
  h.kinds = 0u;
#pragma unroll
  for (int k = 1; k < 9; k++) {
    const uint2 v = p[k];
    h.n += (uint64_t)v.x + v.y;
    h.kinds += (unsigned)(v.x != 0u) + (unsigned)(v.y != 0u);
  }
}

/* the line of record i; the sixteen counts are read again where they are written: a loop, not sixteen copies of the decimal conversion, and no
 * record in registers (the loads hit the lines ep_load has just brought in) */
template <class S>
__device__ __forceinline__ void ep_emit_line(S &s, const ep_head &h, const uint32_t *__restrict__ c, const uint32_t *contig_w, unsigned clen1) {
  s.words(contig_w, clen1);
  mb_put_dec(s, (uint64_t)(h.pos - 1u), '\t');
  mb_put_dec(s, (uint64_t)h.pos + (uint64_t)h.span + 1ull, '\t');
  mb_put_dec(s, h.n, '\t'); /* < 2^36: within mb_put_dec's 10^16 */
  mb_put_dec(s, h.kinds, '\t');
#pragma unroll 1
  for (int k = 0; k < 16; k++) mb_put_dec(s, c[k], k == 15 ? (unsigned)'\n' : (unsigned)'\t');
}

/* tile_bytes[n_tiles] = 0 (so that the scan's last output is the stream's length); *lines += the lines */
extern "C" __global__ __launch_bounds__(256) void bsc_epi_size_kernel(ep_text_args a, uint32_t n_tiles, unsigned long long *__restrict__ tile_bytes,
                                                                      uint16_t *__restrict__ line_len, unsigned long long *__restrict__ lines) {
  __shared__ unsigned long long s_lines;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n = ep_clamp_n(a);
  if (threadIdx.x == 0) s_lines = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  __syncthreads();
  unsigned long long n_lines = 0ull; /* wave-uniform */
  for (uint32_t tile = blockIdx.x * EP_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * EP_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    if (i < n) {
      ep_head h;
      ep_load(h, a, i);
      if (h.n >= a.min_cov) {
        mb_count_sink c = {0u};
        ep_emit_line(c, h, a.win[i].c, a.contig_w, a.clen1);
        len = c.len;
      }
    }
    if (i < a.max_win) line_len[i] = (uint16_t)len;
    n_lines += (unsigned)__popcll(__ballot(len != 0u));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
  if (lane == 0 && n_lines) atomicAdd(&s_lines, n_lines);
  __syncthreads();
  if (threadIdx.x == 0 && s_lines) atomicAdd(lines, s_lines);
}

extern "C" __global__ __launch_bounds__(256) void bsc_epi_write_kernel(ep_text_args a, uint32_t n_tiles, const unsigned long long *__restrict__ tile_off,
                                                                       const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out, uint64_t out_cap,
                                                                       unsigned long long *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[EP_WAVES][EP_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = ep_clamp_n(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = tile_off[n_tiles];
  for (uint32_t tile = blockIdx.x * EP_WAVES + wid; tile < n_tiles; tile += gridDim.x * EP_WAVES) {
    if ((uint64_t)tile * 64u >= n) break; /* wave-uniform; later tiles of this wave lie further out still */
    const uint64_t g_tile = tile_off[tile], g_end = tile_off[tile + 1u];
    if (g_end == g_tile) continue; /* no line in this tile */
    if (g_end > out_cap) continue; /* the host reports the overflow from *total */
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const unsigned len = i < n ? line_len[i] : 0u;
    ep_head h;
    if (len) ep_load(h, a, i);
    unsigned excl, t_all;
    const unsigned inc = rs_wave_excl_scan(len, excl, t_all);
    const unsigned parts = rs_pick_parts<EP_IMG, EP_PARTS>(inc);
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = rs_lane(inc, step * (ps + 1u) - 1u); /* one past its last */
      const bool mine = len && excl >= b0 && excl < b1;
      const uint64_t g0 = g_tile + b0;
      const unsigned ph = (unsigned)(g0 & 15u);
      if (mine) {
        mb_write_sink w = {img + ph + (excl - b0), 0u};
        ep_emit_line(w, h, a.win[i].c, a.contig_w, a.clen1);
      }
      rs_wave_sync();
      rs_copy_out(img, out + (g0 - ph), lane, rs_copy_ranges(ph, b1 - b0));
      rs_wave_sync();
      b0 = b1;
    }
  }
}

extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

static unsigned bsc_epi_grid(uint64_t n_items, int num_cus) {
  uint64_t grid = (n_items + EP_WAVES - 1u) / EP_WAVES;
  /* eight workgroups of four waves a CU fill its SIMDs */
  if (grid > (uint64_t)num_cus * 8u) grid = (uint64_t)num_cus * 8u;
  return grid ? (unsigned)grid : 1u;
}

/* the records' heads behind bsc_dev_launch_cr_sites: win[min(count, cap)] = {pos, span, 0 ..}; *n_win = totals[0] = the count; n = y - x + 1 > 0 */
extern "C" int bsc_dev_launch_epi_init(uint32_t x, uint32_t n, const void *tile_off, const void *tile_mask, void *win, uint64_t cap, void *n_win,
                                       void *totals, int num_cus, void *stream) {
  const uint32_t n_tiles = (uint32_t)(((uint64_t)n + 63u) / 64u);
  hipLaunchKernelGGL(bsc_epi_init_kernel, dim3(bsc_epi_grid(n_tiles, num_cus)), dim3(256), 0, (hipStream_t)stream, x, n_tiles, (const uint32_t *)tile_off,
                     (const unsigned long long *)tile_mask, (bsc_epi_window *)win, cap, (unsigned long long *)n_win, (unsigned long long *)totals);
  return (int)hipGetLastError();
}

/* the walk behind them: the counters of win[<= cap], totals[1 .. 4] += (the caller zeroes them) */
extern "C" int bsc_dev_launch_epi_walk(const void *tpl, uint32_t nr, const void *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, uint32_t min_qual,
                                       const void *tile_off, const void *tile_mask, void *win, uint64_t cap, void *totals, int num_cus, void *stream) {
  if (nr == 0) return 0;
  hipLaunchKernelGGL(bsc_epi_walk_kernel, dim3(bsc_epi_grid(nr, num_cus)), dim3(256), 0, (hipStream_t)stream, (const bsc_template *)tpl, nr,
                     (const uint8_t *)seq, seq_bytes, x, y, min_qual, (const uint32_t *)tile_off, (const unsigned long long *)tile_mask,
                     (bsc_epi_window *)win, cap, (unsigned long long *)totals);
  return (int)hipGetLastError();
}

/*
 * win[min(*n_win, max_win)] -> out[<= out_cap] lines; totals2[0] = the stream's length (also when it exceeds out_cap: then only the tiles that fit
 * whole are written), totals2[1] += lines (the caller zeroes it).  contig: the name, contig_len (1 .. 255) bytes, checked by the caller.
 * tile_bytes / tile_off: max_win / 64 (rounded up) + 1 u64 each; line_len: max_win u16; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of the tiles + 1.
 */
extern "C" int bsc_dev_launch_epi_text(const void *win, const void *n_win, uint64_t max_win, const char *contig, uint32_t contig_len, uint32_t min_cov,
                                       void *tile_bytes, void *tile_off, void *line_len, void *scan_tmp, size_t scan_tmp_bytes, void *out, uint64_t out_cap,
                                       void *totals2, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!contig_len || contig_len > EP_CONTIG_MAX) return (int)hipErrorInvalidValue;
  ep_text_args a;
  a.win = (const bsc_epi_window *)win;
  a.n_win = (const unsigned long long *)n_win;
  a.max_win = max_win;
  a.min_cov = min_cov > 1u ? min_cov : 1u;
  a.clen1 = contig_len + 1u;
  for (int k = 0; k < 64; k++) a.contig_w[k] = 0u;
  __builtin_memcpy(a.contig_w, contig, contig_len);
  ((char *)a.contig_w)[contig_len] = '\t';
  const uint64_t nt64 = (max_win + 63u) / 64u;
  if (nt64 > 0x7fffffffull) return (int)hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)nt64;
  const unsigned grid = bsc_epi_grid(n_tiles, num_cus);
  hipLaunchKernelGGL(bsc_epi_size_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (unsigned long long *)tile_bytes, (uint16_t *)line_len,
                     (unsigned long long *)totals2 + 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int rc = bsc_dev_scan_u64(tile_bytes, tile_off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_epi_write_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (const unsigned long long *)tile_off, (const uint16_t *)line_len,
                     (uint8_t *)out, out_cap, (unsigned long long *)totals2);
  return (int)hipGetLastError();
}
