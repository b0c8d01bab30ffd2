/*
 * cpgreadsdev.hip — the read-level CpG concordance table of a block (include/bscall_amd.h has the rule: COUNTS, SITE, BYTE, STATE, RECORD,
 * TOTALS, LINE; csrc/cpgreads.c the host form, which is the checker): per reference CpG the templates that read it methylated / unmethylated,
 * the eligible and the discordant ones among them, and the 2x2 table with the reference-next CpG — from the prepared templates, their read
 * bytes and the block's reference codes, while they are in HBM.
 *
 *   bsc_cr_site_kernel    one wave per tile of 64 positions (tile k = positions x + 64 k ..): two reference codes a lane, the tile's ballot
 *                         -> tile_mask[k] (a bit per SITE), tile_cnt[k]
 *   (exclusive scan of the tile counts: bsc_dev_scan_u32, sort.hip -> tile_off[k] = the rank of the tile's first site)
 *   bsc_cr_init_kernel    one wave per tile: a lane per site writes its record {pos, dist, 0 ..} at its rank (rank < the room); dist from
 *                         the next set bit of the tile's mask or the first set bit of the masks behind it; the count and totals[0]
 *   bsc_cr_walk_kernel    one wave per template, its rounds the tiles its span touches, lanes own the tile's positions.  A lane whose bit
 *                         of the tile's mask is set loads BYTE itself — at p for a C2T template, at p + 1 for a G2A one, so a site whose C is
 *                         lane 63 needs nothing of the next round — and ballots give the round's M and U masks.  Sweep 1 adds up k_t, has-M
 *                         and has-U over the rounds; sweep 2 runs from the span's last tile to its first, the state of the site at NEXT
 *                         taken from the lane of the next set bit of the tile's mask, or carried in from the round behind (through rounds
 *                         that hold no site; "none" past the span's end), and adds m / u, e, d and the pair count with u32 integer atomics
 *                         at the site's rank = tile_off + the bits of the mask below the lane.  A span of at most CR_KEEP tiles keeps its
 *                         masks in registers between the sweeps and reads no byte twice; a longer one evaluates them again.  Integer adds
 *                         are exact in any order: the output is a function of the input.  Six totals stay in the wave's registers and leave
 *                         the workgroup as six 64-bit atomic adds.
 *   bsc_cr_size_kernel /  the table's lines: the size pass, the scan and the write pass of methdev.hip over the records, with the decimal
 *   bsc_cr_write_kernel   forms of methtext_dev.h and the placement of recstream_dev.h.
 *
 * Longest line: the contig's name (<= 255 bytes) + 122: eleven numbers of at most ten digits (end = pos + 1 <= 2^32), eleven tabs and '\n'.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "recstream_dev.h"
#include "methtext_dev.h"
#include "cpgreads_dev.h"

static_assert(sizeof(bsc_cpg_reads_site) == 40, "bsc_cpg_reads_site is 40 bytes");
static_assert(sizeof(bsc_template) == 40, "bsc_template is 40 bytes");

#define CR_WAVES 4u
#define CR_KEEP 8u /* spans of up to this many tiles (a pair of 2 x 150 bases with an insert of 500 touches 8 or 9) keep their masks between the sweeps */

extern "C" __global__ __launch_bounds__(256) void bsc_cr_site_kernel(const uint8_t *__restrict__ ref, uint32_t n, uint32_t n_tiles,
                                                                     uint32_t *__restrict__ tile_cnt, unsigned long long *__restrict__ tile_mask) {
  const unsigned lane = threadIdx.x & 63u;
  for (uint32_t tile = blockIdx.x * CR_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * CR_WAVES) {
    const uint32_t i = tile * 64u + lane;
    const bool site = i < n && ref[i] == 2 && ref[i + 1u] == 3; /* ref holds n + 2 codes */
    const unsigned long long m = __ballot(site);
    if (lane == 0) {
      tile_cnt[tile] = (uint32_t)__popcll(m);
      tile_mask[tile] = m;
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void bsc_cr_init_kernel(uint32_t x, uint32_t n_tiles, const uint32_t *__restrict__ tile_off,
                                                                     const unsigned long long *__restrict__ tile_mask,
                                                                     bsc_cpg_reads_site *__restrict__ sites, uint64_t cap,
                                                                     unsigned long long *__restrict__ n_sites, unsigned long long *__restrict__ totals) {
  const unsigned lane = threadIdx.x & 63u;
  for (uint32_t tile = blockIdx.x * CR_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * CR_WAVES) {
    const unsigned long long m = tile_mask[tile];
    const uint32_t off = tile_off[tile];
    if (tile == n_tiles - 1u && lane == 0) {
      const unsigned long long cnt = (unsigned long long)off + (unsigned)__popcll(m);
      *n_sites = cnt;
      totals[0] = cnt;
    }
    if (!((m >> lane) & 1ull)) continue;
    const uint64_t rank = (uint64_t)off + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (rank >= cap) continue; /* counted, not stored */
    const uint32_t pos = x + tile * 64u + lane;
    uint32_t dist = 0u;
    const unsigned long long above = lane == 63u ? 0ull : m >> (lane + 1u);
    if (above) dist = (uint32_t)__builtin_ctzll(above) + 1u;
    else
      for (uint32_t t2 = tile + 1u; t2 < n_tiles; t2++) {
        const unsigned long long m2 = tile_mask[t2];
        if (m2) {
          dist = (t2 - tile) * 64u + (uint32_t)__builtin_ctzll(m2) - lane;
          break;
        }
      }
    uint32_t *w = reinterpret_cast<uint32_t *>(sites + rank);
    w[0] = pos;
    w[1] = dist;
#pragma unroll
    for (int k = 2; k < 10; k++) w[k] = 0u;
  }
}

/* sweep 2 of one round: the adds of the lanes that hold a state; carry: the state of the first site behind this round, in and out.
 * Returns the number of pairs counted (wave-uniform) */
__device__ __forceinline__ unsigned cr_add_round(unsigned long long m, unsigned long long mm, unsigned long long mu, uint32_t off, unsigned lane, bool elig,
                                                 bool disc, bsc_cpg_reads_site *__restrict__ sites, uint64_t cap, unsigned &carry) {
  const unsigned st = cr_state_at(mm, mu, lane);
  unsigned nxt = 0u;
  if (st) {
    const unsigned long long above = lane == 63u ? 0ull : m >> (lane + 1u);
    nxt = above ? cr_state_at(mm, mu, lane + 1u + (unsigned)__builtin_ctzll(above)) : carry;
    const uint64_t rank = (uint64_t)off + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (rank < cap) {
      uint32_t *w = reinterpret_cast<uint32_t *>(sites + rank);
      atomicAdd(w + 2u + (st - 1u), 1u); /* m, u */
      if (elig) atomicAdd(w + 4u, 1u);
      if (disc) atomicAdd(w + 5u, 1u);
      if (nxt) atomicAdd(w + 6u + 2u * (st - 1u) + (nxt - 1u), 1u); /* mm, mu, um, uu */
    }
  }
  const unsigned pairs = (unsigned)__popcll(__ballot(st != 0u && nxt != 0u));
  if (m) carry = cr_state_at(mm, mu, (unsigned)__builtin_ctzll(m)); /* (a round without a site hands the carry on) */
  return pairs;
}

extern "C" __global__ __launch_bounds__(256) void bsc_cr_walk_kernel(const bsc_template *__restrict__ tpl, uint32_t nr, const uint8_t *__restrict__ seq,
                                                                     uint64_t seq_bytes, uint32_t x, uint32_t y, unsigned min_qual, uint32_t min_sites,
                                                                     const uint32_t *__restrict__ tile_off,
                                                                     const unsigned long long *__restrict__ tile_mask,
                                                                     bsc_cpg_reads_site *__restrict__ sites, uint64_t cap,
                                                                     unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long s_tot[CR_WAVES][6];
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  unsigned long long t_m = 0, t_u = 0, t_pairs = 0, t_any = 0, t_elig = 0, t_disc = 0; /* wave-uniform */
  for (uint32_t i = blockIdx.x * CR_WAVES + wid; i < nr; i += gridDim.x * CR_WAVES) {
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
    const uint32_t tile_a = (uint32_t)((a - x) >> 6), tile_b = (uint32_t)((b - 1u - x) >> 6), nt = tile_b - tile_a + 1u;
    unsigned kt = 0u;
    bool has_m = false, has_u = false;
    if (nt <= CR_KEEP) {
      unsigned long long ms[CR_KEEP], mms[CR_KEEP], mus[CR_KEEP];
#pragma unroll
      for (unsigned r = 0; r < CR_KEEP; r++) {
        ms[r] = mms[r] = mus[r] = 0ull;
        if (r < nt) {
          ms[r] = tile_mask[tile_a + r];
          if (ms[r]) cr_round(t, seq, x, y, tile_a + r, ms[r], lane, min_qual, mms[r], mus[r]);
          kt += (unsigned)__popcll(mms[r] | mus[r]);
          has_m = has_m || mms[r] != 0ull;
          has_u = has_u || mus[r] != 0ull;
        }
      }
      if (!kt) continue;
      const bool elig = kt >= min_sites, disc = elig && has_m && has_u;
      unsigned carry = 0u;
#pragma unroll
      for (int r = (int)CR_KEEP - 1; r >= 0; r--)
        if ((unsigned)r < nt) t_pairs += cr_add_round(ms[r], mms[r], mus[r], tile_off[tile_a + (unsigned)r], lane, elig, disc, sites, cap, carry);
#pragma unroll
      for (unsigned r = 0; r < CR_KEEP; r++) {
        t_m += (unsigned)__popcll(mms[r]);
        t_u += (unsigned)__popcll(mus[r]);
      }
      t_any++;
      t_elig += elig;
      t_disc += disc;
    } else {
      for (uint32_t tile = tile_a; tile <= tile_b; tile++) {
        const unsigned long long m = tile_mask[tile];
        if (!m) continue;
        unsigned long long mm, mu;
        cr_round(t, seq, x, y, tile, m, lane, min_qual, mm, mu);
        kt += (unsigned)__popcll(mm | mu);
        has_m = has_m || mm != 0ull;
        has_u = has_u || mu != 0ull;
        t_m += (unsigned)__popcll(mm);
        t_u += (unsigned)__popcll(mu);
      }
      if (!kt) continue;
      const bool elig = kt >= min_sites, disc = elig && has_m && has_u;
      unsigned carry = 0u;
      for (uint32_t tile = tile_b;; tile--) {
        const unsigned long long m = tile_mask[tile];
        if (m) {
          unsigned long long mm, mu;
          cr_round(t, seq, x, y, tile, m, lane, min_qual, mm, mu);
          t_pairs += cr_add_round(m, mm, mu, tile_off[tile], lane, elig, disc, sites, cap, carry);
        }
        if (tile == tile_a) break;
      }
      t_any++;
      t_elig += elig;
      t_disc += disc;
    }
  }
  if (lane == 0) {
    unsigned long long *t = s_tot[wid];
    t[0] = t_m;
    t[1] = t_u;
    t[2] = t_pairs;
    t[3] = t_any;
    t[4] = t_elig;
    t[5] = t_disc;
  }
  __syncthreads();
  if (threadIdx.x < 6u) {
    unsigned long long v = 0ull;
    for (unsigned w = 0; w < CR_WAVES; w++) v += s_tot[w][threadIdx.x];
    if (v) atomicAdd(totals + 1u + threadIdx.x, v);
  }
}

/* ---- the table's lines ----------------------------------------------------------------------------------------------------------------------- */
#define CR_CONTIG_MAX 255u
#define CR_LINE_MAX (CR_CONTIG_MAX + 122u)
#define CR_IMG 4096u
#define CR_PARTS 8u
static_assert(CR_IMG >= (RS_LANES / CR_PARTS) * CR_LINE_MAX && CR_IMG % 16u == 0u, "an eighth of a tile of the longest lines must fit the wave's image");
static_assert(CR_LINE_MAX <= 0xffffu, "a line's length is kept in 16 bits");

struct cr_text_args {
  const bsc_cpg_reads_site *sites;
  const unsigned long long *n_sites;
  uint64_t max_sites;
  uint32_t min_cov;      /* max(1, min_cov) */
  uint32_t clen1;        /* the contig's name and the tab behind it, bytes */
  uint32_t contig_w[64]; /* those bytes, zero padded */
};

struct cr_rec {
  uint32_t w[10];
};

__device__ __forceinline__ uint64_t cr_clamp_n(const cr_text_args &a) {
  const unsigned long long n = *a.n_sites;
  return n < a.max_sites ? n : a.max_sites;
}

__device__ __forceinline__ void cr_load(cr_rec &r, const cr_text_args &a, uint64_t i) {
  const uint2 *p = reinterpret_cast<const uint2 *>(a.sites + i); /* 40-byte records, 8-byte aligned */
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const uint2 v = p[k];
    r.w[2 * k] = v.x;
    r.w[2 * k + 1] = v.y;
  }
}

template <class S>
__device__ __forceinline__ void cr_emit_line(S &s, const cr_rec &r, const uint32_t *contig_w, unsigned clen1) {
  s.words(contig_w, clen1);
  mb_put_dec(s, (uint64_t)(r.w[0] - 1u), '\t');
  mb_put_dec(s, (uint64_t)r.w[0] + 1ull, '\t');
  mb_put_dec(s, r.w[2], '\t'); /* m */
  mb_put_dec(s, r.w[3], '\t'); /* u */
  mb_put_dec(s, r.w[4], '\t'); /* e */
  mb_put_dec(s, r.w[5], '\t'); /* d */
  mb_put_dec(s, r.w[1], '\t'); /* dist */
  mb_put_dec(s, r.w[6], '\t');
  mb_put_dec(s, r.w[7], '\t');
  mb_put_dec(s, r.w[8], '\t');
  mb_put_dec(s, r.w[9], '\n');
}

/* tile_bytes[n_tiles] = 0 (so that the scan's last output is the stream's length); *lines += the lines */
extern "C" __global__ __launch_bounds__(256) void bsc_cr_size_kernel(cr_text_args a, uint32_t n_tiles, unsigned long long *__restrict__ tile_bytes,
                                                                     uint16_t *__restrict__ line_len, unsigned long long *__restrict__ lines) {
  __shared__ unsigned long long s_lines;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n = cr_clamp_n(a);
  if (threadIdx.x == 0) s_lines = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  __syncthreads();
  unsigned long long n_lines = 0ull; /* wave-uniform */
  for (uint32_t tile = blockIdx.x * CR_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * CR_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    if (i < n) {
      cr_rec r;
      cr_load(r, a, i);
      if ((uint64_t)r.w[2] + r.w[3] >= a.min_cov) {
        mb_count_sink c = {0u};
        cr_emit_line(c, r, a.contig_w, a.clen1);
        len = c.len;
      }
    }
    if (i < a.max_sites) line_len[i] = (uint16_t)len;
    n_lines += (unsigned)__popcll(__ballot(len != 0u));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
  if (lane == 0 && n_lines) atomicAdd(&s_lines, n_lines);
  __syncthreads();
  if (threadIdx.x == 0 && s_lines) atomicAdd(lines, s_lines);
}

extern "C" __global__ __launch_bounds__(256) void bsc_cr_write_kernel(cr_text_args a, uint32_t n_tiles, const unsigned long long *__restrict__ tile_off,
                                                                      const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out, uint64_t out_cap,
                                                                      unsigned long long *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[CR_WAVES][CR_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = cr_clamp_n(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = tile_off[n_tiles];
  for (uint32_t tile = blockIdx.x * CR_WAVES + wid; tile < n_tiles; tile += gridDim.x * CR_WAVES) {
    if ((uint64_t)tile * 64u >= n) break; /* wave-uniform; later tiles of this wave lie further out still */
    const uint64_t g_tile = tile_off[tile], g_end = tile_off[tile + 1u];
    if (g_end == g_tile) continue; /* no line in this tile */
    if (g_end > out_cap) continue; /* the host reports the overflow from *total */
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const unsigned len = i < n ? line_len[i] : 0u;
    cr_rec r;
    if (len) cr_load(r, a, i);
    unsigned excl, t_all;
    const unsigned inc = rs_wave_excl_scan(len, excl, t_all);
    const unsigned parts = rs_pick_parts<CR_IMG, CR_PARTS>(inc);
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = rs_lane(inc, step * (ps + 1u) - 1u); /* one past its last */
      const bool mine = len && excl >= b0 && excl < b1;
      const uint64_t g0 = g_tile + b0;
      const unsigned ph = (unsigned)(g0 & 15u);
      if (mine) {
        mb_write_sink w = {img + ph + (excl - b0), 0u};
        cr_emit_line(w, r, a.contig_w, a.clen1);
      }
      rs_wave_sync();
      rs_copy_out(img, out + (g0 - ph), lane, rs_copy_ranges(ph, b1 - b0));
      rs_wave_sync();
      b0 = b1;
    }
  }
}

extern "C" int bsc_dev_scan_u32(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */
extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

static unsigned bsc_cr_grid(uint64_t n_items, int num_cus) {
  uint64_t grid = (n_items + CR_WAVES - 1u) / CR_WAVES;
  /* eight workgroups of four waves a CU fill its SIMDs */
  if (grid > (uint64_t)num_cus * 8u) grid = (uint64_t)num_cus * 8u;
  return grid ? (unsigned)grid : 1u;
}

/* the site pass and the scan: tile_cnt / tile_off (n + 63) / 64 words, tile_mask as many u64; n = y - x + 1 > 0, ref: n + 2 codes */
extern "C" int bsc_dev_launch_cr_sites(const void *ref, uint32_t n, void *tile_cnt, void *tile_off, void *tile_mask, void *scan_tmp, size_t scan_tmp_bytes,
                                       int num_cus, void *stream) {
  const uint32_t n_tiles = (uint32_t)(((uint64_t)n + 63u) / 64u);
  hipLaunchKernelGGL(bsc_cr_site_kernel, dim3(bsc_cr_grid(n_tiles, num_cus)), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)ref, n, n_tiles,
                     (uint32_t *)tile_cnt, (unsigned long long *)tile_mask);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return bsc_dev_scan_u32(tile_cnt, tile_off, n_tiles, scan_tmp, scan_tmp_bytes, stream);
}

/* the records' heads: sites[min(count, cap)] = {pos, dist, 0 ..}; *n_sites = totals[0] = the count */
extern "C" int bsc_dev_launch_cr_init(uint32_t x, uint32_t n, const void *tile_off, const void *tile_mask, void *sites, uint64_t cap, void *n_sites,
                                      void *totals, int num_cus, void *stream) {
  const uint32_t n_tiles = (uint32_t)(((uint64_t)n + 63u) / 64u);
  hipLaunchKernelGGL(bsc_cr_init_kernel, dim3(bsc_cr_grid(n_tiles, num_cus)), dim3(256), 0, (hipStream_t)stream, x, n_tiles, (const uint32_t *)tile_off,
                     (const unsigned long long *)tile_mask, (bsc_cpg_reads_site *)sites, cap, (unsigned long long *)n_sites, (unsigned long long *)totals);
  return (int)hipGetLastError();
}

/* the walk behind them: the counters of sites[<= cap], totals[1 .. 6] += (the caller zeroes them) */
extern "C" int bsc_dev_launch_cr_walk(const void *tpl, uint32_t nr, const void *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, uint32_t min_qual,
                                      uint32_t min_sites, const void *tile_off, const void *tile_mask, void *sites, uint64_t cap, void *totals, int num_cus,
                                      void *stream) {
  if (nr == 0) return 0;
  hipLaunchKernelGGL(bsc_cr_walk_kernel, dim3(bsc_cr_grid(nr, num_cus)), dim3(256), 0, (hipStream_t)stream, (const bsc_template *)tpl, nr,
                     (const uint8_t *)seq, seq_bytes, x, y, min_qual, min_sites, (const uint32_t *)tile_off, (const unsigned long long *)tile_mask,
                     (bsc_cpg_reads_site *)sites, cap, (unsigned long long *)totals);
  return (int)hipGetLastError();
}

/*
 * sites[min(*n_sites, max_sites)] -> out[<= out_cap] lines; totals2[0] = the stream's length (also when it exceeds out_cap: then only the tiles
 * that fit whole are written), totals2[1] += lines (the caller zeroes it).  contig: the name, contig_len (1 .. 255) bytes, checked by the
 * caller.  tile_bytes / tile_off: max_sites / 64 (rounded up) + 1 u64 each; line_len: max_sites u16; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of the
 * tiles + 1.
 */
extern "C" int bsc_dev_launch_cr_text(const void *sites, const void *n_sites, uint64_t max_sites, const char *contig, uint32_t contig_len, uint32_t min_cov,
                                      void *tile_bytes, void *tile_off, void *line_len, void *scan_tmp, size_t scan_tmp_bytes, void *out, uint64_t out_cap,
                                      void *totals2, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!contig_len || contig_len > CR_CONTIG_MAX) return (int)hipErrorInvalidValue;
  cr_text_args a;
  a.sites = (const bsc_cpg_reads_site *)sites;
  a.n_sites = (const unsigned long long *)n_sites;
  a.max_sites = max_sites;
  a.min_cov = min_cov > 1u ? min_cov : 1u;
  a.clen1 = contig_len + 1u;
  for (int k = 0; k < 64; k++) a.contig_w[k] = 0u;
  __builtin_memcpy(a.contig_w, contig, contig_len);
  ((char *)a.contig_w)[contig_len] = '\t';
  const uint64_t nt64 = (max_sites + 63u) / 64u;
  if (nt64 > 0x7fffffffull) return (int)hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)nt64;
  const unsigned grid = bsc_cr_grid(n_tiles, num_cus);
  hipLaunchKernelGGL(bsc_cr_size_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (unsigned long long *)tile_bytes, (uint16_t *)line_len,
                     (unsigned long long *)totals2 + 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int rc = bsc_dev_scan_u64(tile_bytes, tile_off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_cr_write_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (const unsigned long long *)tile_off, (const uint16_t *)line_len,
                     (uint8_t *)out, out_cap, (unsigned long long *)totals2);
  return (int)hipGetLastError();
}
