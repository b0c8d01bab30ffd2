/*
 * bigbeddev.hip — the bedMethyl table as bigBed items on the device: from the dense per-position arrays a block call left in HBM, the
 * block's stream of variable-length items, a 24-byte summary of every block of B items (with the block's byte offset in the stream) and
 * of every level-0 zoom window (include/bscall_amd.h has the rule; the host form csrc/bigbed.c is the checker).  The shape of the text
 * encoders (methdev.hip) for the stream, of the bigWig encoder (bigwigdev.hip) for the windows; integers only, no atomics, no result that
 * depends on an order.
 *
 *   bsc_bigbed_size_kernel     one wave per tile of 64 positions: the site predicate and the item's length per lane (the emitter over
 *                              the counting sink) -> item_len[i] (u8; 0 = no site), cnt[tile] sites, tbytes[tile] bytes (u64 each;
 *                              entry n_tiles = 0)
 *   (two exclusive scans, rocPRIM u64: sort.hip; the entries behind the last tile = n_sites, n_bytes)
 *   bsc_bigbed_write_kernel    one wave per tile that has a site: rank = off[tile] + the sites in lower lanes, byte offset = boff[tile]
 *                              + the lengths in lower lanes.  The site's lane stores its start at sites[rank] (a workspace: what the
 *                              window passes read); where the stream fits out_cap it writes its item — the 12-byte head and the text —
 *                              into the wave's LDS image of the tile's span of the stream at its byte offset, whatever its alignment,
 *                              and the wave copies the image out (recstream_dev.h).  Where the blocks fit blk_cap, the lane whose rank is
 *                              a multiple of B stores blocks[rank / B].{start, count, _pad, off}, the block's last lane .end.
 *   bsc_bigbed_heads_kernel    over the COMPACT starts, one wave per 64 ranks: a site is a window's head iff it is the first or its
 *                              window start / reduction differs from the site's before it -> hcnt[tile]
 *   (exclusive scan; the entry behind the last tile = n_windows)
 *   bsc_bigbed_windows_kernel  a head's lane stores its rank at wbeg[its window's index]; wbeg[n_windows] = n_sites
 *   bsc_bigbed_zoom_kernel     one lane per window: {first start, last start + 1, wbeg[k + 1] - wbeg[k]} -> zoom[k]
 *
 * Positions increase with the index, so the compact starts are sorted: a block is a range of ranks, a window too, and a count is a
 * difference of ranks.  A tile's 64 items are at most 64 * BSC_BB_ITEM_MAX = 6400 bytes: the image holds them in one part.  rank / B and
 * start / reduction go through a 64-bit multiply-high with ceil(2^64 / d), as in bigwigdev.hip.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "recstream_dev.h"
#include "methtext_dev.h"

static_assert(sizeof(bsc_vcf_rec) == 128 && sizeof(bsc_vcf_core) == 64, "bsc_vcf_rec is 128 bytes, its core the first 64");
static_assert(sizeof(bsc_bb_sum) == 24, "a summary is 24 bytes");

#define BB_WAVES 4u
#define BB_IMG (RS_LANES * BSC_BB_ITEM_MAX) /* a tile of the longest items */
static_assert(BB_IMG % 16u == 0u && BSC_BB_ITEM_MAX <= 255u, "the image is whole 16-byte pieces; an item's length is kept in 8 bits");

struct bb_args {
  const uint8_t *core, *aux; /* 64 bytes per position each */
  const uint8_t *emit;       /* the chain's byte per position, or NULL */
  uint64_t n;                /* positions */
  int32_t all_contexts;
  uint32_t min_cov, min_phred;
  int32_t pass_only;
  uint32_t x0, chrom_id;
  uint32_t B, red;
  uint64_t B_magic, red_magic; /* ceil(2^64 / d), d >= 2 */
};

/* v / d, v < 2^32 */
__device__ __forceinline__ uint32_t bb_div(uint32_t v, uint32_t d, uint64_t magic) {
  return d == 1u ? v : (uint32_t)__umul64hi((uint64_t)v, magic);
}

/* entry i < n: is it a site, and of what (the per-cytosine rule, restated from the header); its position is x0 + i */
__device__ __forceinline__ bool bb_site_of(mb_site &s, const bb_args &g, uint64_t i) {
  if (g.emit && !g.emit[i]) return false;
  const uint4 *lo = reinterpret_cast<const uint4 *>(g.core + i * 64u);
  const uint4 v0 = lo[0];
  const unsigned emit = v0.y & 0xffu, gt = (v0.y >> 8) & 0xffu, flt = v0.z & 0xffu, phred = (v0.z >> 8) & 0xffu, cg = v0.z >> 24;
  if (!emit || (gt != 4u && gt != 7u)) return false;
  if (cg != 'C' && !(g.all_contexts && cg == 'H')) return false;
  if (phred < g.min_phred || (g.pass_only && flt)) return false;
  const uint4 c1 = reinterpret_cast<const uint4 *>(g.aux + i * 64u)[1]; /* counts[4 .. 7] */
  s.minus = gt == 7u;
  s.a = s.minus ? c1.z : c1.y; /* counts[6] : counts[5] */
  s.b = s.minus ? c1.x : c1.w; /* counts[4] : counts[7] */
  if ((uint64_t)s.a + s.b < (uint64_t)(g.min_cov > 1u ? g.min_cov : 1u)) return false;
  s.pos = g.x0 + (uint32_t)i;
  s.flt = flt;
  s.phred = phred;
  s.label = 0u;
  if (cg != 'C') {
    const uint4 v1 = lo[1]; /* bytes 16 .. 31: cx_gt[0] = byte 19, cx_gt[4] = byte 23 */
    const unsigned n2 = s.minus ? v1.x >> 24 : v1.y >> 24;
    if (n2 == (s.minus ? 'C' : 'G')) s.label = 1u;
    else s.label = (n2 == 'A' || n2 == 'C' || n2 == 'G' || n2 == 'T') ? 2u : 3u;
  }
  return true;
}

/* the item: chromId, chromStart, chromEnd, then the line from its name on, NUL in the newline's place */
template <class S>
__device__ __forceinline__ void bb_emit_item(S &s, const mb_site &m, uint32_t chrom_id) {
  const uint64_t cov = (uint64_t)m.a + m.b;
  const uint32_t start = m.pos - 1u;
  s.bytes((uint64_t)chrom_id | (uint64_t)start << 32, 8u);
  s.bytes(m.pos, 4u);
  mb_emit_cols<0u>(s, m, start, cov, mb_pct(m.a, cov));
}

__device__ __forceinline__ unsigned bb_lanes_below(unsigned long long mask, unsigned lane) {
  return (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

/* item_len: [n]; cnt, tbytes: [n_tiles + 1] */
extern "C" __global__ __launch_bounds__(256) void bsc_bigbed_size_kernel(bb_args g, uint32_t n_tiles, uint8_t *__restrict__ item_len,
                                                                         unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ tbytes) {
  const unsigned lane = threadIdx.x & 63u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cnt[n_tiles] = 0ull;
    tbytes[n_tiles] = 0ull;
  }
  for (uint32_t tile = blockIdx.x * BB_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * BB_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    mb_site m;
    if (i < g.n && bb_site_of(m, g, i)) {
      mb_count_sink c = {0u};
      bb_emit_item(c, m, g.chrom_id);
      len = c.len; /* BSC_BB_ITEM_MIN .. BSC_BB_ITEM_MAX */
    }
    if (i < g.n) item_len[i] = (uint8_t)len;
    const unsigned long long mask = __ballot(len != 0u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0u) {
      cnt[tile] = (unsigned long long)__popcll(mask);
      tbytes[tile] = len;
    }
  }
}

/* off, boff: the scans of cnt and tbytes; sites: [n] starts; totals[0 .. 2] = {n_bytes, n_sites, n_blocks} */
extern "C" __global__ __launch_bounds__(256) void bsc_bigbed_write_kernel(bb_args g, uint32_t n_tiles, const uint8_t *__restrict__ item_len,
                                                                          const unsigned long long *__restrict__ off,
                                                                          const unsigned long long *__restrict__ boff, uint8_t *__restrict__ out,
                                                                          uint64_t out_cap, bsc_bb_sum *__restrict__ blocks, uint64_t blk_cap,
                                                                          uint32_t *__restrict__ sites, unsigned long long *__restrict__ totals) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[BB_WAVES][BB_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n_sites = off[n_tiles], n_bytes = boff[n_tiles]; /* n_sites <= n < 2^32 */
  const uint64_t n_blk = n_sites ? (uint64_t)bb_div((uint32_t)(n_sites - 1u), g.B, g.B_magic) + 1u : 0u;
  const bool fits = n_bytes <= out_cap, blk_ok = n_blk <= blk_cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[0] = n_bytes;
    totals[1] = n_sites;
    totals[2] = n_blk;
  }
  for (uint32_t tile = blockIdx.x * BB_WAVES + wid; tile < n_tiles; tile += gridDim.x * BB_WAVES) {
    const uint64_t g_tile = boff[tile], g_end = boff[tile + 1u];
    if (g_end == g_tile) continue; /* no site in this tile: nothing of it is read (wave-uniform) */
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const unsigned len = i < g.n ? item_len[i] : 0u;
    const unsigned long long mask = __ballot(len != 0u);
    unsigned excl, t_all;
    (void)rs_wave_excl_scan(len, excl, t_all); /* t_all = g_end - g_tile <= BB_IMG */
    mb_site m;
    /* the size pass said so.  The rule is evaluated again from the same bytes — nothing writes core / aux / emit between the two passes of
     * one call — and a lane whose verdict differed would write nothing into its len bytes of the image: wrong bytes, never a byte outside */
    const bool site = len != 0u && bb_site_of(m, g, i);
    const unsigned ph = (unsigned)(g_tile & 15u);
    if (site) {
      const uint32_t rank = (uint32_t)(off[tile] + bb_lanes_below(mask, lane)); /* < n_sites */
      const uint32_t start = m.pos - 1u;
      sites[rank] = start;
      if (fits) {
        mb_write_sink w = {img + ph + excl, 0u}; /* excl + len <= t_all <= BB_IMG */
        bb_emit_item(w, m, g.chrom_id);
      }
      if (blk_ok) {
        const uint32_t k = bb_div(rank, g.B, g.B_magic), in = rank - k * g.B; /* k < n_blk <= blk_cap */
        uint32_t *const h = reinterpret_cast<uint32_t *>(blocks + k);
        if (in == 0u) {
          const uint64_t left = n_sites - (uint64_t)k * g.B;
          h[0] = start;
          h[2] = left < g.B ? (uint32_t)left : g.B;
          h[3] = 0u;
          *reinterpret_cast<unsigned long long *>(h + 4) = g_tile + excl;
        }
        if (in == g.B - 1u || (uint64_t)rank == n_sites - 1u) h[1] = start + 1u;
      }
    }
    if (!fits) continue; /* wave-uniform */
    rs_wave_sync();
    rs_copy_out(img, out + (g_tile - ph), lane, rs_copy_ranges(ph, t_all)); /* the image [ph, ph + t) -> out[g_tile, g_end), g_end <= n_bytes <= out_cap */
    rs_wave_sync();
  }
}

/* the window of a start */
__device__ __forceinline__ uint32_t bb_window(const bb_args &g, uint32_t start) { return bb_div(start, g.red, g.red_magic); }

/* hcnt: [n_tiles + 1]: window heads per 64 compact sites (n_sites <= n: n_tiles tiles cover them) */
extern "C" __global__ __launch_bounds__(256) void bsc_bigbed_heads_kernel(bb_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                                          const uint32_t *__restrict__ sites, unsigned long long *__restrict__ hcnt) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles];
  if (blockIdx.x == 0 && threadIdx.x == 0) hcnt[n_tiles] = 0ull;
  for (uint32_t tile = blockIdx.x * BB_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * BB_WAVES) {
    const uint64_t r = (uint64_t)tile * 64u + lane;
    bool head = false;
    if (r < n_sites) head = r == 0u || bb_window(g, sites[r]) != bb_window(g, sites[r - 1u]);
    const unsigned long long mask = __ballot(head);
    if (lane == 0u) hcnt[tile] = (unsigned long long)__popcll(mask);
  }
}

/* wbeg: [n + 1]: the rank of every window's first site, and n_sites behind the last; totals[3] = n_windows */
extern "C" __global__ __launch_bounds__(256) void bsc_bigbed_windows_kernel(bb_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                                            const unsigned long long *__restrict__ hoff,
                                                                            const uint32_t *__restrict__ sites, uint32_t *__restrict__ wbeg,
                                                                            unsigned long long *__restrict__ totals) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles], n_win = hoff[n_tiles]; /* n_win <= n_sites <= n */
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[3] = n_win;
    wbeg[n_win] = (uint32_t)n_sites;
  }
  for (uint32_t tile = blockIdx.x * BB_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * BB_WAVES) {
    const uint64_t r = (uint64_t)tile * 64u + lane;
    bool head = false;
    if (r < n_sites) head = r == 0u || bb_window(g, sites[r]) != bb_window(g, sites[r - 1u]);
    const unsigned long long mask = __ballot(head);
    if (head) wbeg[hoff[tile] + bb_lanes_below(mask, lane)] = (uint32_t)r; /* < n_win */
  }
}

/* one lane per window */
extern "C" __global__ __launch_bounds__(256) void bsc_bigbed_zoom_kernel(uint32_t n_tiles, const unsigned long long *__restrict__ hoff,
                                                                         const uint32_t *__restrict__ sites, const uint32_t *__restrict__ wbeg,
                                                                         bsc_bb_sum *__restrict__ zoom, uint64_t zoom_cap) {
  const uint64_t n_win = hoff[n_tiles];
  if (n_win > zoom_cap) return;
  for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < n_win; k += (uint64_t)gridDim.x * 256u) {
    const uint32_t lo = wbeg[k], hi = wbeg[k + 1u]; /* hi > lo: a window holds a site */
    bsc_bb_sum s;
    s.start = sites[lo];
    s.end = sites[hi - 1u] + 1u;
    s.count = hi - lo;
    s._pad = 0u;
    s.off = 0ull;
    zoom[k] = s;
  }
}

extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

static uint64_t bb_magic(uint32_t d) { return d < 2u ? 0ull : 0xffffffffffffffffull / d + 1ull; } /* ceil(2^64 / d) */

/*
 * core[n] / aux[n]: the per-position arrays, entry i = position x0 + i; emit: the chain's byte per position or NULL.  item_len: n bytes;
 * cnt / off / tbytes / boff / hcnt / hoff: n / 64 rounded up + 1 u64 each; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of that; sites: n u32;
 * wbeg: n + 1 u32.  out: 16-byte aligned.  totals: four u64.  n >= 1.
 */
extern "C" int bsc_dev_launch_bigbed(const void *core, const void *aux, const void *emit, uint64_t n, uint32_t x0, uint32_t chrom_id,
                                     const bsc_meth_params *par, const bsc_bb_params *bbp, void *item_len, void *cnt, void *off, void *tbytes, void *boff,
                                     void *hcnt, void *hoff, void *scan_tmp, size_t scan_tmp_bytes, void *sites, void *wbeg, void *out, uint64_t out_cap,
                                     void *blocks, uint64_t blk_cap, void *zoom, uint64_t zoom_cap, void *totals, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!par || !bbp || !n || n > 0xffffffffull || !item_len || !cnt || !off || !tbytes || !boff || !hcnt || !hoff || !sites || !wbeg || !totals)
    return (int)hipErrorInvalidValue;
  if (bbp->items_per_block < 1u || bbp->items_per_block > 65535u || bbp->reduction < 1u) return (int)hipErrorInvalidValue;
  if ((out_cap && !out) || (blk_cap && !blocks) || (zoom_cap && !zoom) || ((uintptr_t)out & 15u) || (((uintptr_t)blocks | (uintptr_t)zoom) & 7u))
    return (int)hipErrorInvalidValue;
  bb_args g;
  g.core = (const uint8_t *)core;
  g.aux = (const uint8_t *)aux;
  g.emit = (const uint8_t *)emit;
  g.n = n;
  g.all_contexts = par->contexts == BSC_METH_ALL;
  g.min_cov = par->min_cov;
  g.min_phred = par->min_phred;
  g.pass_only = par->pass_only != 0;
  g.x0 = x0;
  g.chrom_id = chrom_id;
  g.B = bbp->items_per_block;
  g.red = bbp->reduction;
  g.B_magic = bb_magic(g.B);
  g.red_magic = bb_magic(g.red);
  const uint32_t n_tiles = (uint32_t)((n + 63u) / 64u);
  const unsigned cap = (unsigned)(num_cus > 0 ? num_cus : 1) * 8u;
  unsigned grid = (n_tiles + BB_WAVES - 1u) / BB_WAVES;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(bsc_bigbed_size_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (uint8_t *)item_len, (unsigned long long *)cnt,
                     (unsigned long long *)tbytes);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  int rc = bsc_dev_scan_u64(cnt, off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  if ((rc = bsc_dev_scan_u64(tbytes, boff, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream))) return rc;
  hipLaunchKernelGGL(bsc_bigbed_write_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (const uint8_t *)item_len, (const unsigned long long *)off,
                     (const unsigned long long *)boff, (uint8_t *)out, out_cap, (bsc_bb_sum *)blocks, blk_cap, (uint32_t *)sites,
                     (unsigned long long *)totals);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bsc_bigbed_heads_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off, (const uint32_t *)sites,
                     (unsigned long long *)hcnt);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((rc = bsc_dev_scan_u64(hcnt, hoff, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream))) return rc;
  hipLaunchKernelGGL(bsc_bigbed_windows_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off,
                     (const unsigned long long *)hoff, (const uint32_t *)sites, (uint32_t *)wbeg, (unsigned long long *)totals);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  unsigned zgrid = (unsigned)((n + 255u) / 256u);
  if (zgrid > cap) zgrid = cap;
  hipLaunchKernelGGL(bsc_bigbed_zoom_kernel, dim3(zgrid), dim3(256), 0, s, n_tiles, (const unsigned long long *)hoff, (const uint32_t *)sites,
                     (const uint32_t *)wbeg, (bsc_bb_sum *)zoom, zoom_cap);
  return (int)hipGetLastError();
}
