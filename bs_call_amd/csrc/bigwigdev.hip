/*
 * bigwigdev.hip — the methylation bigWig track on the device: from the dense per-position arrays a block call left in HBM, the block's
 * data stream (sections of {start, value} items), the summary of every section and the summary of every level-0 zoom window
 * (include/bscall_amd.h has the rule; the host form csrc/bigwig.c is the checker).  A compaction, two segmented reductions and no
 * floating-point instruction: the value written is entry m of a table of 1001 floats the host made, copied as 32 bits.
 *
 *   bsc_bigwig_tile_kernel     one wave per tile of 64 positions: the site predicate per lane -> cnt[tile] (u64; cnt[n_tiles] = 0)
 *   (exclusive scan, rocPRIM u64: sort.hip; the entry behind the last tile = n_sites)
 *   bsc_bigwig_write_kernel    one wave per tile: rank = scan[tile] + the sites in lower lanes.  The site's lane stores {start, m} at
 *                              sites[rank] (a workspace: what the reductions read) and, where the stream fits out_cap, its 8-byte item at
 *                              (rank / S)(24 + 8 S) + 24 + 8 (rank % S); a section's first lane stores its header, its last lane chromEnd
 *   bsc_bigwig_heads_kernel    over the COMPACT sites, one wave per 64 ranks: a site is a window's head iff it is the first or its
 *                              window start / reduction differs from the site's before it -> hcnt[tile]
 *   (exclusive scan; the entry behind the last tile = n_windows)
 *   bsc_bigwig_windows_kernel  a head's lane stores its rank at wbeg[its window's index]; wbeg[n_windows] = n_sites
 *   bsc_bigwig_reduce_kernel   one wave per section and one per window: its sites' count, min, max, sum of m and of m * m by a strided
 *                              loop and a butterfly of integer adds / min / max -> sections[k] / zoom[k].  A wave owns its destination:
 *                              the only atomics are two 64-bit integer adds per section into the block's totals {sum m, sum m * m},
 *                              which no order can change.
 *
 * Positions increase with the index, so the compact sites are sorted by start: a section is a range of ranks, a window too.
 * The divisions, m and the site predicate are csrc/bigwig_dev.h.
 */
#include "bigwig_dev.h" /* bw_args, bw_div, bw_m, bw_site_of, bw_lanes_below, bw_window: shared with bwcovdev.hip */

/* cnt: [n_tiles + 1] */
extern "C" __global__ __launch_bounds__(256) void bsc_bigwig_tile_kernel(bw_args g, uint32_t n_tiles, unsigned long long *__restrict__ cnt) {
  const unsigned lane = threadIdx.x & 63u;
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[n_tiles] = 0ull;
  for (uint32_t tile = blockIdx.x * BW_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * BW_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    uint32_t a = 0u, b = 0u;
    const bool site = i < g.n && bw_site_of(g, i, a, b);
    const unsigned long long mask = __ballot(site);
    if (lane == 0u) cnt[tile] = (unsigned long long)__popcll(mask);
  }
}

/* off: the scan of cnt; val: the 1001 floats as their 32 bits; sites: [n] {start, m}; totals[0 .. 2] = {n_bytes, n_sites, n_sections} */
extern "C" __global__ __launch_bounds__(256) void bsc_bigwig_write_kernel(bw_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                                          const uint32_t *__restrict__ val, uint8_t *__restrict__ out,
                                                                          uint64_t out_cap, uint2 *__restrict__ sites,
                                                                          unsigned long long *__restrict__ totals) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles]; /* <= n < 2^32 */
  const uint64_t n_sec = n_sites ? (uint64_t)bw_div((uint32_t)(n_sites - 1u), g.S, g.S_magic) + 1u : 0u;
  const uint64_t n_bytes = 24u * n_sec + 8u * n_sites, sec_bytes = 24u + 8u * (uint64_t)g.S;
  const bool fits = n_bytes <= out_cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[0] = n_bytes;
    totals[1] = n_sites;
    totals[2] = n_sec;
  }
  for (uint32_t tile = blockIdx.x * BW_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * BW_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    uint32_t a = 0u, b = 0u;
    const bool site = i < g.n && bw_site_of(g, i, a, b);
    const unsigned long long mask = __ballot(site);
    if (!site) continue;
    const uint32_t rank = (uint32_t)(off[tile] + bw_lanes_below(mask, lane)); /* < n_sites */
    const uint32_t start = g.x0 + (uint32_t)i - 1u, m = bw_m(a, (uint64_t)a + b);
    sites[rank] = make_uint2(start, m);
    if (!fits) continue;
    const uint32_t k = bw_div(rank, g.S, g.S_magic), in = rank - k * g.S;
    uint8_t *const sec = out + (uint64_t)k * sec_bytes; /* k < n_sec: sec + 24 + 8 in + 8 <= n_bytes <= out_cap */
    *reinterpret_cast<uint2 *>(sec + 24u + 8u * (uint64_t)in) = make_uint2(start, val[m]);
    if (in == 0u) {
      const uint64_t left = n_sites - (uint64_t)k * g.S;
      const uint32_t count = left < g.S ? (uint32_t)left : g.S;
      uint32_t *const h = reinterpret_cast<uint32_t *>(sec);
      h[0] = g.chrom_id;
      h[1] = start;
      h[3] = 0u;
      h[4] = 1u;
      h[5] = 2u | (count << 16); /* type = 2 (varStep), reserved = 0, itemCount */
    }
    if (in == g.S - 1u || (uint64_t)rank == n_sites - 1u) reinterpret_cast<uint32_t *>(sec)[2] = start + 1u;
  }
}

/* hcnt: [n_tiles + 1]: window heads per 64 compact sites (n_sites <= n: n_tiles tiles cover them) */
extern "C" __global__ __launch_bounds__(256) void bsc_bigwig_heads_kernel(bw_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                                          const uint2 *__restrict__ sites, unsigned long long *__restrict__ hcnt) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles];
  if (blockIdx.x == 0 && threadIdx.x == 0) hcnt[n_tiles] = 0ull;
  for (uint32_t tile = blockIdx.x * BW_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * BW_WAVES) {
    const uint64_t r = (uint64_t)tile * 64u + lane;
    bool head = false;
    if (r < n_sites) head = r == 0u || bw_window(g, sites[r].x) != bw_window(g, sites[r - 1u].x);
    const unsigned long long mask = __ballot(head);
    if (lane == 0u) hcnt[tile] = (unsigned long long)__popcll(mask);
  }
}

/* wbeg: [n + 1]: the rank of every window's first site, and n_sites behind the last; totals[3] = n_windows */
extern "C" __global__ __launch_bounds__(256) void bsc_bigwig_windows_kernel(bw_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                                            const unsigned long long *__restrict__ hoff,
                                                                            const uint2 *__restrict__ sites, uint32_t *__restrict__ wbeg,
                                                                            unsigned long long *__restrict__ totals) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles], n_win = hoff[n_tiles]; /* n_win <= n_sites <= n */
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[3] = n_win;
    wbeg[n_win] = (uint32_t)n_sites;
  }
  for (uint32_t tile = blockIdx.x * BW_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * BW_WAVES) {
    const uint64_t r = (uint64_t)tile * 64u + lane;
    bool head = false;
    if (r < n_sites) head = r == 0u || bw_window(g, sites[r].x) != bw_window(g, sites[r - 1u].x);
    const unsigned long long mask = __ballot(head);
    if (head) wbeg[hoff[tile] + bw_lanes_below(mask, lane)] = (uint32_t)r; /* < n_win */
  }
}

/* one wave per section, then one per window: the summary of sites[lo .. hi) */
extern "C" __global__ __launch_bounds__(256) void bsc_bigwig_reduce_kernel(bw_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                                           const unsigned long long *__restrict__ hoff,
                                                                           const uint2 *__restrict__ sites, const uint32_t *__restrict__ wbeg,
                                                                           bsc_bw_sum *__restrict__ sections, uint64_t sec_cap,
                                                                           bsc_bw_sum *__restrict__ zoom, uint64_t zoom_cap,
                                                                           unsigned long long *totals) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles], n_win = hoff[n_tiles];
  const uint64_t n_sec = n_sites ? (uint64_t)bw_div((uint32_t)(n_sites - 1u), g.S, g.S_magic) + 1u : 0u;
  const bool sec_ok = n_sec <= sec_cap, zoom_ok = n_win <= zoom_cap;
  for (uint64_t u = (uint64_t)blockIdx.x * BW_WAVES + (threadIdx.x >> 6); u < n_sec + n_win; u += (uint64_t)gridDim.x * BW_WAVES) {
    const bool is_sec = u < n_sec; /* wave-uniform */
    uint64_t lo, hi;
    bsc_bw_sum *dst;
    if (is_sec) {
      lo = u * g.S;
      hi = lo + g.S < n_sites ? lo + g.S : n_sites;
      dst = sec_ok ? sections + u : nullptr;
    } else {
      const uint64_t k = u - n_sec;
      lo = wbeg[k];
      hi = wbeg[k + 1u];
      dst = zoom_ok ? zoom + k : nullptr;
    }
    uint32_t cnt = 0u, mn = 0xffffffffu, mx = 0u;
    unsigned long long sum = 0ull, sum2 = 0ull;
    for (uint64_t r = lo + lane; r < hi; r += 64u) {
      const uint32_t m = sites[r].y;
      cnt++;
      mn = m < mn ? m : mn;
      mx = m > mx ? m : mx;
      sum += m;
      sum2 += (unsigned long long)m * m;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      cnt += __shfl_xor(cnt, d);
      const uint32_t omn = __shfl_xor(mn, d), omx = __shfl_xor(mx, d);
      mn = omn < mn ? omn : mn;
      mx = omx > mx ? omx : mx;
      sum += __shfl_xor(sum, d);
      sum2 += __shfl_xor(sum2, d);
    }
    if (lane == 0u) {
      if (dst) {
        bsc_bw_sum s;
        s.start = sites[lo].x;
        s.end = sites[hi - 1u].x + 1u; /* (hi > lo: a section and a window hold a site) */
        s.count = cnt;
        s.min_m = mn;
        s.max_m = mx;
        s._pad = 0u;
        s.sum_m = sum;
        s.sum_m2 = sum2;
        *dst = s;
      }
      if (is_sec) {
        atomicAdd(&totals[4], sum);
        atomicAdd(&totals[5], sum2);
      }
    }
  }
}

extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

/* the three kernels the coverage launch (bwcovdev.hip) reuses as they are, launched from this file (a kernel is launched where it is compiled) */
extern "C" int bsc_dev_bigwig_tile(const bw_args *g, uint32_t n_tiles, void *cnt, unsigned grid, void *stream) {
  hipLaunchKernelGGL(bsc_bigwig_tile_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *g, n_tiles, (unsigned long long *)cnt);
  return (int)hipGetLastError();
}
extern "C" int bsc_dev_bigwig_heads(const bw_args *g, uint32_t n_tiles, const void *off, const void *sites, void *hcnt, unsigned grid, void *stream) {
  hipLaunchKernelGGL(bsc_bigwig_heads_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *g, n_tiles, (const unsigned long long *)off,
                     (const uint2 *)sites, (unsigned long long *)hcnt);
  return (int)hipGetLastError();
}
extern "C" int bsc_dev_bigwig_windows(const bw_args *g, uint32_t n_tiles, const void *off, const void *hoff, const void *sites, void *wbeg, void *totals,
                                      unsigned grid, void *stream) {
  hipLaunchKernelGGL(bsc_bigwig_windows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *g, n_tiles, (const unsigned long long *)off,
                     (const unsigned long long *)hoff, (const uint2 *)sites, (uint32_t *)wbeg, (unsigned long long *)totals);
  return (int)hipGetLastError();
}

/*
 * core[n] / aux[n]: the per-position arrays, entry i = position x0 + i; emit: the chain's byte per position or NULL.  cnt / off / hcnt /
 * hoff: n / 64 rounded up + 1 u64 each; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of that; sites: n x 8 bytes; wbeg: n + 1 u32; val: the 1001
 * floats.  totals: six u64, [4] and [5] zeroed here.  n >= 1.
 */
extern "C" int bsc_dev_launch_bigwig(const void *core, const void *aux, const void *emit, uint64_t n, uint32_t x0, uint32_t chrom_id,
                                     const bsc_meth_params *par, const bsc_bw_params *bwp, const void *val, void *cnt, void *off, void *hcnt, void *hoff,
                                     void *scan_tmp, size_t scan_tmp_bytes, void *sites, void *wbeg, void *out, uint64_t out_cap, void *sections,
                                     uint64_t sec_cap, void *zoom, uint64_t zoom_cap, void *totals, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!par || !bwp || !n || n > 0xffffffffull || !val || !cnt || !off || !hcnt || !hoff || !sites || !wbeg || !totals) return (int)hipErrorInvalidValue;
  if (bwp->items_per_section < 1u || bwp->items_per_section > 65535u || bwp->reduction < 1u) return (int)hipErrorInvalidValue;
  if ((out_cap && !out) || (sec_cap && !sections) || (zoom_cap && !zoom) || ((uintptr_t)out & 7u)) return (int)hipErrorInvalidValue;
  bw_args g;
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
  g.S = bwp->items_per_section;
  g.red = bwp->reduction;
  g.S_magic = bw_magic(g.S);
  g.red_magic = bw_magic(g.red);
  const uint32_t n_tiles = (uint32_t)((n + 63u) / 64u);
  const unsigned cap = (unsigned)(num_cus > 0 ? num_cus : 1) * 8u;
  unsigned grid = (n_tiles + BW_WAVES - 1u) / BW_WAVES;
  if (grid > cap) grid = cap;
  hipError_t e = hipMemsetAsync((char *)totals + 32, 0, 16, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bsc_bigwig_tile_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (unsigned long long *)cnt);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  int rc = bsc_dev_scan_u64(cnt, off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_bigwig_write_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off, (const uint32_t *)val,
                     (uint8_t *)out, out_cap, (uint2 *)sites, (unsigned long long *)totals);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bsc_bigwig_heads_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off, (const uint2 *)sites,
                     (unsigned long long *)hcnt);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  rc = bsc_dev_scan_u64(hcnt, hoff, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_bigwig_windows_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off,
                     (const unsigned long long *)hoff, (const uint2 *)sites, (uint32_t *)wbeg, (unsigned long long *)totals);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  const uint64_t units = 2u * n; /* at most: every site a section and a window of its own */
  unsigned rgrid = (unsigned)((units + BW_WAVES - 1u) / BW_WAVES < cap ? (units + BW_WAVES - 1u) / BW_WAVES : cap);
  hipLaunchKernelGGL(bsc_bigwig_reduce_kernel, dim3(rgrid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off,
                     (const unsigned long long *)hoff, (const uint2 *)sites, (const uint32_t *)wbeg, (bsc_bw_sum *)sections, sec_cap,
                     (bsc_bw_sum *)zoom, zoom_cap, (unsigned long long *)totals);
  return (int)hipGetLastError();
}
