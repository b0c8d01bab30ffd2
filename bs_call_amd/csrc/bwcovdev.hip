/*
 * bwcovdev.hip — the coverage bigWig track on the device, alone or beside the level track in ONE sweep over the per-position arrays
 * (include/bscall_amd.h has the rule; the host form bsc_bigwig_cov_sections_recs of csrc/bigwig.c is the checker).  Both tracks have the same
 * sites, so the tile pass, the two scans, the heads and the windows passes of csrc/bigwigdev.hip are reused as they are and run once; the two
 * kernels here are templates over the track mask (bit 0 level, bit 1 coverage):
 *
 *   bsc_bwcov_write_kernel<mask>   one wave per tile of 64 positions: rank = scan[tile] + the sites in lower lanes.  The site's lane stores
 *                                  {start, m} at sites[rank] and c = min(a + b, 2^32 - 1) at cov[rank] (workspaces: what the passes behind it
 *                                  read), and its 8-byte item into each requested stream that fits its room; a section's first lane stores
 *                                  the header, its last lane chromEnd, per stream.  m's bisection runs with bit 0 alone.  The coverage float
 *                                  is the hardware's u32 -> f32 conversion (round to nearest even, the default mode): the one
 *                                  floating-point instruction of the file.
 *   bsc_bwcov_reduce_kernel<mask>  one wave per section and one per window over the compact sites, both tracks in one sweep: count, min,
 *                                  max, the sum of m and of m * m as in bigwigdev.hip; for the coverage the sum of c in 64 bits and the
 *                                  sum of c * c in 96 bits — a (lo, hi) pair per lane, the butterfly adds with carry.  A wave owns its
 *                                  destination; the only atomics are the level track's two 64-bit adds into totals[4], totals[5].
 */
#include "bigwig_dev.h"

/* off: the scan of cnt; val: the 1001 floats as their 32 bits; sites: [n] {start, m}; cov: [n] c; totals[0 .. 2] = {n_bytes, n_sites, n_sections} */
template <unsigned MASK>
__global__ __launch_bounds__(256) void bsc_bwcov_write_kernel(bw_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                              const uint32_t *__restrict__ val, uint8_t *__restrict__ lout, uint64_t lcap,
                                                              uint8_t *__restrict__ cout, uint64_t ccap, uint2 *__restrict__ sites,
                                                              uint32_t *__restrict__ cov, unsigned long long *__restrict__ totals) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles]; /* <= n < 2^32 */
  const uint64_t n_sec = n_sites ? (uint64_t)bw_div((uint32_t)(n_sites - 1u), g.S, g.S_magic) + 1u : 0u;
  const uint64_t n_bytes = 24u * n_sec + 8u * n_sites, sec_bytes = 24u + 8u * (uint64_t)g.S;
  const bool lfits = (MASK & 1u) && n_bytes <= lcap, cfits = (MASK & 2u) && n_bytes <= ccap;
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
    const uint32_t start = g.x0 + (uint32_t)i - 1u;
    const uint64_t ab = (uint64_t)a + b;
    const uint32_t m = (MASK & 1u) ? bw_m(a, ab) : 0u;
    const uint32_t c = ab > 0xffffffffull ? 0xffffffffu : (uint32_t)ab;
    sites[rank] = make_uint2(start, m);
    if (MASK & 2u) cov[rank] = c;
    if (!lfits && !cfits) continue;
    const uint32_t k = bw_div(rank, g.S, g.S_magic), in = rank - k * g.S;
    const uint64_t sec_at = (uint64_t)k * sec_bytes; /* k < n_sec: sec_at + 24 + 8 in + 8 <= n_bytes <= the stream's room */
    const uint64_t left = n_sites - (uint64_t)k * g.S;
    const uint32_t count = left < g.S ? (uint32_t)left : g.S;
    const bool last = in == g.S - 1u || (uint64_t)rank == n_sites - 1u;
#pragma unroll
    for (unsigned t = 0; t < 2u; t++) {
      if (!(t ? cfits : lfits)) continue;
      uint8_t *const sec = (t ? cout : lout) + sec_at;
      const uint32_t bits = t ? __float_as_uint(__uint2float_rn(c)) : val[m];
      *reinterpret_cast<uint2 *>(sec + 24u + 8u * (uint64_t)in) = make_uint2(start, bits);
      uint32_t *const h = reinterpret_cast<uint32_t *>(sec);
      if (in == 0u) {
        h[0] = g.chrom_id;
        h[1] = start;
        h[3] = 0u;
        h[4] = 1u;
        h[5] = 2u | (count << 16); /* type = 2 (varStep), reserved = 0, itemCount */
      }
      if (last) h[2] = start + 1u;
    }
  }
}

/* one wave per section, then one per window: the summaries of sites[lo .. hi) / cov[lo .. hi) */
template <unsigned MASK>
__global__ __launch_bounds__(256) void bsc_bwcov_reduce_kernel(bw_args g, uint32_t n_tiles, const unsigned long long *__restrict__ off,
                                                               const unsigned long long *__restrict__ hoff, const uint2 *__restrict__ sites,
                                                               const uint32_t *__restrict__ cov, const uint32_t *__restrict__ wbeg,
                                                               bsc_bw_sum *__restrict__ lsec, uint64_t lsec_cap, bsc_bw_sum *__restrict__ lzoom,
                                                               uint64_t lzoom_cap, bsc_bw_sum *__restrict__ csec, uint64_t csec_cap,
                                                               bsc_bw_sum *__restrict__ czoom, uint64_t czoom_cap, unsigned long long *totals) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n_sites = off[n_tiles], n_win = hoff[n_tiles];
  const uint64_t n_sec = n_sites ? (uint64_t)bw_div((uint32_t)(n_sites - 1u), g.S, g.S_magic) + 1u : 0u;
  for (uint64_t u = (uint64_t)blockIdx.x * BW_WAVES + (threadIdx.x >> 6); u < n_sec + n_win; u += (uint64_t)gridDim.x * BW_WAVES) {
    const bool is_sec = u < n_sec; /* wave-uniform */
    uint64_t lo, hi;
    bsc_bw_sum *ldst = nullptr, *cdst = nullptr;
    if (is_sec) {
      lo = u * g.S;
      hi = lo + g.S < n_sites ? lo + g.S : n_sites;
      if ((MASK & 1u) && n_sec <= lsec_cap) ldst = lsec + u;
      if ((MASK & 2u) && n_sec <= csec_cap) cdst = csec + u;
    } else {
      const uint64_t k = u - n_sec;
      lo = wbeg[k];
      hi = wbeg[k + 1u];
      if ((MASK & 1u) && n_win <= lzoom_cap) ldst = lzoom + k;
      if ((MASK & 2u) && n_win <= czoom_cap) cdst = czoom + k;
    }
    uint32_t cnt = 0u, mn = 0xffffffffu, mx = 0u, cmn = 0xffffffffu, cmx = 0u, c2hi = 0u;
    unsigned long long sum = 0ull, sum2 = 0ull, csum = 0ull, c2lo = 0ull;
    for (uint64_t r = lo + lane; r < hi; r += 64u) {
      cnt++;
      if (MASK & 1u) {
        const uint32_t m = sites[r].y;
        mn = m < mn ? m : mn;
        mx = m > mx ? m : mx;
        sum += m;
        sum2 += (unsigned long long)m * m;
      }
      if (MASK & 2u) {
        const uint32_t c = cov[r];
        const unsigned long long sq = (unsigned long long)c * c; /* < 2^64 */
        cmn = c < cmn ? c : cmn;
        cmx = c > cmx ? c : cmx;
        csum += c; /* a wave's sites are < 2^32: < 2^64 */
        c2lo += sq;
        c2hi += c2lo < sq ? 1u : 0u;
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      cnt += __shfl_xor(cnt, d);
      if (MASK & 1u) {
        const uint32_t omn = __shfl_xor(mn, d), omx = __shfl_xor(mx, d);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        sum += __shfl_xor(sum, d);
        sum2 += __shfl_xor(sum2, d);
      }
      if (MASK & 2u) {
        const uint32_t omn = __shfl_xor(cmn, d), omx = __shfl_xor(cmx, d), ohi = __shfl_xor(c2hi, d);
        const unsigned long long olo = __shfl_xor(c2lo, d);
        cmn = omn < cmn ? omn : cmn;
        cmx = omx > cmx ? omx : cmx;
        csum += __shfl_xor(csum, d);
        c2lo += olo;
        c2hi += ohi + (c2lo < olo ? 1u : 0u);
      }
    }
    if (lane == 0u) {
      bsc_bw_sum s;
      s.start = sites[lo].x;
      s.end = sites[hi - 1u].x + 1u; /* (hi > lo: a section and a window hold a site) */
      s.count = cnt;
      if (ldst) {
        s.min_m = mn;
        s.max_m = mx;
        s._pad = 0u;
        s.sum_m = sum;
        s.sum_m2 = sum2;
        *ldst = s;
      }
      if (cdst) {
        s.min_m = cmn;
        s.max_m = cmx;
        s._pad = c2hi;
        s.sum_m = csum;
        s.sum_m2 = c2lo;
        *cdst = s;
      }
      if ((MASK & 1u) && is_sec) {
        atomicAdd(&totals[4], sum);
        atomicAdd(&totals[5], sum2);
      }
    }
  }
}

extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */
/* bigwigdev.hip: its tile, heads and windows kernels, launched from their own file */
extern "C" int bsc_dev_bigwig_tile(const bw_args *g, uint32_t n_tiles, void *cnt, unsigned grid, void *stream);
extern "C" int bsc_dev_bigwig_heads(const bw_args *g, uint32_t n_tiles, const void *off, const void *sites, void *hcnt, unsigned grid, void *stream);
extern "C" int bsc_dev_bigwig_windows(const bw_args *g, uint32_t n_tiles, const void *off, const void *hoff, const void *sites, void *wbeg, void *totals,
                                      unsigned grid, void *stream);

template <unsigned MASK>
static hipError_t bwcov_write(unsigned grid, hipStream_t s, const bw_args &g, uint32_t n_tiles, const void *off, const void *val,
                              const bsc_bw_track_out &lv, const bsc_bw_track_out &cv, void *sites, void *cov, void *totals) {
  hipLaunchKernelGGL(bsc_bwcov_write_kernel<MASK>, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off, (const uint32_t *)val,
                     (uint8_t *)lv.d_out, lv.out_cap, (uint8_t *)cv.d_out, cv.out_cap, (uint2 *)sites, (uint32_t *)cov, (unsigned long long *)totals);
  return hipGetLastError();
}

template <unsigned MASK>
static hipError_t bwcov_reduce(unsigned grid, hipStream_t s, const bw_args &g, uint32_t n_tiles, const void *off, const void *hoff, const void *sites,
                               const void *cov, const void *wbeg, const bsc_bw_track_out &lv, const bsc_bw_track_out &cv, void *totals) {
  hipLaunchKernelGGL(bsc_bwcov_reduce_kernel<MASK>, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)off,
                     (const unsigned long long *)hoff, (const uint2 *)sites, (const uint32_t *)cov, (const uint32_t *)wbeg, (bsc_bw_sum *)lv.d_sections,
                     lv.sec_cap, (bsc_bw_sum *)lv.d_zoom, lv.zoom_cap, (bsc_bw_sum *)cv.d_sections, cv.sec_cap, (bsc_bw_sum *)cv.d_zoom, cv.zoom_cap,
                     (unsigned long long *)totals);
  return hipGetLastError();
}

static bool bwcov_track_ok(const bsc_bw_track_out *t) {
  return t && !((t->out_cap && !t->d_out) || (t->sec_cap && !t->d_sections) || (t->zoom_cap && !t->d_zoom) || ((uintptr_t)t->d_out & 7u));
}

/*
 * The arguments of bsc_dev_launch_bigwig (bigwigdev.hip) with the track mask, one descriptor per requested track (the other may be NULL) and
 * cov: n x 4 bytes, the compact coverage values (read with bit 1 alone).  tile, scan, write, heads, scan, windows, reduce; the grid caps of
 * bsc_dev_launch_bigwig.  totals: six u64, [4] and [5] zeroed here (and left zero without bit 0).  n >= 1.
 */
extern "C" int bsc_dev_launch_bigwig_tracks(const void *core, const void *aux, const void *emit, uint64_t n, uint32_t x0, uint32_t chrom_id,
                                            const bsc_meth_params *par, const bsc_bw_params *bwp, uint32_t tracks, const void *val, void *cnt, void *off,
                                            void *hcnt, void *hoff, void *scan_tmp, size_t scan_tmp_bytes, void *sites, void *cov, void *wbeg,
                                            const bsc_bw_track_out *level, const bsc_bw_track_out *coverage, void *totals, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!par || !bwp || !n || n > 0xffffffffull || !cnt || !off || !hcnt || !hoff || !sites || !wbeg || !totals) return (int)hipErrorInvalidValue;
  if (tracks < 1u || tracks > 3u || ((tracks & 1u) && (!val || !bwcov_track_ok(level))) || ((tracks & 2u) && (!cov || !bwcov_track_ok(coverage))))
    return (int)hipErrorInvalidValue;
  if (bwp->items_per_section < 1u || bwp->items_per_section > 65535u || bwp->reduction < 1u) return (int)hipErrorInvalidValue;
  const bsc_bw_track_out none = {nullptr, 0, nullptr, 0, nullptr, 0};
  const bsc_bw_track_out lv = (tracks & 1u) ? *level : none, cv = (tracks & 2u) ? *coverage : none;
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
  int rc = bsc_dev_bigwig_tile(&g, n_tiles, cnt, grid, stream);
  if (rc) return rc;
  if ((rc = bsc_dev_scan_u64(cnt, off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream))) return rc;
  e = tracks == 1u   ? bwcov_write<1u>(grid, s, g, n_tiles, off, val, lv, cv, sites, cov, totals)
      : tracks == 2u ? bwcov_write<2u>(grid, s, g, n_tiles, off, val, lv, cv, sites, cov, totals)
                     : bwcov_write<3u>(grid, s, g, n_tiles, off, val, lv, cv, sites, cov, totals);
  if (e != hipSuccess) return (int)e;
  if ((rc = bsc_dev_bigwig_heads(&g, n_tiles, off, sites, hcnt, grid, stream))) return rc;
  if ((rc = bsc_dev_scan_u64(hcnt, hoff, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream))) return rc;
  if ((rc = bsc_dev_bigwig_windows(&g, n_tiles, off, hoff, sites, wbeg, totals, grid, stream))) return rc;
  const uint64_t units = 2u * n; /* at most: every site a section and a window of its own */
  const unsigned rgrid = (unsigned)((units + BW_WAVES - 1u) / BW_WAVES < cap ? (units + BW_WAVES - 1u) / BW_WAVES : cap);
  e = tracks == 1u   ? bwcov_reduce<1u>(rgrid, s, g, n_tiles, off, hoff, sites, cov, wbeg, lv, cv, totals)
      : tracks == 2u ? bwcov_reduce<2u>(rgrid, s, g, n_tiles, off, hoff, sites, cov, wbeg, lv, cv, totals)
                     : bwcov_reduce<3u>(rgrid, s, g, n_tiles, off, hoff, sites, cov, wbeg, lv, cv, totals);
  return (int)e;
}
