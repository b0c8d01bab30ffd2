/*
 * methregionsdev.hip — the per-region methylation summary on the device: for every attached region {start, end} the four sums
 * {sites, sum of a, sum of b, sum of pct} over the cytosines inside it (include/bscall_amd.h has the rule; the host form
 * csrc/methregions.c is the checker).  The first kernels here that REDUCE over positions: an interval that several tiles, and several
 * blocks, contribute to.  The per-position arrays are dense — entry i is position x0 + i — so an interval is a difference of two prefix
 * sums, whatever its length and however the regions overlap, nest or repeat:
 *
 *   bsc_meth_regions_tile_kernel    one wave per tile of 64 positions: every lane evaluates the site predicate on its entry, the wave
 *                                   adds the four values up -> planes[k][tile], k = 0 .. 3 (u64; planes[k][n_tiles] = 0)
 *   (exclusive scan of each plane, rocPRIM u64: sort.hip; the entry behind the last tile = the whole array's sum)
 *   bsc_meth_regions_region_kernel  one wave per CANDIDATE region: in index space i_lo = clamp(start + 1 - x0), i_hi = clamp(end + 1 - x0)
 *                                   into [0, n] (64-bit signed), prefix(i) = scan[i / 64] + the wave's sum over that tile's lanes
 *                                   < i % 64 — the tile evaluated again, and not read at all where i % 64 == 0 —, and
 *                                   prefix(i_hi) - prefix(i_lo), where not all zero, is added to acc[r] by lane 0 with an ordinary load,
 *                                   add and store: one wave owns one region per launch and launches on a stream are ordered, so there
 *                                   are no atomics and the result does not depend on scheduling.
 *
 * Whether an entry is a site is decided from its first 16 bytes (emit, gt, flt, phred, cg) and, for a candidate only, the counts behind
 * them; with the chain's byte per position (emit: not 0 <=> a record is written) a position without a record costs that byte.  The
 * predicate and the percentage are restated here from the header, as the combined-strand encoder restated the per-cytosine rule.
 *
 * All arithmetic is integer; the percentage is found by bisection over 0 .. 100 (a 64-bit division by a variable would be expanded
 * through a floating-point reciprocal).  Every sum is 64 bits from the first add: a lane's a may be 2^32 - 1.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"

static_assert(sizeof(bsc_vcf_rec) == 128 && sizeof(bsc_vcf_core) == 64, "bsc_vcf_rec is 128 bytes, its core the first 64");
static_assert(sizeof(bsc_meth_region) == 8, "a region is two u32");

#define MR_WAVES 4u

struct mr_args {
  const uint8_t *core, *aux; /* 64 bytes per position each */
  const uint8_t *emit;       /* the chain's byte per position, or NULL */
  uint64_t n;                /* positions */
  int32_t all_contexts;
  uint32_t min_cov, min_phred;
  int32_t pass_only;
};

struct mr_sums {
  unsigned long long v[4]; /* sites, a, b, pct */
};

/* (200 a + n) / (2 n), n = a + b > 0: the largest q of 0 .. 100 with 2 n q <= 200 a + n */
__device__ __forceinline__ unsigned mr_pct(uint64_t a, uint64_t n) {
  const uint64_t num = 200ull * a + n, den = 2ull * n;
  unsigned lo = 0u, hi = 100u;
  while (lo < hi) {
    const unsigned mid = (lo + hi + 1u) >> 1;
    if (den * mid <= num) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

/* entry i < n: is it a site, and its a and b */
__device__ __forceinline__ bool mr_site_of(const mr_args &g, uint64_t i, uint32_t &a, uint32_t &b) {
  if (g.emit && !g.emit[i]) return false;
  const uint4 v0 = *reinterpret_cast<const uint4 *>(g.core + i * 64u);
  const unsigned emit = v0.y & 0xffu, gt = (v0.y >> 8) & 0xffu, flt = v0.z & 0xffu, phred = (v0.z >> 8) & 0xffu, cg = v0.z >> 24;
  if (!emit || (gt != 4u && gt != 7u)) return false;
  if (cg != 'C' && !(g.all_contexts && cg == 'H')) return false;
  if (phred < g.min_phred || (g.pass_only && flt)) return false;
  const uint4 c1 = reinterpret_cast<const uint4 *>(g.aux + i * 64u)[1]; /* counts[4 .. 7] */
  const bool minus = gt == 7u;
  a = minus ? c1.z : c1.y; /* counts[6] : counts[5] */
  b = minus ? c1.x : c1.w; /* counts[4] : counts[7] */
  return (uint64_t)a + b >= (uint64_t)(g.min_cov > 1u ? g.min_cov : 1u);
}

/* the wave's four sums over the lanes < lanes of the tile: the same in every lane */
__device__ __forceinline__ mr_sums mr_tile_sums(const mr_args &g, uint64_t tile, unsigned lane, unsigned lanes) {
  const uint64_t i = tile * 64u + lane;
  uint32_t a = 0u, b = 0u;
  const bool site = lane < lanes && i < g.n && mr_site_of(g, i, a, b);
  mr_sums s;
  s.v[0] = (unsigned long long)__popcll(__ballot(site));
  s.v[1] = site ? a : 0ull;
  s.v[2] = site ? b : 0ull;
  s.v[3] = site ? mr_pct(a, (uint64_t)a + b) : 0ull;
  if (s.v[0]) { /* wave-uniform */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      s.v[1] += __shfl_xor(s.v[1], d);
      s.v[2] += __shfl_xor(s.v[2], d);
      s.v[3] += __shfl_xor(s.v[3], d);
    }
  }
  return s;
}

/* planes: [4][n_tiles + 1] */
extern "C" __global__ __launch_bounds__(256) void bsc_meth_regions_tile_kernel(mr_args g, uint32_t n_tiles, unsigned long long *__restrict__ planes) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)n_tiles + 1u;
  if (blockIdx.x == 0 && threadIdx.x < 4u) planes[threadIdx.x * stride + n_tiles] = 0ull;
  for (uint32_t tile = blockIdx.x * MR_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * MR_WAVES) {
    const mr_sums s = mr_tile_sums(g, tile, lane, 64u);
    const unsigned long long mine = lane == 0u ? s.v[0] : (lane == 1u ? s.v[1] : (lane == 2u ? s.v[2] : s.v[3])); /* (no indexed register array) */
    if (lane < 4u) planes[lane * stride + tile] = mine;
  }
}

/* the four sums over entries [0, i), i <= n */
__device__ __forceinline__ mr_sums mr_prefix(const mr_args &g, uint32_t n_tiles, const unsigned long long *__restrict__ scan, uint64_t i, unsigned lane) {
  const uint64_t tile = i >> 6, stride = (uint64_t)n_tiles + 1u; /* tile <= n_tiles; == only where i == n is a multiple of 64 */
  const unsigned rem = (unsigned)(i & 63u);
  mr_sums s;
#pragma unroll
  for (int k = 0; k < 4; k++) s.v[k] = scan[k * stride + tile];
  if (rem) {
    const mr_sums t = mr_tile_sums(g, tile, lane, rem);
#pragma unroll
    for (int k = 0; k < 4; k++) s.v[k] += t.v[k];
  }
  return s;
}

/* regions[r], r in [r_lo, r_hi): acc[r][0 .. 3] += its sums over positions x0 .. x0 + n - 1 */
extern "C" __global__ __launch_bounds__(256) void bsc_meth_regions_region_kernel(mr_args g, uint32_t n_tiles, const unsigned long long *__restrict__ scan,
                                                                                 const bsc_meth_region *__restrict__ regions, uint32_t r_lo,
                                                                                 uint32_t r_hi, uint32_t x0, unsigned long long *acc) {
  const unsigned lane = threadIdx.x & 63u;
  const int64_t n = (int64_t)g.n;
  for (uint64_t r = (uint64_t)r_lo + blockIdx.x * MR_WAVES + (threadIdx.x >> 6); r < r_hi; r += (uint64_t)gridDim.x * MR_WAVES) {
    const bsc_meth_region reg = regions[r];
    /* the site at x0 + i lies inside iff start < x0 + i <= end */
    int64_t i_lo = (int64_t)reg.start + 1 - (int64_t)x0, i_hi = (int64_t)reg.end + 1 - (int64_t)x0;
    i_lo = i_lo < 0 ? 0 : (i_lo > n ? n : i_lo);
    i_hi = i_hi < 0 ? 0 : (i_hi > n ? n : i_hi);
    if (i_hi <= i_lo) continue; /* wave-uniform: a candidate of the superset that holds nothing of this array */
    const mr_sums hi = mr_prefix(g, n_tiles, scan, (uint64_t)i_hi, lane), lo = mr_prefix(g, n_tiles, scan, (uint64_t)i_lo, lane);
    if (lane == 0u && hi.v[0] != lo.v[0]) { /* a site less, and nothing is added */
      unsigned long long *const q = acc + r * 4u;
#pragma unroll
      for (int k = 0; k < 4; k++) q[k] = q[k] + (hi.v[k] - lo.v[k]);
    }
  }
}

extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

/*
 * core[n] / aux[n]: the per-position arrays, entry i = position x0 + i; emit: the chain's byte per position or NULL.  planes / scan:
 * 4 x (n / 64 rounded up + 1) u64 each; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of the tiles + 1.  The tile pass and the four scans always
 * run (scan[k][n_tiles] = the array's totals); the region pass over regions[r_lo .. r_hi) only where that range is not empty.
 */
extern "C" int bsc_dev_launch_meth_regions(const void *core, const void *aux, const void *emit, uint64_t n, uint32_t x0, const bsc_meth_params *par,
                                           void *planes, void *scan, void *scan_tmp, size_t scan_tmp_bytes, const void *regions, uint32_t r_lo,
                                           uint32_t r_hi, void *acc, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!par || !n || n > 0xffffffffull || !planes || !scan) return (int)hipErrorInvalidValue;
  if (r_hi > r_lo && (!regions || !acc)) return (int)hipErrorInvalidValue;
  mr_args g;
  g.core = (const uint8_t *)core;
  g.aux = (const uint8_t *)aux;
  g.emit = (const uint8_t *)emit;
  g.n = n;
  g.all_contexts = par->contexts == BSC_METH_ALL;
  g.min_cov = par->min_cov;
  g.min_phred = par->min_phred;
  g.pass_only = par->pass_only != 0;
  const uint32_t n_tiles = (uint32_t)((n + 63u) / 64u);
  const unsigned cap = (unsigned)(num_cus > 0 ? num_cus : 1) * 8u;
  unsigned grid = (n_tiles + MR_WAVES - 1u) / MR_WAVES;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(bsc_meth_regions_tile_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (unsigned long long *)planes);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  for (unsigned k = 0; k < 4u; k++) {
    const size_t off = (size_t)k * ((size_t)n_tiles + 1u) * 8u;
    const int rc = bsc_dev_scan_u64((const char *)planes + off, (char *)scan + off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
    if (rc) return rc;
  }
  if (r_hi <= r_lo) return 0;
  grid = (r_hi - r_lo + MR_WAVES - 1u) / MR_WAVES;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(bsc_meth_regions_region_kernel, dim3(grid), dim3(256), 0, s, g, n_tiles, (const unsigned long long *)scan,
                     (const bsc_meth_region *)regions, r_lo, r_hi, x0, (unsigned long long *)acc);
  return (int)hipGetLastError();
}
