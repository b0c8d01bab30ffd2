/*
 * bigwig_dev.h — the device helpers the bigWig kernels share (csrc/bigwigdev.hip: the level track; csrc/bwcovdev.hip: the coverage track
 * and both tracks in one sweep): the launch's arguments, the divisions by multiply-high, m by bisection, the site predicate, the rank of a
 * lane inside its tile, the window of a start.  include/bscall_amd.h has the rule; nothing here does floating-point arithmetic.
 *
 * rank / S and start / reduction go through a 64-bit multiply-high with ceil(2^64 / d), exact for a 32-bit dividend and any divisor of
 * 2 .. 2^32 - 1 (d = 1: the dividend itself) — the compiler's expansion of a division by a variable goes through a floating-point
 * reciprocal; m is found by bisection over 0 .. 1000 for the same reason.
 */
#ifndef BSC_BIGWIG_DEV_H
#define BSC_BIGWIG_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"

static_assert(sizeof(bsc_vcf_rec) == 128 && sizeof(bsc_vcf_core) == 64, "bsc_vcf_rec is 128 bytes, its core the first 64");
static_assert(sizeof(bsc_bw_sum) == 40, "a summary is 40 bytes");

#define BW_WAVES 4u

struct bw_args {
  const uint8_t *core, *aux; /* 64 bytes per position each */
  const uint8_t *emit;       /* the chain's byte per position, or NULL */
  uint64_t n;                /* positions */
  int32_t all_contexts;
  uint32_t min_cov, min_phred;
  int32_t pass_only;
  uint32_t x0, chrom_id;
  uint32_t S, red;
  uint64_t S_magic, red_magic; /* ceil(2^64 / d), d >= 2 */
};

/* v / d, v < 2^32 */
__device__ __forceinline__ uint32_t bw_div(uint32_t v, uint32_t d, uint64_t magic) {
  return d == 1u ? v : (uint32_t)__umul64hi((uint64_t)v, magic);
}

/* (2000 a + n) / (2 n), n = a + b > 0: the largest q of 0 .. 1000 with 2 n q <= 2000 a + n */
__device__ __forceinline__ unsigned bw_m(uint64_t a, uint64_t n) {
  const uint64_t num = 2000ull * a + n, den = 2ull * n;
  unsigned lo = 0u, hi = 1000u;
  while (lo < hi) {
    const unsigned mid = (lo + hi + 1u) >> 1;
    if (den * mid <= num) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

/* entry i < n: is it a site, and its a and b (the per-cytosine rule, restated from the header) */
__device__ __forceinline__ bool bw_site_of(const bw_args &g, uint64_t i, uint32_t &a, uint32_t &b) {
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

__device__ __forceinline__ unsigned bw_lanes_below(unsigned long long mask, unsigned lane) {
  return (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}

/* the window of a start */
__device__ __forceinline__ uint32_t bw_window(const bw_args &g, uint32_t start) { return bw_div(start, g.red, g.red_magic); }

/* ceil(2^64 / d) (host) */
static inline uint64_t bw_magic(uint32_t d) { return d < 2u ? 0ull : 0xffffffffffffffffull / d + 1ull; }

#endif
