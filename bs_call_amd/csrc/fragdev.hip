/*
 * fragdev.hip — the per-region fragment methylation summary of a block (include/bscall_amd.h has the rule: COUNTS, SITE, BYTE, STATE of the
 * read-level CpG table, REGION of the region summary; IN, the classes, SUMS, TOTALS; csrc/frag.c the host form, which is the checker): per
 * attached region the templates that are mostly unmethylated, mixed and mostly methylated within it — from the prepared templates, their read
 * bytes and the block's reference codes, while they are in HBM.  Nothing is written but the regions' accumulators and eight totals.
 *
 *   (the site pass is the read-level table's: bsc_dev_launch_cr_sites, cpgreadsdev.hip -> tile_mask[k], a bit per SITE of tile k = positions
 *   x + 64 k ..)
 *   bsc_frag_walk_kernel  one wave per template, grid-stride.
 *     search   the template's sites lie in [a, b) (positions of the C).  Its candidates are the regions of index [lo, hi): hi = the first
 *              region with start >= b, lo = the first whose running maximum of the ends is >= a — two searches over sorted arrays, 64-ary:
 *              every lane probes one of 64 evenly spaced entries and a ballot keeps the one interval that holds the answer, three rounds
 *              for 2^18 regions where a binary search takes eighteen dependent loads.  A superset: each lane tests its own region.
 *     strip    cr_round (cpgreads_dev.h) gives the M and U masks of the tiles the span touches; lane 0 puts them into the wave's strip
 *              in LDS, FR_STRIP tiles a chunk.  A span of more tiles (the 5 000-base read) goes in chunks; the lanes' k and m carry
 *              across the chunks of one round, and the strip is made again for every round of candidates (a template that fits one
 *              chunk, which is every template of a short-read run, makes it once).
 *     regions  64 candidates a round, one lane each: k and m are popcounts of the strip's masks under the region's position range, the
 *              partial tiles at its two ends masked.  A lane with k >= 1 does one 64-bit atomicAdd (short) or up to five (frags, the
 *              class, K, Mm, disc) into its region's row.  Integer adds are exact in any order: the result is a function of the input.
 *     long     a region longer than long_len bases is skipped where it stands and tested from the short list long_idx instead, by every
 *              template, behind the candidates' rounds: its end stays out of the running maximum, so that a chromosome-long region
 *              listed first does not make every template's candidates start at 0.
 *     totals   the lanes' seven sums and the wave's template count meet in the workgroup's LDS and leave it as eight 64-bit atomic adds.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "recstream_dev.h"
#include "cpgreads_dev.h"

static_assert(sizeof(bsc_template) == 40, "bsc_template is 40 bytes");
static_assert(sizeof(bsc_meth_region) == 8, "bsc_meth_region is 8 bytes");
static_assert(BSC_FRAG_N_SUMS == 8 && BSC_FRAG_N_TOTALS == 8, "eight sums a region, eight totals a call");

#define FR_WAVES 4u
#define FR_STRIP 64u /* tiles a chunk: 4 096 positions */

/* the first index k of v[0 .. n) (entries STRIDE words apart, non-decreasing) with v[k] >= key; wave-uniform in and out */
template <unsigned STRIDE>
__device__ __forceinline__ uint32_t fr_lower_bound(const uint32_t *__restrict__ v, uint32_t n, uint64_t key, unsigned lane) {
  uint64_t l = 0, h = n;
  while (l < h) {
    const uint64_t step = (h - l + 63u) / 64u;
    const uint64_t idx = l + (uint64_t)lane * step;
    const bool below = idx < h && (uint64_t)v[idx * STRIDE] < key;
    const unsigned c = (unsigned)__popcll(__ballot(below)); /* a prefix of the lanes: v is sorted */
    if (c == 0u) h = l;
    else {
      const uint64_t nh = l + (uint64_t)c * step; /* the first probe that is not below, or beyond the range */
      l = l + (uint64_t)(c - 1u) * step + 1u;
      h = nh < h ? nh : h;
    }
  }
  return (uint32_t)l;
}

extern "C" __global__ __launch_bounds__(256) void bsc_frag_walk_kernel(const bsc_template *__restrict__ tpl, uint32_t nr, const uint8_t *__restrict__ seq,
                                                                       uint64_t seq_bytes, uint32_t x, uint32_t y, unsigned min_qual,
                                                                       const unsigned long long *__restrict__ tile_mask,
                                                                       const bsc_meth_region *__restrict__ reg, uint32_t n_reg,
                                                                       const uint32_t *__restrict__ maxend, const uint32_t *__restrict__ long_idx,
                                                                       uint32_t n_long, uint32_t long_len, uint32_t min_sites, uint32_t u_max_pct,
                                                                       uint32_t m_min_pct, unsigned long long *__restrict__ acc,
                                                                       unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long s_mm[FR_WAVES][FR_STRIP], s_mu[FR_WAVES][FR_STRIP];
  __shared__ unsigned long long s_tot[BSC_FRAG_N_TOTALS];
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  if (threadIdx.x < BSC_FRAG_N_TOTALS) s_tot[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long l_frags = 0, l_cu = 0, l_cx = 0, l_cm = 0, l_k = 0, l_m = 0, l_disc = 0; /* per lane */
  unsigned long long t_any = 0;                                                               /* wave-uniform */
  for (uint32_t i = blockIdx.x * FR_WAVES + wid; i < nr; i += gridDim.x * FR_WAVES) {
    const bsc_template *tp = tpl + i; /* one address a wave: the loads are broadcast */
    cr_tpl t;
    t.bs = tp->bs_strand;
    if (t.bs != 1u && t.bs != 2u) continue; /* wave-uniform */
    uint64_t lo_p = ~0ull, hi_p = 0ull;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint64_t len = tp->len[k], off = tp->off[k];
      const bool have = len != 0u && off <= seq_bytes && len <= seq_bytes - off;
      t.pos[k] = tp->pos[k];
      t.end[k] = have ? t.pos[k] + len : t.pos[k]; /* (empty: no q lies in it) */
      t.off[k] = off;
      if (have) {
        lo_p = t.pos[k] < lo_p ? t.pos[k] : lo_p;
        hi_p = t.end[k] > hi_p ? t.end[k] : hi_p;
      }
    }
    if (hi_p == 0ull) continue;
    /* the sites that can have a state: p in [lo, hi) for C2T, [lo - 1, hi - 1) for G2A, within x .. y */
    const uint64_t sh = t.bs == 2u ? 1u : 0u;
    uint64_t a = lo_p >= sh ? lo_p - sh : 0ull, b = hi_p - sh; /* [a, b) */
    if (a < x) a = x;
    if (b > (uint64_t)y + 1u) b = (uint64_t)y + 1u;
    if (a >= b) continue;
    const uint32_t tile_a = (uint32_t)((a - x) >> 6), tile_b = (uint32_t)((b - 1u - x) >> 6);
    const uint32_t n_chunks = (tile_b - tile_a) / FR_STRIP + 1u;
    /* the candidates: start < b and end >= a */
    uint32_t c_hi = 0u, c_lo = 0u;
    if (n_reg) {
      c_hi = fr_lower_bound<2>(reinterpret_cast<const uint32_t *>(reg), n_reg, b, lane);
      c_lo = fr_lower_bound<1>(maxend, n_reg, a, lane);
    }
    const uint32_t r_main = c_hi > c_lo ? (c_hi - c_lo + 63u) / 64u : 0u, r_long = (n_long + 63u) / 64u;
    const uint32_t rounds = r_main + r_long ? r_main + r_long : 1u; /* (one round at least: the template's own count) */
    unsigned kt = 0u;
    for (uint32_t round = 0; round < rounds; round++) {
      /* this lane's region and the positions of it that the template's sites can lie in: [ps, pe] */
      bool valid = false;
      uint32_t idx = 0u;
      uint64_t ps = 0, pe = 0;
      {
        bool have = false;
        if (round < r_main) {
          const uint64_t j = (uint64_t)c_lo + (uint64_t)round * 64u + lane;
          have = j < c_hi;
          idx = (uint32_t)j;
        } else if (round - r_main < r_long) {
          const uint64_t j = (uint64_t)(round - r_main) * 64u + lane;
          have = j < n_long;
          if (have) idx = long_idx[j];
        }
        if (have) {
          const bsc_meth_region rg = reg[idx];
          const bool is_long = rg.end - rg.start > long_len;
          ps = (uint64_t)rg.start + 1u;
          pe = rg.end;
          if (ps < a) ps = a;
          if (pe > b - 1u) pe = b - 1u;
          valid = ps <= pe && is_long == (round >= r_main);
        }
      }
      if (round != 0u && !__ballot(valid)) continue; /* wave-uniform */
      const uint32_t lo_off = (uint32_t)(ps - x), hi_off = (uint32_t)(pe - x); /* (valid lanes: x <= a <= ps <= pe <= y) */
      unsigned k = 0u, m = 0u;
      for (uint32_t chunk = 0; chunk < n_chunks; chunk++) {
        const uint32_t c0 = tile_a + chunk * FR_STRIP, c1 = tile_b - c0 < FR_STRIP ? tile_b : c0 + FR_STRIP - 1u;
        if (n_chunks > 1u || round == 0u) {
          rs_wave_sync(); /* the strip's last readers are done */
          for (uint32_t tile = c0; tile <= c1; tile++) {
            const unsigned long long ms = tile_mask[tile];
            unsigned long long mm = 0ull, mu = 0ull;
            if (ms) cr_round(t, seq, x, y, tile, ms, lane, min_qual, mm, mu);
            if (lane == 0u) {
              s_mm[wid][tile - c0] = mm;
              s_mu[wid][tile - c0] = mu;
            }
            if (round == 0u) kt += (unsigned)__popcll(mm | mu);
          }
          rs_wave_sync();
        }
        if (valid) {
          const uint32_t ta = lo_off >> 6, tb = hi_off >> 6;
          const uint32_t t0 = ta > c0 ? ta : c0, t1 = tb < c1 ? tb : c1;
          for (uint32_t tile = t0; tile <= t1; tile++) {
            unsigned long long mask = ~0ull;
            if (tile == ta) mask &= ~0ull << (lo_off & 63u);
            if (tile == tb) mask &= ~0ull >> (63u - (hi_off & 63u));
            const unsigned long long vm = s_mm[wid][tile - c0] & mask, vu = s_mu[wid][tile - c0] & mask;
            k += (unsigned)__popcll(vm | vu);
            m += (unsigned)__popcll(vm);
          }
        }
      }
      if (valid && k) {
        unsigned long long *row = acc + (uint64_t)idx * BSC_FRAG_N_SUMS;
        if (k < min_sites) atomicAdd(row + 7, 1ull);
        else {
          const uint64_t m100 = 100ull * m;
          const unsigned cls = m100 <= (uint64_t)u_max_pct * k ? 1u : (m100 >= (uint64_t)m_min_pct * k ? 3u : 2u);
          const bool disc = m > 0u && m < k;
          atomicAdd(row + 0, 1ull);
          atomicAdd(row + cls, 1ull);
          atomicAdd(row + 4, (unsigned long long)k);
          if (m) atomicAdd(row + 5, (unsigned long long)m);
          if (disc) atomicAdd(row + 6, 1ull);
          l_frags++;
          l_cu += cls == 1u;
          l_cx += cls == 2u;
          l_cm += cls == 3u;
          l_k += k;
          l_m += m;
          l_disc += disc;
        }
      }
    }
    t_any += kt != 0u;
  }
  /* once a kernel: the lanes' seven sums and the wave's count into the workgroup's eight (LDS atomics), then eight global ones */
  if (l_frags) {
    atomicAdd(&s_tot[1], l_frags);
    if (l_cu) atomicAdd(&s_tot[2], l_cu);
    if (l_cx) atomicAdd(&s_tot[3], l_cx);
    if (l_cm) atomicAdd(&s_tot[4], l_cm);
    atomicAdd(&s_tot[5], l_k);
    if (l_m) atomicAdd(&s_tot[6], l_m);
    if (l_disc) atomicAdd(&s_tot[7], l_disc);
  }
  if (lane == 0u && t_any) atomicAdd(&s_tot[0], t_any);
  __syncthreads();
  if (threadIdx.x < BSC_FRAG_N_TOTALS && s_tot[threadIdx.x]) atomicAdd(totals + threadIdx.x, s_tot[threadIdx.x]);
}

static unsigned bsc_frag_grid(uint64_t n_items, int num_cus) {
  uint64_t grid = (n_items + FR_WAVES - 1u) / FR_WAVES;
  /* eight workgroups of four waves a CU fill its SIMDs */
  if (grid > (uint64_t)num_cus * 8u) grid = (uint64_t)num_cus * 8u;
  return grid ? (unsigned)grid : 1u;
}

/*
 * the walk behind bsc_dev_launch_cr_sites: acc[n_reg][8] += and totals[8] += (the caller zeroes the totals).  reg: the attached regions, sorted
 * by (start, end); maxend[n_reg]: the running maximum of the ends of the regions that are not long; long_idx[n_long]: the indices of those
 * that are (end - start > long_len), each below n_reg.
 */
extern "C" int bsc_dev_launch_frag_walk(const void *tpl, uint32_t nr, const void *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, uint32_t min_qual,
                                        const void *tile_mask, const void *reg, uint32_t n_reg, const void *maxend, const void *long_idx, uint32_t n_long,
                                        uint32_t long_len, uint32_t min_sites, uint32_t u_max_pct, uint32_t m_min_pct, void *acc, void *totals, int num_cus,
                                        void *stream) {
  if (nr == 0) return 0;
  hipLaunchKernelGGL(bsc_frag_walk_kernel, dim3(bsc_frag_grid(nr, num_cus)), dim3(256), 0, (hipStream_t)stream, (const bsc_template *)tpl, nr,
                     (const uint8_t *)seq, seq_bytes, x, y, min_qual, (const unsigned long long *)tile_mask, (const bsc_meth_region *)reg, n_reg,
                     (const uint32_t *)maxend, (const uint32_t *)long_idx, n_long, long_len, min_sites, u_max_pct, m_min_pct, (unsigned long long *)acc,
                     (unsigned long long *)totals);
  return (int)hipGetLastError();
}
