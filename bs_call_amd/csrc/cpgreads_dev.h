/*
 * cpgreads_dev.h — what the walks over the prepared templates share (include/bscall_amd.h: COUNTS, BYTE, STATE): a template's fields as a wave
 * reads them, BYTE of a lane, the M and U masks of one round over a tile's sites, and the state of one bit of them.  Used by the read-level CpG
 * table (cpgreadsdev.hip) and by the allele-specific methylation table (asmdev.hip).  Device code only.
 */
#ifndef BSC_CPGREADS_DEV_H
#define BSC_CPGREADS_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

/* a template's fields as the walk reads them; a read that is absent, or lies outside the read buffer, has len 0 */
struct cr_tpl {
  uint64_t pos[2], end[2], off[2]; /* end: one past the read's last position */
  unsigned bs;
};

/* BYTE(t, q) of this lane: -1 = none.  q within x .. y is the caller's */
__device__ __forceinline__ int cr_byte(const cr_tpl &t, const uint8_t *__restrict__ seq, uint64_t q, unsigned min_qual) {
#pragma unroll
  for (int k = 0; k < 2; k++)
    if (q >= t.pos[k] && q < t.end[k]) {
      const unsigned b = seq[t.off[k] + (q - t.pos[k])];
      if ((b >> 2) >= min_qual && (b >> 2) < 63u) return (int)b;
    }
  return -1;
}

/* the M and U masks of one round: tile `tile` of the block, m its sites */
__device__ __forceinline__ void cr_round(const cr_tpl &t, const uint8_t *__restrict__ seq, uint32_t x, uint32_t y, uint32_t tile, unsigned long long m,
                                         unsigned lane, unsigned min_qual, unsigned long long &mm, unsigned long long &mu) {
  bool is_m = false, is_u = false;
  if ((m >> lane) & 1ull) {
    const uint64_t q = (uint64_t)x + (uint64_t)tile * 64u + lane + (t.bs == 2u ? 1u : 0u);
    if (q <= y) { /* (q >= x: the tile's positions are) */
      const int b = cr_byte(t, seq, q, min_qual);
      if (b >= 0) {
        const unsigned base = (unsigned)b & 3u;
        is_m = base == (t.bs == 1u ? 1u : 2u);
        is_u = base == (t.bs == 1u ? 3u : 0u);
      }
    }
  }
  mm = __ballot(is_m);
  mu = __ballot(is_u);
}

/* the state (0 none, 1 M, 2 U) of the site at bit j of a round */
__device__ __forceinline__ unsigned cr_state_at(unsigned long long mm, unsigned long long mu, unsigned j) {
  return (unsigned)((mm >> j) & 1ull) | (unsigned)((mu >> j) & 1ull) << 1;
}

#endif
