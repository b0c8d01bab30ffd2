/*
 * mbiasdev.hip — the M-bias table on the device (include/bscall_amd.h: READ, END, CYCLE, G(j), COUNTS, CONTEXT, TABLE, TOTALS), one walk over the
 * RAW templates as the device reader leaves them in HBM.  csrc/mbias.c is the host form and the checker.
 *
 * A wave per template, its two reads in turn, 64 consecutive read bytes a round: lane l owns byte j0 + l, so the loads of seq are coalesced.
 * Everything that decides a read's fate — the template's fields, the READ tests, the whole mismatch list — is the same for the 64 lanes:
 * the wave's index is made a scalar (readfirstlane), so the template and the list come in by scalar loads and the list's loops do not
 * diverge.  The list is walked twice: once to validate it (a malformed list skips the read before a single byte is touched), then round by
 * round — entries that end before the round are folded into two wave-wide sums (bytes taken out, genome offset added), the few that overlap
 * the round are applied per lane as compares and adds.  The positions of non-MISMS entries of a valid list never decrease, so a round looks
 * at the entries that overlap it and at no other: O(entries + rounds) per read.
 * The reference codes a lane needs (r(G) and two neighbours on the strand's side) are byte loads at G - x .. G - x +- 2: within a round the
 * lanes' G are consecutive except across an indel, so the three loads of a wave hit the same two or three lines.
 * Counters: the cells of cycles below MB_LDS_CYCLES are u32 in LDS ([12 bins][min(n_cycles, 256)][2 states], 24 KiB at the most), updated
 * with LDS atomics and flushed once, at the workgroup's end, non-zero cells alone, by 64-bit atomic adds; the cells of cycles 256 .. 1023
 * (reads longer than a short-read machine's) are added to the u64 table in HBM directly.  Integer atomics alone: the bytes of the table are a
 * function of the input, whatever the grid.
 * Measured: the walk is bound by the CU's one scalar unit, where all of the wave-uniform work above runs — not by the
 * loads' bytes or their latency.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"

#define MB_THREADS 512u
#define MB_WAVES 8u
#define MB_LDS_CYCLES 256u
#define MB_WG_PER_CU 3u /* the workgroups of this kernel a CU holds at once: see bsc_dev_launch_mbias */
#define MB_SUB 2u /* rounds of 64 bytes whose loads are in flight together */
/* A u32 cell in LDS receives at most one count per byte walked, so it cannot wrap while the workgroup's eight waves together walk fewer than
 * 2^32 bytes through LDS: every wave has a budget of floor((2^32 - 1) / 8) bytes, a read that does not fit into what is left of it adds to the
 * table in HBM directly, as the cycles beyond MB_LDS_CYCLES do (bsc_dev_launch_mbias: the grid does not enter the bound). */
#define MB_WAVE_LDS_BYTES (0xffffffffull / MB_WAVES)

struct mb_args {
  const bsc_raw_template *raw;
  const uint8_t *seq;
  const bsc_misms *misms;
  const uint8_t *ref;
  unsigned long long *counts, *totals;
  uint64_t seq_bytes, n_misms;
  uint32_t nr, x, y, min_qual, n_cycles;
};

/* G(j)'s malformed-list test: the same for every lane */
__device__ __forceinline__ bool mb_list_ok(const bsc_misms *__restrict__ m, uint32_t nm, uint32_t len) {
  uint64_t cursor = 0;
  for (uint32_t z = 0; z < nm; z++) {
    const uint32_t type = m[z].type;
    const uint64_t pos = m[z].position, end = pos + m[z].size;
    if (type == BSC_MISMS_MISMS) continue;
    if (type > BSC_MISMS_SOFT || pos < cursor) return false;
    if (type == BSC_MISMS_INS) {
      cursor = pos;
      continue;
    }
    if (type == BSC_MISMS_SOFT && z != 0 && z != nm - 1u) return false;
    if (end > len) return false;
    cursor = end;
  }
  return true;
}

extern "C" __global__ __launch_bounds__(MB_THREADS) void bsc_mbias_walk_kernel(mb_args a) {
  __shared__ uint32_t cells[BSC_MBIAS_N_BINS * MB_LDS_CYCLES * 2u];
  __shared__ unsigned long long wg_tot[BSC_MBIAS_N_TOTALS];
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wid = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t lc = a.n_cycles < MB_LDS_CYCLES ? a.n_cycles : MB_LDS_CYCLES; /* the cycles kept in LDS */
  const uint32_t n_lds = BSC_MBIAS_N_BINS * lc * 2u;
  for (uint32_t i = threadIdx.x; i < n_lds; i += MB_THREADS) cells[i] = 0;
  if (threadIdx.x < BSC_MBIAS_N_TOTALS) wg_tot[threadIdx.x] = 0;
  __syncthreads();
  /* the wave's totals, the same value in every lane (ballots) */
  unsigned long long n_walked = 0, n_g = 0, n_cell = 0, n_over = 0, n_cm = 0, n_cu = 0, n_skip = 0;
  uint64_t budget = MB_WAVE_LDS_BYTES;
  for (uint64_t i = (uint64_t)blockIdx.x * MB_WAVES + wid; i < a.nr; i += (uint64_t)gridDim.x * MB_WAVES) {
    const bsc_raw_template *__restrict__ r = a.raw + i;
    const unsigned bs = r->bs_strand, orient = r->orientation;
    if (bs == 0) continue;
#pragma unroll 1
    for (unsigned k = 0; k < 2; k++) {
      const uint32_t len = r->len[k];
      if (len == 0) continue;
      const uint64_t off = r->off[k], mo = r->misms_off[k];
      const uint32_t nm = r->n_misms[k];
      bool ok = off <= a.seq_bytes && len <= a.seq_bytes - off && mo <= a.n_misms && nm <= a.n_misms - mo && bs <= 2u && orient <= 1u;
      const bsc_misms *__restrict__ m = a.misms + (ok ? mo : 0);
      if (ok) ok = mb_list_ok(m, nm, len);
      if (!ok) {
        n_skip++;
        continue;
      }
      n_walked++;
      const bool lds_ok = len <= budget;
      if (lds_ok) budget -= len;
      const uint8_t *__restrict__ b = a.seq + off;
      const uint64_t pos = r->pos[k];
      const unsigned bin0 = ((k ^ orient) * 2u + (bs - 1u)) * 3u;
      const bool c2t = bs == 1u;
      uint32_t z = 0;
      uint64_t rem_u = 0, ins_u = 0; /* of the entries that end at or before the round's first byte */
      for (uint64_t j0 = 0; j0 < len; j0 += 64u * MB_SUB) {
        /* MB_SUB rounds of 64 bytes at a time, in three steps — G of every lane from the list, then every load (the byte and the three
         * reference codes: their addresses need the list alone, so none waits for another), then the counting — so that the loads of the
         * rounds are in flight together (worth 8 % when it was measured; the waves wait in a fifth of their cycles only) */
        bool has_g[MB_SUB];
        uint64_t jj[MB_SUB], gi[MB_SUB];
#pragma unroll
        for (unsigned s = 0; s < MB_SUB; s++) {
          const uint64_t js = j0 + 64u * s;
          while (z < nm) {
            const uint32_t type = m[z].type;
            const uint64_t p = m[z].position, size = m[z].size;
            if (type == BSC_MISMS_MISMS) {
              z++;
            } else if (type == BSC_MISMS_INS) {
              if (p > js) break;
              ins_u += size;
              z++;
            } else {
              if (p + size > js) break;
              rem_u += size;
              z++;
            }
          }
          const uint64_t j = js + lane;
          uint64_t rem = rem_u, ins = ins_u;
          bool taken = false;
          for (uint32_t zz = z; zz < nm; zz++) {
            const uint32_t type = m[zz].type;
            const uint64_t p = m[zz].position, size = m[zz].size;
            if (type == BSC_MISMS_MISMS) continue;
            if (p >= js + 64u) break;
            if (type == BSC_MISMS_INS) {
              if (j >= p) ins += size;
            } else if (j >= p + size) {
              rem += size;
            } else if (j >= p) {
              taken = true;
            }
          }
          const uint64_t G = pos + (j - rem) + ins;
          has_g[s] = j < len && !taken && G >= a.x && G <= a.y;
          jj[s] = j;
          gi[s] = G - a.x; /* with a G: <= y - x, so gi + 2 is within the y - x + 3 codes */
        }
        unsigned byte[MB_SUB], r0[MB_SUB], n1[MB_SUB], n2[MB_SUB];
#pragma unroll
        for (unsigned s = 0; s < MB_SUB; s++) {
          byte[s] = r0[s] = n1[s] = n2[s] = 0;
          if (has_g[s]) {
            byte[s] = b[jj[s]];
            r0[s] = a.ref[gi[s]];
            if (c2t) {
              n1[s] = a.ref[gi[s] + 1u];
              n2[s] = a.ref[gi[s] + 2u];
            } else {
              if (gi[s] >= 1u) n1[s] = a.ref[gi[s] - 1u];
              if (gi[s] >= 2u) n2[s] = a.ref[gi[s] - 2u];
            }
          }
        }
#pragma unroll
        for (unsigned s = 0; s < MB_SUB; s++) {
          bool cell = false, over = false, in_lds = false;
          unsigned ctx = 0, state = 0;
          uint32_t c = 0;
          const unsigned qual = byte[s] >> 2, base = byte[s] & 3u;
          if (has_g[s] && qual >= a.min_qual && qual < 63u) {
            const unsigned here = c2t ? 2u : 3u, partner = c2t ? 3u : 2u;
            bool has_ctx = true;
            if (n1[s] == partner) ctx = 0;
            else if (n1[s] == 0u) has_ctx = false;
            else if (n2[s] == partner) ctx = 1;
            else if (n2[s] == 0u) has_ctx = false;
            else ctx = 2;
            bool has_state = true;
            if (base == (c2t ? 1u : 2u)) state = 0;
            else if (base == (c2t ? 3u : 0u)) state = 1;
            else has_state = false;
            if (r0[s] == here && has_ctx && has_state) {
              c = (uint32_t)(k == 0 ? jj[s] : (uint64_t)len - 1u - jj[s]);
              over = c >= a.n_cycles;
              cell = !over;
              in_lds = cell && lds_ok && c < lc;
            }
          }
          if (in_lds) atomicAdd(&cells[((bin0 + ctx) * lc + c) * 2u + state], 1u);
          else if (cell) atomicAdd(&a.counts[((size_t)(bin0 + ctx) * a.n_cycles + c) * 2u + state], 1ull);
          n_g += (unsigned)__popcll(__ballot(has_g[s]));
          n_cell += (unsigned)__popcll(__ballot(cell));
          n_over += (unsigned)__popcll(__ballot(over));
          n_cm += (unsigned)__popcll(__ballot(cell && ctx == 0 && state == 0));
          n_cu += (unsigned)__popcll(__ballot(cell && ctx == 0 && state == 1));
        }
      }
    }
  }
  if (lane == 0) {
    if (n_walked) atomicAdd(&wg_tot[0], n_walked);
    if (n_g) atomicAdd(&wg_tot[1], n_g);
    if (n_cell) atomicAdd(&wg_tot[2], n_cell);
    if (n_over) atomicAdd(&wg_tot[3], n_over);
    if (n_cm) atomicAdd(&wg_tot[4], n_cm);
    if (n_cu) atomicAdd(&wg_tot[5], n_cu);
    if (n_skip) atomicAdd(&wg_tot[6], n_skip);
  }
  __syncthreads();
  /* the workgroup's one flush: cell i of LDS is (bin, c, state) = (i / (2 lc), (i / 2) % lc, i & 1) */
  for (uint32_t i = threadIdx.x; i < n_lds; i += MB_THREADS) {
    const uint32_t v = cells[i];
    if (v) {
      const uint32_t bin = i / (2u * lc), rest = i - bin * 2u * lc;
      atomicAdd(&a.counts[(size_t)bin * a.n_cycles * 2u + rest], (unsigned long long)v);
    }
  }
  if (threadIdx.x < BSC_MBIAS_N_TOTALS && wg_tot[threadIdx.x]) atomicAdd(&a.totals[threadIdx.x], wg_tot[threadIdx.x]);
}

/* counts: 12 * n_cycles * 2 u64, totals: eight u64, both ADDED to; n_cycles within 1 .. BSC_MBIAS_MAX_CYCLES, y >= x and the pointers'
 * alignment are the caller's (bsc_mbias_device).  The grid: a wave per template up to MB_WG_PER_CU workgroups a CU, the rest by grid stride.
 * Three, because three are resident: the kernel's 106 SGPRs allow 7 waves a SIMD (the compiler's listing, profiles/mbiasdev_resources.txt), a
 * workgroup of 8 waves puts 2 on each SIMD, so a fourth workgroup waits for a slot and runs as a tail on a third of the CU — measured, a grid of
 * four a CU takes 9.01 ms where three take 8.31; LDS (24 KiB of 160) and VGPRs (45) would admit more.  The LDS cells' bound
 * is per wave (MB_WAVE_LDS_BYTES), so no grid can make one wrap. */
extern "C" int bsc_dev_launch_mbias(const void *raw, uint32_t nr, const void *seq, uint64_t seq_bytes, const void *misms, uint64_t n_misms, uint32_t x,
                                    uint32_t y, const void *ref, uint32_t min_qual, uint32_t n_cycles, void *counts, void *totals, int num_cus,
                                    void *stream) {
  if (!nr) return 0;
  mb_args a;
  a.raw = (const bsc_raw_template *)raw;
  a.seq = (const uint8_t *)seq;
  a.misms = (const bsc_misms *)misms;
  a.ref = (const uint8_t *)ref;
  a.counts = (unsigned long long *)counts;
  a.totals = (unsigned long long *)totals;
  a.seq_bytes = seq_bytes;
  a.n_misms = n_misms;
  a.nr = nr;
  a.x = x;
  a.y = y;
  a.min_qual = min_qual;
  a.n_cycles = n_cycles;
  uint64_t grid = ((uint64_t)nr + MB_WAVES - 1u) / MB_WAVES;
  if (num_cus < 1) num_cus = 1;
  if (grid > (uint64_t)num_cus * MB_WG_PER_CU) grid = (uint64_t)num_cus * MB_WG_PER_CU;
  hipLaunchKernelGGL(bsc_mbias_walk_kernel, dim3((unsigned)grid), dim3(MB_THREADS), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
