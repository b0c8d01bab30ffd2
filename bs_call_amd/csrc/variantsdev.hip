/*
 * variantsdev.hip — the variant-only call set of a block: the records whose ALT column is not '.', selected from the per-position arrays a
 * block call left in HBM and packed for the encoders (include/bscall_amd.h has the rule, csrc/variants.c the host form).  About one record
 * in a thousand is one, so the cost is the selection: a byte per position and the 16-byte head of every emitted record, read once.
 *
 *   bsc_var_select_kernel   one wave per 64-position tile: the emit byte (where the array is given), behind it the first 16 bytes of the
 *                           core record — pos, emit, gt, ref_code, flt, phred and alt[2] lie in bytes 0..13 —, and byte 49 of aux
 *                           (rs_found) for the lanes that pass every other test.  The tile's ballot goes out as the count AND as the mask
 *                           (8 bytes a tile: the packing pass reads no head again).  The ten counters stay in the wave's registers over
 *                           its rounds (popcounts of ballots; the phred sum per lane, added across the wave once) and leave the workgroup
 *                           as ten 64-bit atomic adds — integer sums, no order.
 *   (exclusive scan of the tile counts: bsc_dev_scan_u32, sort.hip)
 *   bsc_var_pack_kernel     eight lanes per selected record, as bsc_compact_aux_emit_kernel (compact.hip): lanes 0-3 its core record, lanes
 *                           4-7 its aux half, 16 bytes a lane; records beyond the room are counted and not stored.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"

static_assert(sizeof(bsc_vcf_rec) == 128, "bsc_vcf_rec is 128 bytes");
static_assert(sizeof(bsc_var_params) == 16, "bsc_var_params is 16 bytes");

#define BSC_VAR_N_TOTALS 10

extern "C" __global__ __launch_bounds__(256) void bsc_var_select_kernel(const uint8_t *__restrict__ core, const uint8_t *__restrict__ aux,
                                                                        const uint8_t *__restrict__ emit_b, uint32_t n, uint32_t min_phred,
                                                                        int pass_only, int known_only, uint32_t *__restrict__ tile_cnt,
                                                                        unsigned long long *__restrict__ tile_mask,
                                                                        unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long s_tot[4][BSC_VAR_N_TOTALS];
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint32_t n_tiles = (n + 63u) / 64u;
  unsigned long long t_rec = 0, t_snp = 0, t_het = 0, t_pass = 0, t_known = 0, t_kp = 0, t_ts = 0, t_tv = 0; /* wave-uniform */
  unsigned long long ph = 0;                                                                              /* this lane's share of the phred sum */
  for (uint32_t tile = blockIdx.x * 4u + wid; tile < n_tiles; tile += gridDim.x * 4u) {
    const uint32_t i = tile * 64u + lane;
    bool sel = i < n && (!emit_b || emit_b[i] != 0);
    uint32_t gt = 0, ref_code = 0, flt = 0, phred = 0, alt0 = 0, alt1 = 0, rs = 0;
    if (sel) {
      const uint4 c0 = *reinterpret_cast<const uint4 *>(core + (uint64_t)i * 64u);
      gt = (c0.y >> 8) & 0xffu;
      ref_code = (c0.y >> 16) & 0xffu;
      flt = c0.z & 0xffu;
      phred = (c0.z >> 8) & 0xffu;
      alt0 = c0.w & 0xffu;
      alt1 = (c0.w >> 8) & 0xffu;
      sel = (c0.y & 0xffu) != 0 && alt0 != 0 && phred >= min_phred && (!pass_only || flt == 0);
    }
    if (sel) {
      rs = aux[(uint64_t)i * 64u + 49u]; /* bsc_vcf_rec.rs_found */
      sel = !known_only || rs != 0;
    }
    const unsigned long long m = __ballot(sel);
    if (lane == 0) {
      tile_cnt[tile] = (uint32_t)__popcll(m);
      tile_mask[tile] = m;
    }
    if (!m) continue; /* wave-uniform */
    const bool snp = sel && alt1 == 0;
    const bool acgt = alt0 == 'A' || alt0 == 'C' || alt0 == 'G' || alt0 == 'T';
    const bool tstv = snp && ref_code >= 1u && ref_code <= 4u && acgt;
    const uint32_t alt_code = alt0 == 'A' ? 1u : alt0 == 'C' ? 2u : alt0 == 'G' ? 3u : 4u;
    /* {A, G} = codes {1, 3}, {C, T} = {2, 4}: two different codes of one parity */
    const bool ts = tstv && alt_code != ref_code && ((alt_code ^ ref_code) & 1u) == 0;
    t_rec += (unsigned)__popcll(m);
    t_snp += (unsigned)__popcll(__ballot(snp));
    t_het += (unsigned)__popcll(__ballot(sel && gt <= 8u && ((0x16eu >> gt) & 1u))); /* 1, 2, 3, 5, 6, 8 */
    t_pass += (unsigned)__popcll(__ballot(sel && flt == 0));
    t_known += (unsigned)__popcll(__ballot(sel && rs != 0));
    t_kp += (unsigned)__popcll(__ballot(sel && rs != 0 && flt == 0));
    t_ts += (unsigned)__popcll(__ballot(ts));
    t_tv += (unsigned)__popcll(__ballot(tstv && !ts));
    if (sel) ph += phred;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) ph += __shfl_xor(ph, d);
  if (lane == 0) {
    unsigned long long *t = s_tot[wid];
    t[0] = t_rec;
    t[1] = t_snp;
    t[2] = t_rec - t_snp;
    t[3] = t_het;
    t[4] = t_pass;
    t[5] = t_known;
    t[6] = t_kp;
    t[7] = t_ts;
    t[8] = t_tv;
    t[9] = ph;
  }
  __syncthreads();
  if (threadIdx.x < BSC_VAR_N_TOTALS) {
    const unsigned long long v = s_tot[0][threadIdx.x] + s_tot[1][threadIdx.x] + s_tot[2][threadIdx.x] + s_tot[3][threadIdx.x];
    if (v) atomicAdd(totals + threadIdx.x, v);
  }
}

extern "C" __global__ __launch_bounds__(256) void bsc_var_pack_kernel(const uint8_t *__restrict__ core, const uint8_t *__restrict__ aux, uint32_t n,
                                                                      const uint32_t *__restrict__ tile_off,
                                                                      const unsigned long long *__restrict__ tile_mask,
                                                                      uint8_t *__restrict__ out, uint64_t out_cap,
                                                                      unsigned long long *__restrict__ total) {
  __shared__ uint8_t s_idx[4][64];
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const unsigned sub = lane & 7u, grp = lane >> 3;
  uint8_t *const idx = s_idx[wid];
  const uint32_t n_tiles = (n + 63u) / 64u;
  for (uint32_t tile = blockIdx.x * 4u + wid; tile < n_tiles; tile += gridDim.x * 4u) {
    const unsigned long long m = tile_mask[tile]; /* wave-uniform; a bit is set only for a position < n */
    const unsigned cnt = (unsigned)__popcll(m);
    const uint32_t off = tile_off[tile];
    if (tile == n_tiles - 1u && lane == 0) *total = (unsigned long long)off + cnt;
    if (!cnt) continue;
    if ((m >> lane) & 1ull) idx[__popcll(m & ((1ull << lane) - 1ull))] = (uint8_t)lane;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (unsigned base = 0; base < cnt; base += 8u) {
      const unsigned r = base + grp;
      const uint64_t slot = (uint64_t)off + r;
      if (r < cnt && slot < out_cap) { /* beyond the room: counted in *total, not stored */
        const uint64_t p = (uint64_t)tile * 64u + idx[r];
        const uint8_t *src = sub < 4u ? core + p * 64u + 16u * sub : aux + p * 64u + 16u * (sub - 4u);
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        *reinterpret_cast<uint4 *>(out + slot * 128u + 16u * sub) = v;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier(); /* the list is rewritten for the wave's next tile */
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

extern "C" int bsc_dev_scan_u32(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

static unsigned bsc_var_grid(uint32_t n_tiles, int num_cus) {
  unsigned grid = (n_tiles + 3u) / 4u;
  /* eight workgroups of four waves a CU fill its SIMDs; more would only add rounds of the ten atomics at the end */
  if (grid > (unsigned)num_cus * 8u) grid = (unsigned)num_cus * 8u;
  return grid ? grid : 1u;
}

/* the select pass and the scan: tile_cnt / tile_off (n + 63) / 64 words, tile_mask as many u64; totals: ten u64, zeroed by the caller */
extern "C" int bsc_dev_launch_var_select(const void *core, const void *aux, const void *emit, uint32_t n, const bsc_var_params *p, void *tile_cnt,
                                         void *tile_off, void *tile_mask, void *scan_tmp, size_t scan_tmp_bytes, void *totals, int num_cus,
                                         void *stream) {
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t n_tiles = (n + 63u) / 64u;
  hipLaunchKernelGGL(bsc_var_select_kernel, dim3(bsc_var_grid(n_tiles, num_cus)), dim3(256), 0, s, (const uint8_t *)core, (const uint8_t *)aux,
                     (const uint8_t *)emit, n, p->min_phred, (int)(p->pass_only != 0), (int)(p->known_only != 0), (uint32_t *)tile_cnt,
                     (unsigned long long *)tile_mask, (unsigned long long *)totals);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return bsc_dev_scan_u32(tile_cnt, tile_off, n_tiles, scan_tmp, scan_tmp_bytes, stream);
}

/* the pack pass behind it: out[min(count, out_cap)] records, *total = the count */
extern "C" int bsc_dev_launch_var_pack(const void *core, const void *aux, uint32_t n, const void *tile_off, const void *tile_mask, void *out,
                                       uint64_t out_cap, void *total, int num_cus, void *stream) {
  if (n == 0) return 0;
  const uint32_t n_tiles = (n + 63u) / 64u;
  hipLaunchKernelGGL(bsc_var_pack_kernel, dim3(bsc_var_grid(n_tiles, num_cus)), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)core,
                     (const uint8_t *)aux, n, (const uint32_t *)tile_off, (const unsigned long long *)tile_mask, (uint8_t *)out, out_cap,
                     (unsigned long long *)total);
  return (int)hipGetLastError();
}
