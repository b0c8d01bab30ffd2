/*
 * asmdev.hip — the allele-specific methylation table of a block (include/bscall_amd.h has the rule: SNP, ALLELE, WINDOW, RECORD, AQ, TOTALS, LINE
 * on top of COUNTS, SITE, BYTE and STATE of the read-level CpG table; csrc/asm.c the host form, which is the checker): for every heterozygous
 * SNP the caller wrote and every reference CpG within max_dist of it, how many templates carrying allele 1 / allele 2 read the CpG methylated
 * / unmethylated, and Fisher's two-sided p of that 2x2 table as a phred — from the dense per-position records, the prepared templates, their
 * read bytes and the site masks of cpgreadsdev.hip, while they are in HBM.
 *
 *   bsc_asm_snp_kernel     one wave per tile of 64 positions (the tile grid of the site masks): a lane reads its emit byte and the 16-byte head
 *                          of its bsc_vcf_core; the ballot -> snp_mask[k], snp_cnt[k]
 *   (exclusive scan of the counts: bsc_dev_scan_u32 -> snp_off[k] = the rank of the tile's first SNP)
 *   bsc_asm_span_kernel    one wave per tile, a lane per SNP j of it: snp_idx[j] = h - x, first[j] = RANK(max(x, h - W)), cnt[j] = RANK(min(y,
 *                          h + W) + 1) - first[j]; RANK(p) = the sites below p = tile_off + the bits of the tile's site mask below p.  The
 *                          sum of cnt as one 64-bit add a workgroup (the record count, which may not fit 32 bits: the host refuses then)
 *   (exclusive scan of cnt -> pair_off[j])
 *   bsc_asm_init_kernel    one wave per SNP, its rounds the tiles of the window, a lane per site: the record's head {snp_pos, cpg_pos, 0 .., gt |
 *                          OVERLAPPED << 8} at pair_off[j] + (the site's rank - first[j]) where that lies inside the room; the count, totals[0 .. 1]
 *   bsc_asm_walk_kernel    one wave per template.  Over the tiles of its span the bits of snp_mask inside the span: most templates see none and
 *                          leave after a few broadcast loads.  Per SNP found ALLELE is wave-uniform (one byte, gt from the dense record); then
 *                          cr_round over the tiles of (the template's sites) x (the window), the tile's mask cut to both and the overlapped
 *                          bits cleared; a lane that holds a state does one u32 atomic add into its record.  Integer adds alone: the bytes are
 *                          a function of the input.  Three totals stay in registers and leave the workgroup as three 64-bit adds.
 *   bsc_asm_finish_kernel  one lane per stored record: DEEP, Fisher's test by fisher_dev's statements with the clamp of the rule, aq; the tables
 *                          in LDS as bsc_fisher_kernel stages them
 *   bsc_asm_size_kernel /  the table's lines: the size pass, the scan and the write pass of cpgreadsdev.hip over these records, with a signed
 *   bsc_asm_write_kernel   decimal for dist.
 *
 * Longest line: the contig's name (<= 255 bytes) + 104: eight numbers of at most ten digits (end = cpg_pos + 1 <= 2^32), two letters, a sign and
 * ten digits, ten tabs and '\n'.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "callmath.h"
#include "devtables.h"
#include "recstream_dev.h"
#include "methtext_dev.h"
#include "cpgreads_dev.h"

static_assert(sizeof(bsc_asm_pair) == 32, "bsc_asm_pair is 32 bytes");
static_assert(sizeof(bsc_template) == 40, "bsc_template is 40 bytes");
static_assert(sizeof(bsc_vcf_core) == 64, "bsc_vcf_core is 64 bytes");

#define AS_WAVES 4u
#define AS_FLAG_OVERLAPPED 1u
#define AS_FLAG_DEEP 2u
#define AS_DEEP_ABOVE 46340u

typedef unsigned long long as_u64;

__device__ __forceinline__ as_u64 as_below(unsigned bit) { return (1ull << bit) - 1ull; } /* bit: 0 .. 63 */

extern "C" __global__ __launch_bounds__(256) void bsc_asm_snp_kernel(const uint8_t *__restrict__ core, const uint8_t *__restrict__ emit_b, uint32_t n,
                                                                     uint32_t n_tiles, uint32_t min_phred, int pass_only,
                                                                     uint32_t *__restrict__ snp_cnt, as_u64 *__restrict__ snp_mask) {
  const unsigned lane = threadIdx.x & 63u;
  for (uint32_t tile = blockIdx.x * AS_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * AS_WAVES) {
    const uint32_t i = tile * 64u + lane;
    bool snp = i < n && (!emit_b || emit_b[i] != 0);
    if (snp) {
      const uint4 c0 = *reinterpret_cast<const uint4 *>(core + (uint64_t)i * 64u); /* pos | emit, gt, ref_code, gt_enc | flt, phred, .. */
      const uint32_t gt = (c0.y >> 8) & 0xffu, flt = c0.z & 0xffu, phred = (c0.z >> 8) & 0xffu;
      snp = (c0.y & 0xffu) != 0 && gt <= 8u && ((0x16eu >> gt) & 1u) && phred >= min_phred && (!pass_only || flt == 0); /* 1, 2, 3, 5, 6, 8 */
    }
    const as_u64 m = __ballot(snp);
    if (lane == 0) {
      snp_cnt[tile] = (uint32_t)__popcll(m);
      snp_mask[tile] = m;
    }
  }
}

/* RANK of block index k (0 .. n): the sites at indices below k */
__device__ __forceinline__ uint32_t as_rank(uint64_t k, uint32_t n_tiles, const uint32_t *__restrict__ tile_off, const as_u64 *__restrict__ tile_mask) {
  const uint64_t t = k >> 6;
  if (t >= n_tiles) return tile_off[n_tiles - 1u] + (uint32_t)__popcll(tile_mask[n_tiles - 1u]); /* (k == n, n a multiple of 64) */
  return tile_off[t] + (uint32_t)__popcll(tile_mask[t] & as_below((unsigned)(k & 63u)));
}

extern "C" __global__ __launch_bounds__(256) void bsc_asm_span_kernel(uint32_t n, uint32_t n_tiles, uint32_t W, const uint32_t *__restrict__ snp_off,
                                                                      const as_u64 *__restrict__ snp_mask, const uint32_t *__restrict__ tile_off,
                                                                      const as_u64 *__restrict__ tile_mask, uint32_t *__restrict__ snp_idx,
                                                                      uint32_t *__restrict__ first, uint32_t *__restrict__ cnt,
                                                                      as_u64 *__restrict__ n_pairs) {
  __shared__ as_u64 s_sum;
  const unsigned lane = threadIdx.x & 63u;
  if (threadIdx.x == 0) s_sum = 0ull;
  __syncthreads();
  as_u64 acc = 0ull; /* this lane's share */
  for (uint32_t tile = blockIdx.x * AS_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * AS_WAVES) {
    const as_u64 m = snp_mask[tile];
    if (!((m >> lane) & 1ull)) continue;
    const uint32_t j = snp_off[tile] + (uint32_t)__popcll(m & as_below(lane));
    const uint64_t i = (uint64_t)tile * 64u + lane; /* h - x; < n */
    const uint64_t lo = i > W ? i - W : 0ull, hi = i + W < (uint64_t)n - 1u ? i + W : (uint64_t)n - 1u;
    const uint32_t f = as_rank(lo, n_tiles, tile_off, tile_mask), c = as_rank(hi + 1u, n_tiles, tile_off, tile_mask) - f;
    snp_idx[j] = (uint32_t)i;
    first[j] = f;
    cnt[j] = c;
    acc += c;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d);
  if (lane == 0 && acc) atomicAdd(&s_sum, acc);
  __syncthreads();
  if (threadIdx.x == 0 && s_sum) atomicAdd(n_pairs, s_sum);
}

/* the window of SNP index i cut to tile t: the bits of m at block indices lo .. hi */
__device__ __forceinline__ as_u64 as_cut(as_u64 m, uint64_t t, uint64_t lo, uint64_t hi) {
  if (t == (lo >> 6)) m &= ~as_below((unsigned)(lo & 63u));
  if (t == (hi >> 6) && (hi & 63u) != 63u) m &= as_below((unsigned)(hi & 63u) + 1u);
  return m;
}

extern "C" __global__ __launch_bounds__(256) void bsc_asm_init_kernel(const uint8_t *__restrict__ core, uint32_t x, uint32_t n, uint32_t W, uint32_t n_snps,
                                                                      as_u64 n_pairs, const uint32_t *__restrict__ snp_idx,
                                                                      const uint32_t *__restrict__ first, const uint32_t *__restrict__ pair_off,
                                                                      const uint32_t *__restrict__ tile_off, const as_u64 *__restrict__ tile_mask,
                                                                      bsc_asm_pair *__restrict__ pairs, uint64_t cap, as_u64 *__restrict__ d_n_pairs,
                                                                      as_u64 *__restrict__ totals) {
  const unsigned lane = threadIdx.x & 63u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *d_n_pairs = n_pairs;
    totals[0] = n_snps;
    totals[1] = n_pairs;
  }
  for (uint32_t j = blockIdx.x * AS_WAVES + (threadIdx.x >> 6); j < n_snps; j += gridDim.x * AS_WAVES) {
    const uint64_t i = snp_idx[j];
    const uint64_t base = (uint64_t)pair_off[j];
    if (base >= cap) continue; /* counted, not stored (wave-uniform) */
    const uint32_t f = first[j];
    const uint32_t gt = core[i * 64u + 5u];
    const uint64_t lo = i > W ? i - W : 0ull, hi = i + W < (uint64_t)n - 1u ? i + W : (uint64_t)n - 1u;
    for (uint64_t t = lo >> 6; t <= (hi >> 6); t++) {
      const as_u64 full = tile_mask[t], m = as_cut(full, t, lo, hi);
      if (!((m >> lane) & 1ull)) continue;
      const uint64_t s = t * 64u + lane; /* the site's index */
      const uint64_t idx = base + (tile_off[t] + (uint32_t)__popcll(full & as_below(lane)) - f);
      if (idx >= cap) continue;
      const uint32_t ovl = (i == s || i == s + 1u) ? AS_FLAG_OVERLAPPED : 0u;
      uint2 *w = reinterpret_cast<uint2 *>(pairs + idx);
      w[0] = make_uint2(x + (uint32_t)i, x + (uint32_t)s);
      w[1] = make_uint2(0u, 0u);
      w[2] = make_uint2(0u, 0u);
      w[3] = make_uint2(0u, gt | ovl << 8);
    }
  }
}

/* ALLELE from the template's strand, the genotype and the base of BYTE(t, h): 0 none, 1, 2 */
__device__ __forceinline__ unsigned as_allele(unsigned bs, unsigned gt, unsigned base) {
  if ((bs == 1u && gt == 6u) || (bs == 2u && gt == 2u)) return 0u;
  const unsigned a1 = (0xE9500u >> (2u * gt)) & 3u, a2 = (0xFB9E4u >> (2u * gt)) & 3u; /* the genotype's two letters, two bits each */
  const unsigned also = bs == 1u ? (base == 3u ? 1u : 4u) : (base == 0u ? 2u : 4u);    /* a read T may be a C, a read A a G; 4: nothing more */
  const bool in1 = a1 == base || a1 == also, in2 = a2 == base || a2 == also;
  return in1 == in2 ? 0u : (in1 ? 1u : 2u);
}

extern "C" __global__ __launch_bounds__(256) void bsc_asm_walk_kernel(const bsc_template *__restrict__ tpl, uint32_t nr, const uint8_t *__restrict__ seq,
                                                                      uint64_t seq_bytes, uint32_t x, uint32_t y, unsigned min_qual, uint32_t W,
                                                                      const uint8_t *__restrict__ core, const uint32_t *__restrict__ snp_off,
                                                                      const as_u64 *__restrict__ snp_mask, const uint32_t *__restrict__ first,
                                                                      const uint32_t *__restrict__ pair_off, const uint32_t *__restrict__ tile_off,
                                                                      const as_u64 *__restrict__ tile_mask, bsc_asm_pair *__restrict__ pairs, uint64_t cap,
                                                                      as_u64 *__restrict__ totals) {
  __shared__ as_u64 s_tot[AS_WAVES][3];
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint64_t n = (uint64_t)y - x + 1u;
  as_u64 t_obs = 0, t_a1 = 0, t_adds = 0; /* wave-uniform */
  for (uint32_t it = blockIdx.x * AS_WAVES + wid; it < nr; it += gridDim.x * AS_WAVES) {
    const bsc_template *tp = tpl + it; /* one address a wave: the loads are broadcast */
    cr_tpl t;
    t.bs = tp->bs_strand;
    if (t.bs != 1u && t.bs != 2u) continue; /* wave-uniform */
    uint64_t lo = ~0ull, hi = 0ull;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint64_t len = tp->len[k], off = tp->off[k];
      const bool have = len != 0u && off <= seq_bytes && len <= seq_bytes - off;
      t.pos[k] = tp->pos[k];
      t.end[k] = have ? t.pos[k] + len : t.pos[k];
      t.off[k] = off;
      if (have) {
        lo = t.pos[k] < lo ? t.pos[k] : lo;
        hi = t.end[k] > hi ? t.end[k] : hi;
      }
    }
    if (hi == 0ull) continue;
    /* the SNPs that can have a byte: block indices [ha, hb] */
    if (hi <= x || lo > y) continue;
    const uint64_t ha = lo > x ? lo - x : 0ull, hb = (hi - 1u < y ? hi - 1u : (uint64_t)y) - x;
    /* the sites that can have a state (cpgreadsdev.hip): indices [sa, sb] */
    const uint64_t sh = t.bs == 2u ? 1u : 0u;
    uint64_t a = lo >= sh ? lo - sh : 0ull, b = hi - sh; /* [a, b) */
    if (a < x) a = x;
    if (b > (uint64_t)y + 1u) b = (uint64_t)y + 1u;
    const bool sites = a < b;
    const uint64_t sa = a - x, sb = sites ? b - 1u - x : 0ull;
    for (uint64_t ht = ha >> 6; ht <= (hb >> 6); ht++) {
      const as_u64 sfull = snp_mask[ht];
      as_u64 sm = as_cut(sfull, ht, ha, hb);
      while (sm) { /* wave-uniform */
        const unsigned bit = (unsigned)__builtin_ctzll(sm);
        sm &= sm - 1ull;
        const uint64_t i = ht * 64u + bit; /* h - x */
        const int byte = cr_byte(t, seq, (uint64_t)x + i, min_qual);
        if (byte < 0) continue;
        const unsigned gt = core[i * 64u + 5u];
        const unsigned al = as_allele(t.bs, gt, (unsigned)byte & 3u);
        if (!al) continue;
        t_obs++;
        t_a1 += al == 1u;
        if (!sites) continue;
        const uint64_t wl = i > W ? i - W : 0ull, wh = i + W < n - 1u ? i + W : n - 1u;
        const uint64_t ra = sa > wl ? sa : wl, rb = sb < wh ? sb : wh;
        if (ra > rb) continue;
        const uint32_t j = snp_off[ht] + (uint32_t)__popcll(sfull & as_below(bit));
        const uint64_t base = (uint64_t)pair_off[j];
        const uint32_t f = first[j];
        for (uint64_t tt = ra >> 6; tt <= (rb >> 6); tt++) {
          const as_u64 full = tile_mask[tt];
          as_u64 m = as_cut(full, tt, ra, rb);
          /* OVERLAPPED: the sites at h and at h - 1 */
          if (tt == (i >> 6)) m &= ~(1ull << (i & 63u));
          if (i && tt == ((i - 1u) >> 6)) m &= ~(1ull << ((i - 1u) & 63u));
          if (!m) continue;
          as_u64 mm, mu;
          cr_round(t, seq, x, y, (uint32_t)tt, m, lane, min_qual, mm, mu);
          t_adds += (unsigned)__popcll(mm | mu);
          const unsigned st = cr_state_at(mm, mu, lane);
          if (st) {
            const uint64_t idx = base + (tile_off[tt] + (uint32_t)__popcll(full & as_below(lane)) - f);
            if (idx < cap) atomicAdd(reinterpret_cast<uint32_t *>(pairs + idx) + 2u + 2u * (al - 1u) + (st - 1u), 1u);
          }
        }
      }
    }
  }
  if (lane == 0) {
    s_tot[wid][0] = t_obs;
    s_tot[wid][1] = t_a1;
    s_tot[wid][2] = t_adds;
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    as_u64 v = 0ull;
    for (unsigned w = 0; w < AS_WAVES; w++) v += s_tot[w][threadIdx.x];
    if (v) atomicAdd(totals + 2u + threadIdx.x, v);
  }
}

/* ---- AQ -------------------------------------------------------------------------------------------------------------------------------------- */
/* a point term of Fisher's test with the rule's clamp */
__device__ __forceinline__ double as_point(double arg, const uint64_t *exptab) { return arg < -700.0 ? 0.0 : bsm_exp_t(arg, exptab); }

/* fisher_dev (callmath.h) statement for statement, its point terms through as_point */
__device__ static double as_fisher(int c0, int c1, int c2, int c3, const double *lf, const double *logtab, const uint64_t *exptab) {
#define LF(v) lfact_dev((v), lf, logtab)
  const int row0 = c0 + c1, row1 = c2 + c3, col0 = c0 + c2, col1 = c1 + c3;
  const int n = row0 + row1;
  if (n == 0) return 1.0;
  const double delta = (double)c0 - (double)(row0 * col0) / (double)n;
  const double knst = LF(col0) + LF(col1) + LF(row0) + LF(row1) - LF(n);
  double l = as_point(knst - LF(c0) - LF(c1) - LF(c2) - LF(c3), exptab);
  double p = l;
  if (delta > 0.0) {
    int mn = c1 < c2 ? c1 : c2;
    for (int i = 0; i < mn; i++) {
      l *= (double)((c1 - i) * (c2 - i)) / (double)((c0 + i + 1) * (c3 + i + 1));
      p += l;
    }
    mn = c0 < c3 ? c0 : c3;
    const int k = (int)ceil(2.0 * delta);
    if (k <= mn) {
      c0 -= k; c3 -= k; c1 += k; c2 += k;
      l = as_point(knst - LF(c0) - LF(c1) - LF(c2) - LF(c3), exptab);
      p += l;
      for (int i = 0; i < mn - k; i++) {
        l *= (double)((c0 - i) * (c3 - i)) / (double)((c1 + i + 1) * (c2 + i + 1));
        p += l;
      }
    }
  } else {
    int mn = c0 < c3 ? c0 : c3;
    for (int i = 0; i < mn; i++) {
      l *= (double)((c0 - i) * (c3 - i)) / (double)((c1 + i + 1) * (c2 + i + 1));
      p += l;
    }
    mn = c1 < c2 ? c1 : c2;
    int k = (int)ceil(-2.0 * delta);
    if (!k) k = 1;
    if (k <= mn) {
      c0 += k; c3 += k; c1 -= k; c2 -= k;
      l = as_point(knst - LF(c0) - LF(c1) - LF(c2) - LF(c3), exptab);
      p += l;
      for (int i = 0; i < mn - k; i++) {
        l *= (double)((c1 - i) * (c2 - i)) / (double)((c0 + i + 1) * (c3 + i + 1));
        p += l;
      }
    }
  }
  return p;
#undef LF
}

extern "C" __global__ __launch_bounds__(256) void bsc_asm_finish_kernel(bsc_asm_pair *__restrict__ pairs, uint64_t n_stored,
                                                                        const bsc_dev_tables *__restrict__ tb, as_u64 *__restrict__ totals) {
  __shared__ double s_lf[256];
  __shared__ double s_logtab[256];
  __shared__ as_u64 s_exptab[256];
  __shared__ as_u64 s_deep;
  const unsigned tid = threadIdx.x;
  s_lf[tid] = tb->lfact[tid];
  s_logtab[tid] = tb->log_tab[tid];
  s_exptab[tid] = tb->exp_tab[tid];
  if (tid == 0) s_deep = 0ull;
  __syncthreads();
  unsigned deep = 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + tid; i < n_stored; i += (uint64_t)gridDim.x * 256u) {
    uint2 *w = reinterpret_cast<uint2 *>(pairs + i);
    const uint2 c01 = w[1], c23 = w[2];
    uint2 tail = w[3];
    if ((tail.y >> 8) & AS_FLAG_OVERLAPPED) continue; /* (aq is 0 since the head was written) */
    const uint64_t sum = (uint64_t)c01.x + c01.y + c23.x + c23.y;
    uint32_t aq = 0u;
    if (sum > AS_DEEP_ABOVE) {
      tail.y |= AS_FLAG_DEEP << 8;
      deep++;
    } else {
      const double z = as_fisher((int)c01.x, (int)c01.y, (int)c23.x, (int)c23.y, s_lf, s_logtab, (const uint64_t *)s_exptab);
      aq = z >= 1.0e-100 ? (uint32_t)(int)(-(bsm_log_t(z, s_logtab) / BSM_LN10) * 10.0 + 0.5) : 1000u;
    }
    tail.x = aq;
    w[3] = tail;
  }
  if (deep) atomicAdd(&s_deep, (as_u64)deep);
  __syncthreads();
  if (tid == 0 && s_deep) atomicAdd(totals + 5u, s_deep);
}

/* ---- the table's lines ----------------------------------------------------------------------------------------------------------------------- */
#define AS_CONTIG_MAX 255u
#define AS_LINE_MAX (AS_CONTIG_MAX + 104u)
#define AS_IMG 4096u
#define AS_PARTS 8u
static_assert(AS_IMG >= (RS_LANES / AS_PARTS) * AS_LINE_MAX && AS_IMG % 16u == 0u, "an eighth of a tile of the longest lines must fit the wave's image");
static_assert(AS_LINE_MAX <= 0xffffu, "a line's length is kept in 16 bits");

struct as_text_args {
  const bsc_asm_pair *pairs;
  const as_u64 *n_pairs;
  uint64_t max_pairs;
  uint32_t min_cov;      /* max(1, min_cov) */
  uint32_t clen1;        /* the contig's name and the tab behind it, bytes */
  uint32_t contig_w[64]; /* those bytes, zero padded */
};

struct as_rec {
  uint32_t w[8];
};

__device__ __forceinline__ uint64_t as_clamp_n(const as_text_args &a) {
  const as_u64 n = *a.n_pairs;
  return n < a.max_pairs ? n : a.max_pairs;
}

__device__ __forceinline__ void as_load(as_rec &r, const as_text_args &a, uint64_t i) {
  const uint2 *p = reinterpret_cast<const uint2 *>(a.pairs + i); /* 32-byte records, 8-byte aligned */
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint2 v = p[k];
    r.w[2 * k] = v.x;
    r.w[2 * k + 1] = v.y;
  }
}

__device__ __forceinline__ bool as_line_written(const as_rec &r, uint32_t min_cov) {
  return (r.w[7] >> 8) == 0u && (uint64_t)r.w[2] + r.w[3] >= min_cov && (uint64_t)r.w[4] + r.w[5] >= min_cov;
}

template <class S>
__device__ __forceinline__ void as_emit_line(S &s, const as_rec &r, const uint32_t *contig_w, unsigned clen1) {
  s.words(contig_w, clen1);
  mb_put_dec(s, (uint64_t)(r.w[1] - 1u), '\t');
  mb_put_dec(s, (uint64_t)r.w[1] + 1ull, '\t');
  mb_put_dec(s, r.w[0], '\t');
  const unsigned gt = r.w[7] & 0xffu; /* AA AC AG AT CC CG CT GG GT TT, two bits a letter; anything else NN */
  const unsigned a1 = (0xE9500u >> (2u * gt)) & 3u, a2 = (0xFB9E4u >> (2u * gt)) & 3u;
  const uint32_t acgt = (uint32_t)'A' | (uint32_t)'C' << 8 | (uint32_t)'G' << 16 | (uint32_t)'T' << 24;
  const unsigned l1 = gt <= 9u ? (acgt >> (8u * a1)) & 0xffu : 'N', l2 = gt <= 9u ? (acgt >> (8u * a2)) & 0xffu : 'N';
  s.bytes((uint64_t)l1 | (uint64_t)l2 << 8 | (uint64_t)'\t' << 16, 3u);
  mb_put_dec(s, r.w[2], '\t');
  mb_put_dec(s, r.w[3], '\t');
  mb_put_dec(s, r.w[4], '\t');
  mb_put_dec(s, r.w[5], '\t');
  mb_put_dec(s, r.w[6], '\t');
  const int64_t dist = (int64_t)r.w[1] - (int64_t)r.w[0];
  if (dist < 0) s.u8('-');
  mb_put_dec(s, (uint64_t)(dist < 0 ? -dist : dist), '\n');
}

/* tile_bytes[n_tiles] = 0 (so that the scan's last output is the stream's length); *lines += the lines */
extern "C" __global__ __launch_bounds__(256) void bsc_asm_size_kernel(as_text_args a, uint32_t n_tiles, as_u64 *__restrict__ tile_bytes,
                                                                      uint16_t *__restrict__ line_len, as_u64 *__restrict__ lines) {
  __shared__ as_u64 s_lines;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n = as_clamp_n(a);
  if (threadIdx.x == 0) s_lines = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  __syncthreads();
  as_u64 n_lines = 0ull; /* wave-uniform */
  for (uint32_t tile = blockIdx.x * AS_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * AS_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    if (i < n) {
      as_rec r;
      as_load(r, a, i);
      if (as_line_written(r, a.min_cov)) {
        mb_count_sink c = {0u};
        as_emit_line(c, r, a.contig_w, a.clen1);
        len = c.len;
      }
    }
    if (i < a.max_pairs) line_len[i] = (uint16_t)len;
    n_lines += (unsigned)__popcll(__ballot(len != 0u));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
  if (lane == 0 && n_lines) atomicAdd(&s_lines, n_lines);
  __syncthreads();
  if (threadIdx.x == 0 && s_lines) atomicAdd(lines, s_lines);
}

extern "C" __global__ __launch_bounds__(256) void bsc_asm_write_kernel(as_text_args a, uint32_t n_tiles, const as_u64 *__restrict__ tile_off,
                                                                       const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out, uint64_t out_cap,
                                                                       as_u64 *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[AS_WAVES][AS_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = as_clamp_n(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = tile_off[n_tiles];
  for (uint32_t tile = blockIdx.x * AS_WAVES + wid; tile < n_tiles; tile += gridDim.x * AS_WAVES) {
    if ((uint64_t)tile * 64u >= n) break; /* wave-uniform; later tiles of this wave lie further out still */
    const uint64_t g_tile = tile_off[tile], g_end = tile_off[tile + 1u];
    if (g_end == g_tile) continue; /* no line in this tile */
    if (g_end > out_cap) continue; /* the host reports the overflow from *total */
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const unsigned len = i < n ? line_len[i] : 0u;
    as_rec r;
    if (len) as_load(r, a, i);
    unsigned excl, t_all;
    const unsigned inc = rs_wave_excl_scan(len, excl, t_all);
    const unsigned parts = rs_pick_parts<AS_IMG, AS_PARTS>(inc);
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = rs_lane(inc, step * (ps + 1u) - 1u); /* one past its last */
      const bool mine = len && excl >= b0 && excl < b1;
      const uint64_t g0 = g_tile + b0;
      const unsigned ph = (unsigned)(g0 & 15u);
      if (mine) {
        mb_write_sink w = {img + ph + (excl - b0), 0u};
        as_emit_line(w, r, a.contig_w, a.clen1);
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

static unsigned bsc_asm_grid(uint64_t n_items, int num_cus) {
  uint64_t grid = (n_items + AS_WAVES - 1u) / AS_WAVES;
  /* eight workgroups of four waves a CU fill its SIMDs */
  if (grid > (uint64_t)num_cus * 8u) grid = (uint64_t)num_cus * 8u;
  return grid ? (unsigned)grid : 1u;
}

/* the SNP pass and the scan: snp_cnt / snp_off (n + 63) / 64 words, snp_mask as many u64; core: n records, emit: n bytes or NULL */
extern "C" int bsc_dev_launch_asm_snps(const void *core, const void *emit, uint32_t n, uint32_t min_phred, int pass_only, void *snp_cnt, void *snp_off,
                                       void *snp_mask, void *scan_tmp, size_t scan_tmp_bytes, int num_cus, void *stream) {
  const uint32_t n_tiles = (uint32_t)(((uint64_t)n + 63u) / 64u);
  hipLaunchKernelGGL(bsc_asm_snp_kernel, dim3(bsc_asm_grid(n_tiles, num_cus)), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)core,
                     (const uint8_t *)emit, n, n_tiles, min_phred, pass_only, (uint32_t *)snp_cnt, (as_u64 *)snp_mask);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return bsc_dev_scan_u32(snp_cnt, snp_off, n_tiles, scan_tmp, scan_tmp_bytes, stream);
}

/* the windows: snp_idx / first / cnt / pair_off n_snps (> 0) words each, *n_pairs (a device u64, zeroed here) = the sum of cnt */
extern "C" int bsc_dev_launch_asm_spans(uint32_t n, uint32_t W, uint32_t n_snps, const void *snp_off, const void *snp_mask, const void *tile_off,
                                        const void *tile_mask, void *snp_idx, void *first, void *cnt, void *pair_off, void *n_pairs, void *scan_tmp,
                                        size_t scan_tmp_bytes, int num_cus, void *stream) {
  const uint32_t n_tiles = (uint32_t)(((uint64_t)n + 63u) / 64u);
  hipError_t e = hipMemsetAsync(n_pairs, 0, sizeof(as_u64), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(bsc_asm_span_kernel, dim3(bsc_asm_grid(n_tiles, num_cus)), dim3(256), 0, (hipStream_t)stream, n, n_tiles, W, (const uint32_t *)snp_off,
                     (const as_u64 *)snp_mask, (const uint32_t *)tile_off, (const as_u64 *)tile_mask, (uint32_t *)snp_idx, (uint32_t *)first, (uint32_t *)cnt,
                     (as_u64 *)n_pairs);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return bsc_dev_scan_u32(cnt, pair_off, n_snps, scan_tmp, scan_tmp_bytes, stream);
}

/* the records: heads, walk, finish.  totals: eight device u64 the caller zeroed; n_pairs <= 2^32 - 1 */
extern "C" int bsc_dev_launch_asm_pairs(const void *tpl, uint32_t nr, const void *seq, uint64_t seq_bytes, uint32_t x, uint32_t y, uint32_t min_qual,
                                        uint32_t W, const void *core, uint32_t n_snps, uint64_t n_pairs, const void *snp_off, const void *snp_mask,
                                        const void *snp_idx, const void *first, const void *pair_off, const void *tile_off, const void *tile_mask,
                                        const void *tables, void *pairs, uint64_t cap, void *d_n_pairs, void *totals, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const uint32_t n = y - x + 1u;
  hipLaunchKernelGGL(bsc_asm_init_kernel, dim3(bsc_asm_grid(n_snps, num_cus)), dim3(256), 0, s, (const uint8_t *)core, x, n, W, n_snps, (as_u64)n_pairs,
                     (const uint32_t *)snp_idx, (const uint32_t *)first, (const uint32_t *)pair_off, (const uint32_t *)tile_off, (const as_u64 *)tile_mask,
                     (bsc_asm_pair *)pairs, cap, (as_u64 *)d_n_pairs, (as_u64 *)totals);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if (!n_snps) return 0;
  if (nr) { /* (also where no window holds a site: the observations are counted all the same) */
    hipLaunchKernelGGL(bsc_asm_walk_kernel, dim3(bsc_asm_grid(nr, num_cus)), dim3(256), 0, s, (const bsc_template *)tpl, nr, (const uint8_t *)seq, seq_bytes,
                       x, y, min_qual, W, (const uint8_t *)core, (const uint32_t *)snp_off, (const as_u64 *)snp_mask, (const uint32_t *)first,
                       (const uint32_t *)pair_off, (const uint32_t *)tile_off, (const as_u64 *)tile_mask, (bsc_asm_pair *)pairs, cap, (as_u64 *)totals);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const uint64_t n_stored = n_pairs < cap ? n_pairs : cap;
  if (!n_stored) return 0;
  uint64_t grid = (n_stored + 255u) / 256u;
  if (grid > (uint64_t)num_cus * 8u) grid = (uint64_t)num_cus * 8u;
  hipLaunchKernelGGL(bsc_asm_finish_kernel, dim3((unsigned)grid), dim3(256), 0, s, (bsc_asm_pair *)pairs, n_stored, (const bsc_dev_tables *)tables,
                     (as_u64 *)totals);
  return (int)hipGetLastError();
}

/*
 * pairs[min(*n_pairs, max_pairs)] -> out[<= out_cap] lines; totals2[0] = the stream's length (also when it exceeds out_cap: then only the tiles
 * that fit whole are written), totals2[1] += lines (the caller zeroes it).  contig: the name, contig_len (1 .. 255) bytes, checked by the
 * caller.  tile_bytes / tile_off: max_pairs / 64 (rounded up) + 1 u64 each; line_len: max_pairs u16; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of the
 * tiles + 1.
 */
extern "C" int bsc_dev_launch_asm_text(const void *pairs, const void *n_pairs, uint64_t max_pairs, const char *contig, uint32_t contig_len, uint32_t min_cov,
                                       void *tile_bytes, void *tile_off, void *line_len, void *scan_tmp, size_t scan_tmp_bytes, void *out, uint64_t out_cap,
                                       void *totals2, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!contig_len || contig_len > AS_CONTIG_MAX) return (int)hipErrorInvalidValue;
  as_text_args a;
  a.pairs = (const bsc_asm_pair *)pairs;
  a.n_pairs = (const as_u64 *)n_pairs;
  a.max_pairs = max_pairs;
  a.min_cov = min_cov > 1u ? min_cov : 1u;
  a.clen1 = contig_len + 1u;
  for (int k = 0; k < 64; k++) a.contig_w[k] = 0u;
  __builtin_memcpy(a.contig_w, contig, contig_len);
  ((char *)a.contig_w)[contig_len] = '\t';
  const uint64_t nt64 = (max_pairs + 63u) / 64u;
  if (nt64 > 0x7fffffffull) return (int)hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)nt64;
  const unsigned grid = bsc_asm_grid(n_tiles, num_cus);
  hipLaunchKernelGGL(bsc_asm_size_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (as_u64 *)tile_bytes, (uint16_t *)line_len, (as_u64 *)totals2 + 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int rc = bsc_dev_scan_u64(tile_bytes, tile_off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_asm_write_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (const as_u64 *)tile_off, (const uint16_t *)line_len, (uint8_t *)out,
                     out_cap, (as_u64 *)totals2);
  return (int)hipGetLastError();
}
