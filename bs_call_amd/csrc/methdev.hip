/*
 * methdev.hip — a block's cytosines as a bedMethyl table on the device: for every record that gives a line (include/bscall_amd.h has
 * the rule and the columns; the reference's src/print_vcf.c:442-515 the sites and the counts), in position order, the line
 * bsc_meth_format_rec writes for it.  The host form csrc/methbed.c is the checker.  The placement — wave prefix sum, the parts, the
 * image's copy-out — is recstream_dev.h's, shared with the BCF encoder (bcfdev.hip) and the VCF text encoder (vcftextdev.hip):
 *
 *   bsc_meth_size_kernel   one wave per tile of 64 records / positions: every lane the length of its line (the emitter over the
 *                          counting sink) -> line_len[i] (u16; 0 = no line), the tile's sum -> tile_bytes[tile]; lines, sum of a, sum
 *                          of b -> totals[1 .. 3]
 *   (exclusive scan of the tile sums, rocPRIM u64: sort.hip; one more entry behind the last tile = the stream's length)
 *   bsc_meth_write_kernel  one wave per tile that has bytes: lane offsets from a wave prefix sum of line_len, every lane writes its
 *                          line into the wave's LDS image of the tile's span of the stream, then the wave copies the image out.  A
 *                          tile whose span does not fit the image (4 KB) goes out in 2, 4 or 8 parts.
 *
 * Whether a record gives a line is decided from its first 16 bytes (emit, gt, flt, phred, cg) and, behind them, its counts: a
 * position that gives none costs those 16 bytes (their 64-byte sector) — or, with the chain's byte per position (emit: not 0 <=> the
 * record is written), a position without a record costs that byte.  Half of a record is never read: GL, FS, QD, DP, MQ, AMQ.
 *
 * All arithmetic is integer: the decimal conversion divides by constants, the percentage is found by bisection over 0 .. 100 (a
 * 64-bit division by a variable would be expanded through a floating-point reciprocal).
 *
 * Longest line: the contig's name (<= 255 bytes) + 111 = 366 bytes:
 *   "\t" start 10 "\t" end 10 "\t" name 3 "\t" score 4 "\t" strand 1 "\t" start 10 "\t" end 10 "\t"                          = 56
 *   rgb 9 "\t" coverage 10 "\t" pct 2 "\t" a 10 "\t" b 10 "\t" GQ 3 "\t" filter 4 "\n"   (pct 100: rgb 7, b 8 digits)        = 55
 * a line's length fits 16 bits, eight lines always fit the image.
 *
 * The combined-strand CpG table (one line per CpG dinucleotide; the rule is the header's, the checker csrc/methcpg.c) is the same two
 * passes over the same placement, bsc_meth_cpg_size_kernel / bsc_meth_cpg_write_kernel, and the one encoder whose line depends on a
 * record's neighbours: a plus half needs the half-ness, counts, phred and flt of record i + 1, a minus half the half-ness of record
 * i - 1.  The size pass decides: every lane evaluates its own record (16 bytes; a candidate's counts behind them), the neighbours'
 * verdicts move one lane up and down the wave, and only lane 63 (a plus half) and lane 0 (a minus half) read the next / previous
 * tile's edge record from memory — bytes that tile's own lane fetches too.  It leaves bit 15 of line_len[i] set for a pair's line, so
 * that the write pass evaluates no rule again: a lane with a line, or behind a lane with a pair's line, loads its record; the partner's
 * counts move one lane down, and lane 63 of a pair reads record i + 1 itself (its tile may have no bytes and no wave).  Same longest
 * line: the name is a byte shorter ("CG"), A + B (2^34 - 4 at most) a digit longer.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "recstream_dev.h"
#include "methtext_dev.h" /* the sinks, the decimal and pct forms, columns 4 .. 15: shared with bigbeddev.hip */

static_assert(sizeof(bsc_vcf_rec) == 128 && sizeof(bsc_vcf_core) == 64, "bsc_vcf_rec is 128 bytes, its core the first 64");

#define MB_WAVES 4u
#define MB_CONTIG_MAX 255u
#define MB_LINE_MAX (MB_CONTIG_MAX + 111u)
#define MB_IMG 4096u /* the wave's image: a tile of 64 ordinary lines (~60 bytes each) in one part */
#define MB_PARTS 8u
static_assert(MB_IMG >= (RS_LANES / MB_PARTS) * MB_LINE_MAX && MB_IMG % 16u == 0u, "an eighth of a tile of the longest lines must fit the wave's image");
static_assert(MB_LINE_MAX <= 0xffffu, "a line's length is kept in 16 bits");

struct mb_args {
  rs_src src;
  const uint8_t *emit; /* the chain's byte per position (not 0 <=> a record is written), or NULL */
  int32_t all_contexts;
  uint32_t min_cov, min_phred;
  int32_t pass_only;
  uint32_t clen1;        /* the contig's name and the tab behind it, bytes */
  uint32_t contig_w[64]; /* those bytes, zero padded */
};

/* record / position i: does it give a line, and of what.  known: the caller knows it does (the size pass said so) — the loads leave
 * together; otherwise the record's first 16 bytes decide whether the others are fetched. */
__device__ __forceinline__ bool mb_site_of(mb_site &s, const mb_args &a, uint64_t i, bool known) {
  const uint4 *lo = reinterpret_cast<const uint4 *>(a.src.recs ? a.src.recs + i * 128u : a.src.core + i * 64u);
  const uint4 *hi = a.src.recs ? lo + 4 : reinterpret_cast<const uint4 *>(a.src.aux + i * 64u);
  const uint4 v0 = lo[0];
  const unsigned emit = v0.y & 0xffu, gt = (v0.y >> 8) & 0xffu, flt = v0.z & 0xffu, phred = (v0.z >> 8) & 0xffu, cg = v0.z >> 24;
  if (!known) {
    if (!emit || (gt != 4u && gt != 7u)) return false;
    if (cg != 'C' && !(a.all_contexts && cg == 'H')) return false;
    if (phred < a.min_phred || (a.pass_only && flt)) return false;
  }
  const uint4 v1 = lo[1], c1 = hi[1]; /* bytes 16 .. 31 (cx_gt: 19 .. 23), counts[4 .. 7] */
  s.minus = gt == 7u;
  s.a = s.minus ? c1.z : c1.y; /* counts[6] : counts[5] */
  s.b = s.minus ? c1.x : c1.w; /* counts[4] : counts[7] */
  const uint64_t cov = (uint64_t)s.a + s.b;
  if (!known && cov < (uint64_t)(a.min_cov > 1u ? a.min_cov : 1u)) return false;
  s.pos = v0.x;
  s.flt = flt;
  s.phred = phred;
  s.label = 0u;
  if (cg != 'C') {
    const unsigned n2 = s.minus ? v1.x >> 24 : v1.y >> 24; /* cx_gt[0] = byte 19, cx_gt[4] = byte 23 */
    if (n2 == (s.minus ? 'C' : 'G')) s.label = 1u;
    else s.label = (n2 == 'A' || n2 == 'C' || n2 == 'G' || n2 == 'T') ? 2u : 3u;
  }
  return true;
}

template <class S>
__device__ __forceinline__ void mb_emit_line(S &s, const mb_site &m, const uint32_t *contig_w, unsigned clen1) {
  const uint64_t cov = (uint64_t)m.a + m.b;
  const unsigned pct = mb_pct(m.a, cov);
  const uint32_t start = m.pos - 1u;
  s.words(contig_w, clen1);
  mb_put_dec(s, start, '\t');
  mb_put_dec(s, m.pos, '\t');
  mb_emit_cols<'\n'>(s, m, start, cov, pct);
}

/* n_tiles = tiles of max_recs; tile_bytes[n_tiles] = 0 (so that the scan's last output is the stream's length); sums[0] += lines,
 * sums[1] += their a, sums[2] += their b */
extern "C" __global__ __launch_bounds__(256) void bsc_meth_size_kernel(mb_args a, uint32_t n_tiles, unsigned long long *__restrict__ tile_bytes,
                                                                       uint16_t *__restrict__ line_len, unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long s_sum[3];
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n = rs_clamp_n(a.src);
  if (threadIdx.x < 3u) s_sum[threadIdx.x] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  __syncthreads();
  unsigned long long n_lines = 0ull, sum_a = 0ull, sum_b = 0ull; /* this lane's */
  for (uint32_t tile = blockIdx.x * MB_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * MB_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    mb_site m;
    if (i < n && (!a.emit || a.emit[i]) && mb_site_of(m, a, i, false)) {
      mb_count_sink c = {0u};
      mb_emit_line(c, m, a.contig_w, a.clen1);
      len = c.len;
      n_lines++;
      sum_a += m.a;
      sum_b += m.b;
    }
    if (i < a.src.max_recs) line_len[i] = (uint16_t)len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
  /* once per wave into the workgroup's words, once per workgroup into the totals (atomics on one word are served one after the other) */
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    n_lines += __shfl_xor(n_lines, d);
    sum_a += __shfl_xor(sum_a, d);
    sum_b += __shfl_xor(sum_b, d);
  }
  if (lane == 0 && n_lines) {
    atomicAdd(&s_sum[0], n_lines);
    atomicAdd(&s_sum[1], sum_a);
    atomicAdd(&s_sum[2], sum_b);
  }
  __syncthreads();
  if (threadIdx.x < 3u && s_sum[threadIdx.x]) atomicAdd(sums + threadIdx.x, s_sum[threadIdx.x]);
}

extern "C" __global__ __launch_bounds__(256) void bsc_meth_write_kernel(mb_args a, uint32_t n_tiles, const unsigned long long *__restrict__ tile_off,
                                                                        const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out, uint64_t out_cap,
                                                                        unsigned long long *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[MB_WAVES][MB_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = rs_clamp_n(a.src);
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = tile_off[n_tiles];
  for (uint32_t tile = blockIdx.x * MB_WAVES + wid; tile < n_tiles; tile += gridDim.x * MB_WAVES) {
    if ((uint64_t)tile * 64u >= n) break; /* wave-uniform; later tiles of this wave lie further out still */
    const uint64_t g_tile = tile_off[tile], g_end = tile_off[tile + 1u];
    if (g_end == g_tile) continue;  /* no line in this tile: nothing of it is read */
    if (g_end > out_cap) continue;  /* the host reports the overflow from *total */
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const unsigned len = i < n ? line_len[i] : 0u;
    mb_site m;
    if (len) (void)mb_site_of(m, a, i, true);
    unsigned excl, t_all;
    const unsigned inc = rs_wave_excl_scan(len, excl, t_all);
    const unsigned parts = rs_pick_parts<MB_IMG, MB_PARTS>(inc);
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = rs_lane(inc, step * (ps + 1u) - 1u); /* one past its last */
      const bool mine = len && excl >= b0 && excl < b1;
      const uint64_t g0 = g_tile + b0;
      const unsigned ph = (unsigned)(g0 & 15u);
      if (mine) {
        mb_write_sink w = {img + ph + (excl - b0), 0u};
        mb_emit_line(w, m, a.contig_w, a.clen1);
      }
      rs_wave_sync();
      rs_copy_out(img, out + (g0 - ph), lane, rs_copy_ranges(ph, b1 - b0)); /* the image [ph, ph + t) -> out[g0, g0 + t) */
      rs_wave_sync();
      b0 = b1;
    }
  }
}

/* ---- the combined-strand CpG table ---------------------------------------------------------------------------------------------------------- */
#define MC_PAIR 0x8000u /* line_len[i]: the line is a pair's */
static_assert(MB_LINE_MAX < MC_PAIR, "bit 15 of a line's length is free");

/* what record / position j is to the pairing: bits 1 = a half, 2 = a minus half */
struct mc_half {
  unsigned bits, pf; /* pf: phred | flt << 8 */
  uint32_t pos, a, b;
};

/* j < n, and its emit byte not 0 where there is one: the record's first 16 bytes say whether it is a candidate, and only a candidate's
 * counts are fetched */
__device__ __forceinline__ mc_half mc_half_of(const mb_args &a, uint64_t j, uint64_t n) {
  mc_half h = {0u, 0u, 0u, 0u, 0u};
  if (j >= n || (a.emit && !a.emit[j])) return h;
  const uint4 *lo = reinterpret_cast<const uint4 *>(a.src.recs ? a.src.recs + j * 128u : a.src.core + j * 64u);
  const uint4 v0 = lo[0];
  const unsigned emit = v0.y & 0xffu, gt = (v0.y >> 8) & 0xffu, flt = v0.z & 0xffu, phred = (v0.z >> 8) & 0xffu, cg = v0.z >> 24;
  if (!emit || (gt != 4u && gt != 7u) || cg != 'C') return h;
  if (phred < a.min_phred || (a.pass_only && flt)) return h;
  const uint4 c1 = (a.src.recs ? lo + 4 : reinterpret_cast<const uint4 *>(a.src.aux + j * 64u))[1]; /* counts[4 .. 7] */
  const bool minus = gt == 7u;
  h.a = minus ? c1.z : c1.y;
  h.b = minus ? c1.x : c1.w;
  if (!(h.a | h.b)) return h;
  h.bits = minus ? 3u : 1u;
  h.pf = phred | flt << 8;
  h.pos = v0.x;
  return h;
}

/* a line of the combined table */
struct mc_site {
  uint32_t start;
  uint64_t A, B;
  unsigned strand, phred, flt;
};

__device__ __forceinline__ void mc_make_site(mc_site &m, uint32_t pos, bool minus, uint32_t a, uint32_t b, unsigned pf, bool pair, uint32_t na, uint32_t nb,
                                             unsigned npf) {
  m.start = pos - (minus ? 2u : 1u);
  m.A = (uint64_t)a + (pair ? na : 0u);
  m.B = (uint64_t)b + (pair ? nb : 0u);
  const unsigned ph = pf & 0xffu, nph = npf & 0xffu;
  m.phred = pair && nph < ph ? nph : ph;
  m.flt = (pf >> 8) | (pair ? npf >> 8 : 0u);
  m.strand = pair ? '.' : (minus ? '-' : '+');
}

template <class S>
__device__ __forceinline__ void mc_emit_line(S &s, const mc_site &m, const uint32_t *contig_w, unsigned clen1) {
  const uint64_t cov = m.A + m.B, end = (uint64_t)m.start + 2u;
  const unsigned pct = mb_pct(m.A, cov);
  s.words(contig_w, clen1);
  mb_put_dec(s, m.start, '\t');
  mb_put_dec(s, end, '\t');
  s.bytes(MB_STR4('C', 'G', '\t', 0), 3u);
  mb_put_dec(s, cov < 1000ull ? cov : 1000ull, '\t');
  s.bytes((uint64_t)m.strand | (uint64_t)'\t' << 8, 2u);
  mb_put_dec(s, m.start, '\t');
  mb_put_dec(s, end, '\t');
  {
    const unsigned k = pct / 10u;
    const unsigned r = k < 5u ? (k ? 5u + 50u * k : 0u) : 255u, g = k <= 5u ? 255u : (k < 10u ? 5u + 50u * (10u - k) : 0u);
    mb_put_dec(s, r, ',');
    mb_put_dec(s, g, ',');
    s.bytes((uint64_t)'0' | (uint64_t)'\t' << 8, 2u);
  }
  mb_put_dec(s, cov, '\t');
  mb_put_dec(s, pct, '\t');
  mb_put_dec(s, m.A, '\t');
  mb_put_dec(s, m.B, '\t');
  mb_put_dec(s, m.phred, '\t');
  s.bytes(((m.flt & 127u) ? MB_STR4('f', 'a', 'i', 'l') : ((m.flt & 128u) ? MB_STR4('m', 'a', 'c', '1') : MB_STR4('P', 'A', 'S', 'S'))) | (uint64_t)'\n' << 32, 5u);
}

/* as bsc_meth_size_kernel; line_len[i] |= MC_PAIR for a pair's line; sums[0 .. 3] += lines, their A, their B, pairs written */
extern "C" __global__ __launch_bounds__(256) void bsc_meth_cpg_size_kernel(mb_args a, uint32_t n_tiles, unsigned long long *__restrict__ tile_bytes,
                                                                           uint16_t *__restrict__ line_len, unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long s_sum[4];
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n = rs_clamp_n(a.src);
  const uint64_t min_cov = a.min_cov > 1u ? a.min_cov : 1u;
  if (threadIdx.x < 4u) s_sum[threadIdx.x] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  __syncthreads();
  unsigned long long n_lines = 0ull, sum_a = 0ull, sum_b = 0ull, n_pairs = 0ull; /* this lane's */
  for (uint32_t tile = blockIdx.x * MB_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * MB_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const mc_half h = mc_half_of(a, i, n);
    /* the next record's verdict and what a pair takes from it; the previous record's verdict */
    mc_half nx;
    nx.bits = __shfl_down(h.bits, 1);
    nx.pos = __shfl_down(h.pos, 1);
    nx.a = __shfl_down(h.a, 1);
    nx.b = __shfl_down(h.b, 1);
    nx.pf = __shfl_down(h.pf, 1);
    unsigned pv_bits = __shfl_up(h.bits, 1);
    uint32_t pv_pos = __shfl_up(h.pos, 1);
    if (lane == 63u) { /* the next tile's first record: only a plus half looks */
      nx.bits = 0u;
      if (h.bits == 1u) nx = mc_half_of(a, i + 1u, n);
    }
    if (lane == 0u) { /* the previous tile's last record: only a minus half looks */
      pv_bits = 0u;
      if (h.bits == 3u && i) {
        const mc_half pv = mc_half_of(a, i - 1u, n);
        pv_bits = pv.bits;
        pv_pos = pv.pos;
      }
    }
    const bool pair = h.bits == 1u && nx.bits == 3u && (uint64_t)nx.pos == (uint64_t)h.pos + 1u;
    const bool taken = h.bits == 3u && pv_bits == 1u && (uint64_t)pv_pos + 1u == (uint64_t)h.pos; /* its pair's line is the plus half's */
    unsigned len = 0u;
    if (h.bits && !taken) {
      mc_site m;
      mc_make_site(m, h.pos, h.bits == 3u, h.a, h.b, h.pf, pair, nx.a, nx.b, nx.pf);
      if (m.A + m.B >= min_cov) {
        mb_count_sink c = {0u};
        mc_emit_line(c, m, a.contig_w, a.clen1);
        len = c.len;
        n_lines++;
        sum_a += m.A;
        sum_b += m.B;
        n_pairs += pair;
      }
    }
    if (i < a.src.max_recs) line_len[i] = (uint16_t)(len | (len && pair ? MC_PAIR : 0u));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    n_lines += __shfl_xor(n_lines, d);
    sum_a += __shfl_xor(sum_a, d);
    sum_b += __shfl_xor(sum_b, d);
    n_pairs += __shfl_xor(n_pairs, d);
  }
  if (lane == 0 && n_lines) {
    atomicAdd(&s_sum[0], n_lines);
    atomicAdd(&s_sum[1], sum_a);
    atomicAdd(&s_sum[2], sum_b);
    atomicAdd(&s_sum[3], n_pairs);
  }
  __syncthreads();
  if (threadIdx.x < 4u && s_sum[threadIdx.x]) atomicAdd(sums + threadIdx.x, s_sum[threadIdx.x]);
}

/* record j's fields for a line the size pass has decided on: no rule, the two loads leave together */
__device__ __forceinline__ void mc_fields_of(const mb_args &a, uint64_t j, uint32_t &pos, bool &minus, uint32_t &ca, uint32_t &cb, unsigned &pf) {
  const uint4 *lo = reinterpret_cast<const uint4 *>(a.src.recs ? a.src.recs + j * 128u : a.src.core + j * 64u);
  const uint4 v0 = lo[0], c1 = (a.src.recs ? lo + 4 : reinterpret_cast<const uint4 *>(a.src.aux + j * 64u))[1];
  pos = v0.x;
  minus = ((v0.y >> 8) & 0xffu) == 7u;
  ca = minus ? c1.z : c1.y;
  cb = minus ? c1.x : c1.w;
  pf = ((v0.z >> 8) & 0xffu) | (v0.z & 0xffu) << 8;
}

extern "C" __global__ __launch_bounds__(256) void bsc_meth_cpg_write_kernel(mb_args a, uint32_t n_tiles, const unsigned long long *__restrict__ tile_off,
                                                                            const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out,
                                                                            uint64_t out_cap, unsigned long long *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[MB_WAVES][MB_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = rs_clamp_n(a.src);
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = tile_off[n_tiles];
  for (uint32_t tile = blockIdx.x * MB_WAVES + wid; tile < n_tiles; tile += gridDim.x * MB_WAVES) {
    if ((uint64_t)tile * 64u >= n) break; /* wave-uniform; later tiles of this wave lie further out still */
    const uint64_t g_tile = tile_off[tile], g_end = tile_off[tile + 1u];
    if (g_end == g_tile) continue;  /* no line in this tile: nothing of it is read */
    if (g_end > out_cap) continue;  /* the host reports the overflow from *total */
    const uint64_t i = (uint64_t)tile * 64u + lane;
    const unsigned ll = i < n ? line_len[i] : 0u;
    const unsigned len = ll & (MC_PAIR - 1u);
    const bool pair = (ll & MC_PAIR) != 0u;
    const unsigned up = __shfl_up(ll, 1);
    const bool lent = lane != 0u && (up & MC_PAIR); /* the minus half of the pair's line one lane up (lane 0's pair is read by the tile before) */
    uint32_t pos = 0u, ca = 0u, cb = 0u;
    unsigned pf = 0u;
    bool minus = false;
    if (len || lent) mc_fields_of(a, i, pos, minus, ca, cb, pf); /* (lent: i < n — the size pass found it a half) */
    uint32_t na = __shfl_down(ca, 1), nb = __shfl_down(cb, 1);
    unsigned npf = __shfl_down(pf, 1);
    if (lane == 63u && pair) { /* i + 1 < n: the size pass paired it */
      uint32_t npos;
      bool nminus;
      mc_fields_of(a, i + 1u, npos, nminus, na, nb, npf);
    }
    mc_site m;
    mc_make_site(m, pos, minus, ca, cb, pf, pair, na, nb, npf);
    unsigned excl, t_all;
    const unsigned inc = rs_wave_excl_scan(len, excl, t_all);
    const unsigned parts = rs_pick_parts<MB_IMG, MB_PARTS>(inc);
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = rs_lane(inc, step * (ps + 1u) - 1u); /* one past its last */
      const bool mine = len && excl >= b0 && excl < b1;
      const uint64_t g0 = g_tile + b0;
      const unsigned ph = (unsigned)(g0 & 15u);
      if (mine) {
        mb_write_sink w = {img + ph + (excl - b0), 0u};
        mc_emit_line(w, m, a.contig_w, a.clen1);
      }
      rs_wave_sync();
      rs_copy_out(img, out + (g0 - ph), lane, rs_copy_ranges(ph, b1 - b0)); /* the image [ph, ph + t) -> out[g0, g0 + t) */
      rs_wave_sync();
      b0 = b1;
    }
  }
}

extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

/*
 * recs[<= max_recs] packed records, *n_recs of them (device u64) — or, recs == NULL, core[max_recs] / aux[max_recs] as the reads-in
 * chain leaves them, emit its byte per position or NULL — -> out[<= out_cap] lines; totals[0] = the stream's length (also when it
 * exceeds out_cap: then only the tiles that fit whole are written), totals[1 .. 3] += lines, the sum of their a, of their b (the
 * caller zeroes them).  cpg != 0: the combined-strand table (contexts must be BSC_METH_CPG), totals[1 .. 4] += lines, sum A, sum B,
 * pairs written.  contig: the name, contig_len (1 .. 255) bytes, checked by the caller.  tile_bytes / tile_off: max_recs / 64
 * (rounded up) + 1 u64 each; line_len: max_recs u16; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of the tiles + 1.
 */
extern "C" int bsc_dev_launch_meth(const void *recs, const void *core, const void *aux, const void *n_recs, uint64_t max_recs, const void *emit,
                                   const char *contig, uint32_t contig_len, const bsc_meth_params *par, void *tile_bytes, void *tile_off, void *line_len,
                                   void *scan_tmp, size_t scan_tmp_bytes, void *out, uint64_t out_cap, void *totals, int cpg, int num_cus,
                                   void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!contig_len || contig_len > MB_CONTIG_MAX || !par) return (int)hipErrorInvalidValue;
  if (cpg && par->contexts != BSC_METH_CPG) return (int)hipErrorInvalidValue;
  mb_args a;
  a.src = rs_make_src(recs, core, aux, n_recs, max_recs, NULL, NULL, NULL, 0u);
  a.emit = recs ? NULL : (const uint8_t *)emit;
  a.all_contexts = par->contexts == BSC_METH_ALL;
  a.min_cov = par->min_cov;
  a.min_phred = par->min_phred;
  a.pass_only = par->pass_only != 0;
  a.clen1 = contig_len + 1u;
  for (int k = 0; k < 64; k++) a.contig_w[k] = 0u;
  __builtin_memcpy(a.contig_w, contig, contig_len);
  ((char *)a.contig_w)[contig_len] = '\t';
  const uint64_t nt64 = (max_recs + 63u) / 64u;
  if (nt64 > 0x7fffffffull) return (int)hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)nt64;
  unsigned grid = (n_tiles + MB_WAVES - 1u) / MB_WAVES;
  if (grid > (unsigned)num_cus * 8u) grid = (unsigned)num_cus * 8u;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(cpg ? bsc_meth_cpg_size_kernel : bsc_meth_size_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (unsigned long long *)tile_bytes,
                     (uint16_t *)line_len, (unsigned long long *)totals + 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int rc = bsc_dev_scan_u64(tile_bytes, tile_off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(cpg ? bsc_meth_cpg_write_kernel : bsc_meth_write_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles,
                     (const unsigned long long *)tile_off, (const uint16_t *)line_len, (uint8_t *)out, out_cap, (unsigned long long *)totals);
  return (int)hipGetLastError();
}
