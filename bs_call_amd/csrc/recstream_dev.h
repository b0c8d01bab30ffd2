/*
 * recstream_dev.h — a tile's variable-length records placed into the output stream: what the BCF encoder (bcfdev.hip) and the
 * VCF text encoder (vcftextdev.hip) have in common.  A wave owns a tile of 64 records / positions; every lane knows the length
 * of what it writes (0: nothing).  The lane offsets are a wave prefix sum; the lanes write into the wave's LDS image of the
 * tile's span of the stream, the image starting at the span's phase within 16 bytes; the wave then copies the image out: whole
 * 16-byte pieces as one dwordx4 store per lane, the ragged head and tail byte by byte — the neighbouring tiles own the other
 * bytes of those pieces, so an index that is off by one there is another tile's record silently overwritten.  A tile whose
 * span does not fit the image goes out in the fewest parts of equal lane counts that do.
 *
 * The index arithmetic (rs_copy_ranges, rs_pick_parts_at) is __host__ __device__ and compiles for a host compiler as
 * fmtg_dev.h does: tests/test_recstream_host.py walks it exhaustively.  Everything else is device code.
 */
#ifndef BSC_RECSTREAM_DEV_H
#define BSC_RECSTREAM_DEV_H
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_FN __host__ __device__ __forceinline__
#define RS_MFN __host__ __device__ __forceinline__
#else
#define RS_FN static inline
#define RS_MFN inline
#endif

#define RS_LANES 64u
#define RS_PIECE 16u /* the copy-out's unit: one dwordx4 store; the wave's stride is RS_LANES of them */

/* the record's fields as the emitters read them: one 128-byte record (bsc_vcf_rec) in eight 16-byte loads */
struct rs_rec {
  uint32_t w[32];
  RS_MFN uint8_t byte(unsigned o) const { return (uint8_t)(w[o >> 2] >> (8u * (o & 3u))); }
};

/* The image [ph, ph + t) -> the stream, ph < 16 the phase of the span's first byte: bytes [ph, head_end) singly (nothing when
 * ph == 0), the pieces of [body0, body1) whole, bytes [tail0, end) singly. */
struct rs_ranges {
  unsigned head0, head_end, body0, body1, tail0, end;
};
RS_FN rs_ranges rs_copy_ranges(unsigned ph, unsigned t) {
  rs_ranges c;
  c.head0 = ph;
  c.end = ph + t;
  c.head_end = ph ? (c.end < RS_PIECE ? c.end : RS_PIECE) : 0u;
  c.body0 = ph ? RS_PIECE : 0u;
  c.body1 = c.end & ~(RS_PIECE - 1u);
  c.tail0 = c.body1 > c.head_end ? c.body1 : c.head_end;
  return c;
}

/* One part when the tile's span fits the image (the usual case), else the fewest parts (2, 4 .. MAX_PARTS) of equal lane counts
 * that each do; MAX_PARTS when none does — the caller's static_assert: 64 / MAX_PARTS of the longest records fit.  at(l): the
 * inclusive prefix of the lengths at lane l. */
template <unsigned IMG, unsigned MAX_PARTS, class At>
RS_FN unsigned rs_pick_parts_at(At at) {
  unsigned parts = 1u;
  if (at(RS_LANES - 1u) > IMG) {
    for (parts = 2u; parts < MAX_PARTS; parts <<= 1) {
      const unsigned step = RS_LANES / parts;
      bool fits = true;
      unsigned prev = 0u;
      for (unsigned q = 0; q < parts; q++) {
        const unsigned e = at(step * (q + 1u) - 1u);
        fits = fits && e - prev <= IMG;
        prev = e;
      }
      if (fits) break;
    }
  }
  return parts;
}

#if defined(__HIPCC__)
/* where the records are, and the block's names table */
struct rs_src {
  const uint8_t *recs;              /* bsc_vcf_rec[] — or NULL: the records are taken where the chain left them, */
  const uint8_t *core, *aux;        /* bsc_vcf_core[] and the chain's aux array (64 B per position: the second half of a bsc_vcf_rec) */
  const unsigned long long *n_recs; /* device: how many records / positions (NULL: max_recs of them) */
  uint64_t max_recs;                /* never more than this (the arrays' size) */
  const uint32_t *name_pos;         /* n_names sorted 1-based positions, or NULL */
  const uint32_t *name_off;         /* n_names + 1 offsets into name_bytes */
  const uint8_t *name_bytes;
  uint32_t n_names;
};

/* (host) the launchers' arguments as they arrive; no table without positions */
static inline rs_src rs_make_src(const void *recs, const void *core, const void *aux, const void *n_recs, uint64_t max_recs, const void *name_pos,
                                 const void *name_off, const void *name_bytes, uint32_t n_names) {
  rs_src a;
  a.recs = (const uint8_t *)recs;
  a.core = (const uint8_t *)core;
  a.aux = (const uint8_t *)aux;
  a.n_recs = (const unsigned long long *)n_recs;
  a.max_recs = max_recs;
  a.name_pos = (const uint32_t *)name_pos;
  a.name_off = (const uint32_t *)name_off;
  a.name_bytes = (const uint8_t *)name_bytes;
  a.n_names = name_pos ? n_names : 0u;
  return a;
}

__device__ __forceinline__ uint64_t rs_clamp_n(const rs_src &a) {
  if (!a.n_recs) return a.max_recs;
  const unsigned long long n = *a.n_recs;
  return n < a.max_recs ? n : a.max_recs;
}

/* record / position i into registers; false: nothing is written for it (emit == 0).  gate == 0: nothing to load.  gate < 0: the
 * flag is in the record's first 16 bytes — a position that writes no record costs those (their 64-byte sector), and a record's
 * other loads wait for them.  gate > 0: the caller knows there is a record, and its eight loads leave together. */
__device__ __forceinline__ bool rs_load(rs_rec &r, const rs_src &a, uint64_t i, int gate) {
  if (gate == 0) return false;
  const uint4 *lo = reinterpret_cast<const uint4 *>(a.recs ? a.recs + i * 128u : a.core + i * 64u);
  const uint4 v0 = lo[0];
  r.w[0] = v0.x; r.w[1] = v0.y; r.w[2] = v0.z; r.w[3] = v0.w;
  if (gate < 0 && !(v0.y & 0xffu)) return false; /* bsc_vcf_core.emit */
  const uint4 *hi = a.recs ? lo + 4 : reinterpret_cast<const uint4 *>(a.aux + i * 64u);
#pragma unroll
  for (int k = 1; k < 4; k++) {
    const uint4 v = lo[k];
    r.w[4 * k] = v.x; r.w[4 * k + 1] = v.y; r.w[4 * k + 2] = v.z; r.w[4 * k + 3] = v.w;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint4 v = hi[k];
    r.w[16 + 4 * k] = v.x; r.w[17 + 4 * k] = v.y; r.w[18 + 4 * k] = v.z; r.w[19 + 4 * k] = v.w;
  }
  return true;
}

/* the name of a flagged record (rs_found set): binary search of its position in the block's table.  Returns the table's length
 * of it, whatever that is — how much of it is written is the caller's rule. */
__device__ __forceinline__ unsigned rs_find_name(const rs_src &a, const rs_rec &r, const uint8_t *&id) {
  id = nullptr;
  if (!a.n_names || !r.byte(113)) return 0u;
  const uint32_t pos = r.w[0];
  uint32_t lo = 0, hi = a.n_names;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.name_pos[mid] < pos) lo = mid + 1u; else hi = mid;
  }
  if (lo >= a.n_names || a.name_pos[lo] != pos) return 0u;
  const uint32_t o0 = a.name_off[lo], o1 = a.name_off[lo + 1u];
  id = a.name_bytes + o0;
  return o1 - o0;
}

/* v of lane l, l wave-uniform */
__device__ __forceinline__ unsigned rs_lane(unsigned v, unsigned l) { return (unsigned)__builtin_amdgcn_readlane((int)v, (int)l); }

/* the inclusive prefix of len over the wave; excl: the exclusive one, total: the tile's sum */
__device__ __forceinline__ unsigned rs_wave_excl_scan(unsigned len, unsigned &excl, unsigned &total) {
  const unsigned lane = threadIdx.x & 63u;
  unsigned inc = len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned v = __shfl_up(inc, d);
    if (lane >= (unsigned)d) inc += v;
  }
  excl = inc - len;
  total = rs_lane(inc, RS_LANES - 1u);
  return inc;
}

struct rs_lane_of {
  unsigned inc;
  __device__ __forceinline__ unsigned operator()(unsigned l) const { return rs_lane(inc, l); }
};
template <unsigned IMG, unsigned MAX_PARTS>
__device__ __forceinline__ unsigned rs_pick_parts(unsigned inc) {
  return rs_pick_parts_at<IMG, MAX_PARTS>(rs_lane_of{inc});
}

/* The lanes of a wave run in lockstep but the compiler does not know it: what one lane has stored to the image is another lane's to
 * read (or to store over) only behind this — the release orders this lane's LDS stores before the barrier, the acquire keeps the
 * loads and stores that follow behind it.  No instruction of its own beyond the wait for the LDS. */
__device__ __forceinline__ void rs_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* the image -> dst, both counted from the 16-byte piece that holds the span's first byte (dst = out + g0 - ph) */
__device__ __forceinline__ void rs_copy_out(const uint8_t *img, uint8_t *dst, unsigned lane, const rs_ranges &c) {
  if (lane >= c.head0 && lane < c.head_end) dst[lane] = img[lane];
  for (unsigned o = c.body0 + RS_PIECE * lane; o < c.body1; o += RS_PIECE * RS_LANES)
    *reinterpret_cast<uint4 *>(dst + o) = *reinterpret_cast<const uint4 *>(img + o);
  if (c.tail0 + lane < c.end) dst[c.tail0 + lane] = img[c.tail0 + lane];
}

/* dst[k] += the workgroup's sum of cnt[k], cnt wave-uniform: once per workgroup — atomics on one word are served one after the
 * other, 23 ns each (one per wave of 12 288 waves was the whole 0.25 ms of the first form of the BCF size kernel) */
template <unsigned N>
__device__ __forceinline__ void rs_flush_counts(const unsigned (&cnt)[N], unsigned long long *dst) {
  __shared__ unsigned s_cnt[N];
  if (threadIdx.x < N) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (unsigned k = 0; k < N; k++)
      if (cnt[k]) atomicAdd(&s_cnt[k], cnt[k]);
  }
  __syncthreads();
  if (threadIdx.x < N && s_cnt[threadIdx.x]) atomicAdd(dst + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}
#endif /* __HIPCC__ */

#endif
