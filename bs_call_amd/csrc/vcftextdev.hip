/*
 * vcftextdev.hip — a block's written records as VCF TEXT on the device: for every record with emit != 0, in position order, the
 * line bsc_vcf_format_rec writes for it and '\n' (the reference's -O v; through the BGZF writer, bgzfdev.hip, its -O z).  The
 * emitter is vcftext_emit.h, the number formatter fmtg_dev.h; the host form csrc/vcf_format.c is the checker of both.  The
 * placement is bcfdev.hip's:
 *
 *   bsc_vtext_size_kernel   one wave per tile of 64 records / positions: every lane the length of its line (the emitter over the
 *                           counting sink) -> line_len[i] (u16; 0 = nothing written), the tile's sum -> tile_bytes[tile]
 *   (exclusive scan of the tile sums, rocPRIM u64: sort.hip; one more entry behind the last tile = the stream's length)
 *   bsc_vtext_write_kernel  one wave per tile: lane offsets from a wave prefix sum of line_len (fetched a tile ahead: a position
 *                           without a record costs those two bytes and nothing of its record), every lane writes its line into
 *                           the wave's LDS image of the tile's span of the stream, the image starting at the span's phase within
 *                           16 bytes; then the wave copies the image out: whole 16-byte pieces as one dwordx4 store per lane, the
 *                           ragged head and tail byte by byte (the neighbouring tiles own the other bytes of those pieces).  A tile
 *                           whose span does not fit the image (12 KB) goes out in 2, 4, 8 or 16 parts.
 *
 * The lengths are kept between the passes because a line costs far more arithmetic than a BCF record (six %g conversions and
 * some twenty decimal ones): the write pass does not run the emitter a second time to find its lane offsets.
 *
 * Two sources, as the BCF encoder: packed records (bsc_vcf_text_block_device), or the per-position arrays the reads-in chain
 * leaves (bsc_vcf_text_sites_device): the size pass then reads a position's first 16 bytes (its emit flag) and the rest only of
 * a record that is written.  The chain's length byte is not used: it holds BCF lengths.
 *
 * Longest line: the contig's name (<= 255 bytes) + 410 = 665 bytes (vcftext_emit.h has the sum); a line's length fits 16 bits,
 * four lines always fit the image.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bscall_amd.h"
#include "vcftext_emit.h"

static_assert(sizeof(bsc_vcf_rec) == 128, "bsc_vcf_rec is 128 bytes");

#define VT_WAVES 4u
#define VT_IMG 12288u /* the wave's image: a tile of 64 ordinary lines (~110 bytes each) in one part */
static_assert(VT_IMG >= 4u * VT_LINE_MAX && VT_IMG % 16u == 0u, "a sixteenth of a tile of the longest lines must fit the wave's image");

struct vt_args {
  const uint8_t *recs;              /* bsc_vcf_rec[] — or NULL: */
  const uint8_t *core, *aux;        /* bsc_vcf_core[] and the chain's aux array (the second half of a bsc_vcf_rec) */
  const unsigned long long *n_recs; /* device: how many records (NULL: max_recs of them) */
  uint64_t max_recs;
  const uint32_t *name_pos; /* n_names sorted 1-based positions, or NULL */
  const uint32_t *name_off; /* n_names + 1 offsets into name_bytes */
  const uint8_t *name_bytes;
  uint32_t n_names;
  uint32_t clen1;        /* the contig's name and the tab behind it, bytes */
  uint32_t contig_w[64]; /* those bytes, zero padded */
};

__device__ __forceinline__ uint64_t vt_clamp_n(const vt_args &a) {
  if (!a.n_recs) return a.max_recs;
  const unsigned long long n = *a.n_recs;
  return n < a.max_recs ? n : a.max_recs;
}

/* record / position i into registers.  probe: first the 16 bytes that hold the emit flag — false when it is 0 */
__device__ __forceinline__ bool vt_load(vt_rec &r, const vt_args &a, uint64_t i, bool probe) {
  const uint4 *lo = reinterpret_cast<const uint4 *>(a.recs ? a.recs + i * 128u : a.core + i * 64u);
  const uint4 v0 = lo[0];
  r.w[0] = v0.x; r.w[1] = v0.y; r.w[2] = v0.z; r.w[3] = v0.w;
  if (probe && !(v0.y & 0xffu)) return false; /* bsc_vcf_core.emit */
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

/* the name of a flagged record (the BCF encoder's rule: rs_found set, the position listed, at most 63 bytes), as far as a host "%s"
 * would print it: up to a NUL */
__device__ __forceinline__ unsigned vt_find_name(const vt_args &a, const vt_rec &r, const uint8_t *&id) {
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
  uint32_t l = o1 - o0;
  l = l > VT_ID_MAX ? VT_ID_MAX : l;
  for (uint32_t k = 0; k < l; k++)
    if (!id[k]) return k;
  return l;
}

/* n_tiles = tiles of max_recs; tile_bytes[n_tiles] = 0 (so that the scan's last output is the stream's length); err[0] += records
 * written with a clamped gt / n_gl, err[1] += records written */
extern "C" __global__ __launch_bounds__(256) void bsc_vtext_size_kernel(vt_args a, uint32_t n_tiles, unsigned long long *__restrict__ tile_bytes,
                                                                        uint16_t *__restrict__ line_len, unsigned long long *__restrict__ err) {
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t n = vt_clamp_n(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  unsigned n_written = 0, n_clamped = 0; /* wave-uniform */
  for (uint32_t tile = blockIdx.x * VT_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * VT_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    bool clamped = false;
    vt_rec r;
    if (i < n && vt_load(r, a, i, true)) {
      const uint8_t *id;
      const unsigned id_len = vt_find_name(a, r, id);
      vt_count_sink c = {0u};
      vt_emit_line(c, r, a.contig_w, a.clen1, id, id_len, clamped);
      len = c.len;
    }
    if (i < a.max_recs) line_len[i] = (uint16_t)len;
    n_clamped += (unsigned)__popcll(__ballot(clamped));
    n_written += (unsigned)__popcll(__ballot(len != 0u));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
  /* the totals once per workgroup: atomics on one word are served one after the other */
  __shared__ unsigned s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  if (lane == 0 && n_written) atomicAdd(&s_cnt[1], n_written);
  if (lane == 0 && n_clamped) atomicAdd(&s_cnt[0], n_clamped);
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(err + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

extern "C" __global__ __launch_bounds__(256) void bsc_vtext_write_kernel(vt_args a, uint32_t n_tiles, const unsigned long long *__restrict__ tile_off,
                                                                         const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out, uint64_t out_cap,
                                                                         unsigned long long *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[VT_WAVES][VT_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = vt_clamp_n(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = tile_off[n_tiles];
  const uint32_t tile0 = blockIdx.x * VT_WAVES + wid;
  unsigned len_next = 0u;
  if (tile0 < n_tiles && (uint64_t)tile0 * 64u + lane < n) len_next = line_len[(uint64_t)tile0 * 64u + lane];
  for (uint32_t tile = tile0; tile < n_tiles; tile += gridDim.x * VT_WAVES) {
    if ((uint64_t)tile * 64u >= n) break; /* wave-uniform; later tiles of this wave lie further out still */
    const unsigned len = len_next;
    {
      const uint64_t nt = (uint64_t)tile + (uint64_t)gridDim.x * VT_WAVES;
      len_next = 0u;
      if (nt < n_tiles && nt * 64u + lane < n) len_next = line_len[nt * 64u + lane];
    }
    vt_rec r;
    const uint8_t *id = nullptr;
    unsigned id_len = 0u;
    if (len) {
      (void)vt_load(r, a, (uint64_t)tile * 64u + lane, false);
      id_len = vt_find_name(a, r, id);
    }
    /* exclusive prefix of the lengths over the wave */
    unsigned inc = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned v = __shfl_up(inc, d);
      if (lane >= (unsigned)d) inc += v;
    }
    const unsigned excl = inc - len;
    const unsigned t_all = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);
    const uint64_t g_tile = tile_off[tile];
    if (g_tile + t_all > out_cap) continue; /* the host reports the overflow from *total */
    /* one part when the tile's span fits the image (the usual case), else the fewest parts of equal lane counts that do */
    unsigned parts = 1u;
    if (t_all > VT_IMG) {
      for (parts = 2u; parts < 16u; parts <<= 1) {
        const unsigned step = 64u / parts;
        bool fits = true;
        unsigned prev = 0u;
        for (unsigned q = 0; q < parts; q++) {
          const unsigned e = (unsigned)__shfl((int)inc, (int)(step * (q + 1u) - 1u));
          fits = fits && e - prev <= VT_IMG;
          prev = e;
        }
        if (fits) break;
      }
    }
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = (unsigned)__shfl((int)inc, (int)(step * (ps + 1u) - 1u)); /* one past its last */
      const bool mine = len && excl >= b0 && excl < b1;
      const uint64_t g0 = g_tile + b0;
      const unsigned ph = (unsigned)(g0 & 15u);
      if (mine) {
        vt_write_sink w = {img + ph + (excl - b0), 0u};
        bool clamped;
        vt_emit_line(w, r, a.contig_w, a.clen1, id, id_len, clamped);
        /* the length the line was placed by is the length written: anything else would be a stream with a hole or an overlap — counted
         * with the clamped records, so a block entry fails instead (never seen: one emitter over two sinks) */
        if (w.len != len) atomicAdd(total + 1, 1ull);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      /* the image [ph, ph + t) -> out[g0, g0 + t) */
      const unsigned t = b1 - b0, end = ph + t;
      uint8_t *const dst = out + (g0 - ph);
      const unsigned head_end = ph ? (end < 16u ? end : 16u) : 0u; /* bytes [ph, head_end) singly */
      if (lane >= ph && lane < head_end) dst[lane] = img[lane];
      const unsigned body0 = ph ? 16u : 0u, body1 = end & ~15u;
      for (unsigned o = body0 + 16u * lane; o < body1; o += 1024u) *reinterpret_cast<uint4 *>(dst + o) = *reinterpret_cast<const uint4 *>(img + o);
      const unsigned tail0 = body1 > head_end ? body1 : head_end;
      if (tail0 + lane < end) dst[tail0 + lane] = img[tail0 + lane];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      b0 = b1;
    }
  }
}

/* the number formatter alone, a value per thread: out16[i] = the characters, zero padding, the length in byte 15 */
extern "C" __global__ __launch_bounds__(256) void bsc_fmt_g_kernel(const uint32_t *__restrict__ v, uint64_t n, uint4 *__restrict__ out16) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const fmtg_str s = fmtg_format(v[i]);
    uint4 o;
    o.x = (uint32_t)s.lo;
    o.y = (uint32_t)(s.lo >> 32);
    o.z = (uint32_t)s.hi;
    o.w = (uint32_t)(s.hi >> 32) | s.n << 24;
    out16[i] = o;
  }
}

extern "C" int bsc_dev_launch_fmt_g(const void *v, uint64_t n, void *out16, int num_cus, void *stream) {
  if (!n) return 0;
  uint64_t grid = (n + 255u) / 256u;
  if (grid > (uint64_t)num_cus * 16u) grid = (uint64_t)num_cus * 16u;
  hipLaunchKernelGGL(bsc_fmt_g_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)v, n, (uint4 *)out16);
  return (int)hipGetLastError();
}

extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */

/*
 * recs[<= max_recs] packed records, *n_recs of them (device u64) — or, recs == NULL, core[max_recs] / aux[max_recs] as the reads-in
 * chain leaves them — -> out[<= out_cap] text; totals[0] = the stream's length (also when it exceeds out_cap: then only the tiles
 * that fit whole are written), totals[1] += records written with a clamped gt / n_gl, totals[2] += records written.  contig: the
 * name, contig_len (1 .. 255) bytes, checked by the caller.  tile_bytes / tile_off: max_recs / 64 (rounded up) + 1 u64 each;
 * line_len: max_recs u16; scan_tmp: bsc_dev_scan_tmp_bytes_u64 of the tiles + 1.
 */
extern "C" int bsc_dev_launch_vcf_text(const void *recs, const void *core, const void *aux, const void *n_recs, uint64_t max_recs, const char *contig,
                                       uint32_t contig_len, const void *name_pos, const void *name_off, const void *name_bytes, uint32_t n_names,
                                       void *tile_bytes, void *tile_off, void *line_len, void *scan_tmp, size_t scan_tmp_bytes, void *out, uint64_t out_cap,
                                       void *totals, int num_cus, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!contig_len || contig_len > VT_CONTIG_MAX) return (int)hipErrorInvalidValue;
  vt_args a;
  a.recs = (const uint8_t *)recs;
  a.core = (const uint8_t *)core;
  a.aux = (const uint8_t *)aux;
  a.n_recs = (const unsigned long long *)n_recs;
  a.max_recs = max_recs;
  a.name_pos = (const uint32_t *)name_pos;
  a.name_off = (const uint32_t *)name_off;
  a.name_bytes = (const uint8_t *)name_bytes;
  a.n_names = name_pos ? n_names : 0u;
  a.clen1 = contig_len + 1u;
  for (int k = 0; k < 64; k++) a.contig_w[k] = 0u;
  __builtin_memcpy(a.contig_w, contig, contig_len);
  ((char *)a.contig_w)[contig_len] = '\t';
  const uint64_t nt64 = (max_recs + 63u) / 64u;
  if (nt64 > 0x7fffffffull) return (int)hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)nt64;
  unsigned grid = (n_tiles + VT_WAVES - 1u) / VT_WAVES;
  if (grid > (unsigned)num_cus * 12u) grid = (unsigned)num_cus * 12u;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(bsc_vtext_size_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (unsigned long long *)tile_bytes, (uint16_t *)line_len,
                     (unsigned long long *)totals + 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int rc = bsc_dev_scan_u64(tile_bytes, tile_off, n_tiles + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_vtext_write_kernel, dim3(grid), dim3(256), 0, s, a, n_tiles, (const unsigned long long *)tile_off, (const uint16_t *)line_len,
                     (uint8_t *)out, out_cap, (unsigned long long *)totals);
  return (int)hipGetLastError();
}
