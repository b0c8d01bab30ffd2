/*
 * vcftextdev.hip — a block's written records as VCF TEXT on the device: for every record with emit != 0, in position order, the
 * line bsc_vcf_format_rec writes for it and '\n' (the reference's -O v; through the BGZF writer, bgzfdev.hip, its -O z).  The
 * emitter is vcftext_emit.h, the number formatter fmtg_dev.h; the host form csrc/vcf_format.c is the checker of both.  The
 * placement — record loader, name lookup, wave prefix sum, the parts, the image's copy-out — is recstream_dev.h's, shared with
 * the BCF encoder (bcfdev.hip):
 *
 *   bsc_vtext_size_kernel   one wave per tile of 64 records / positions: every lane the length of its line (the emitter over the
 *                           counting sink) -> line_len[i] (u16; 0 = nothing written), the tile's sum -> tile_bytes[tile]
 *   (exclusive scan of the tile sums, rocPRIM u64: sort.hip; one more entry behind the last tile = the stream's length)
 *   bsc_vtext_write_kernel  one wave per tile: lane offsets from a wave prefix sum of line_len (fetched a tile ahead: a position
 *                           without a record costs those two bytes and nothing of its record), every lane writes its line into
 *                           the wave's LDS image of the tile's span of the stream, then the wave copies the image out.  A tile
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
  rs_src src;
  uint32_t clen1;        /* the contig's name and the tab behind it, bytes */
  uint32_t contig_w[64]; /* those bytes, zero padded */
};

/* the name of a flagged record (the BCF encoder's rule: rs_found set, the position listed, at most 63 bytes), as far as a host "%s"
 * would print it: up to a NUL */
__device__ __forceinline__ unsigned vt_find_name(const vt_args &a, const vt_rec &r, const uint8_t *&id) {
  uint32_t l = rs_find_name(a.src, r, id);
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
  const uint64_t n = rs_clamp_n(a.src);
  if (blockIdx.x == 0 && threadIdx.x == 0) tile_bytes[n_tiles] = 0ull;
  unsigned n_written = 0, n_clamped = 0; /* wave-uniform */
  for (uint32_t tile = blockIdx.x * VT_WAVES + (threadIdx.x >> 6); tile < n_tiles; tile += gridDim.x * VT_WAVES) {
    const uint64_t i = (uint64_t)tile * 64u + lane;
    unsigned len = 0u;
    bool clamped = false;
    vt_rec r;
    if (i < n && rs_load(r, a.src, i, -1)) {
      const uint8_t *id;
      const unsigned id_len = vt_find_name(a, r, id);
      vt_count_sink c = {0u};
      vt_emit_line(c, r, a.contig_w, a.clen1, id, id_len, clamped);
      len = c.len;
    }
    if (i < a.src.max_recs) line_len[i] = (uint16_t)len;
    n_clamped += (unsigned)__popcll(__ballot(clamped));
    n_written += (unsigned)__popcll(__ballot(len != 0u));
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) len += __shfl_xor(len, d);
    if (lane == 0) tile_bytes[tile] = len;
  }
  const unsigned cnt[2] = {n_clamped, n_written};
  rs_flush_counts(cnt, err);
}

extern "C" __global__ __launch_bounds__(256) void bsc_vtext_write_kernel(vt_args a, uint32_t n_tiles, const unsigned long long *__restrict__ tile_off,
                                                                         const uint16_t *__restrict__ line_len, uint8_t *__restrict__ out, uint64_t out_cap,
                                                                         unsigned long long *__restrict__ total) {
  __shared__ __attribute__((aligned(16))) uint8_t s_img[VT_WAVES][VT_IMG + 32u]; /* 15 bytes of phase in front */
  const unsigned lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint8_t *const img = s_img[wid];
  const uint64_t n = rs_clamp_n(a.src);
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
      (void)rs_load(r, a.src, (uint64_t)tile * 64u + lane, 1);
      id_len = vt_find_name(a, r, id);
    }
    unsigned excl, t_all;
    const unsigned inc = rs_wave_excl_scan(len, excl, t_all);
    const uint64_t g_tile = tile_off[tile];
    if (g_tile + t_all > out_cap) continue; /* the host reports the overflow from *total */
    const unsigned parts = rs_pick_parts<VT_IMG, 16u>(inc);
    const unsigned step = 64u / parts;
    unsigned b0 = 0u; /* the part's first byte within the tile */
    for (unsigned ps = 0; ps < parts; ps++) {
      const unsigned b1 = rs_lane(inc, step * (ps + 1u) - 1u); /* one past its last */
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
      rs_wave_sync();
      rs_copy_out(img, out + (g0 - ph), lane, rs_copy_ranges(ph, b1 - b0)); /* the image [ph, ph + t) -> out[g0, g0 + t) */
      rs_wave_sync();
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
  a.src = rs_make_src(recs, core, aux, n_recs, max_recs, name_pos, name_off, name_bytes, n_names);
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
