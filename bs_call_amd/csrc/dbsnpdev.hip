/*
 * dbsnpdev.hip — the two per-block products of a dbSNP index, made on the device from the contig kept in HBM (bsc_dbsnp_attach):
 *
 *   bsc_dbsnp_flags_kernel   rs_found (0 / 1 / 3), a byte per position of x0 .. x0 + n - 1 — what bsc_dbsnp_flags writes on the host and
 *                            the chain kernel reads as `dbsnp`.  A lane forms 16 positions from the two bins its window touches
 *                            (bsc_dbf_window) and stores them as one 16-byte word; the stores start at the first 16-byte boundary of the
 *                            output, whatever its alignment, and the up to 15 bytes in front of it and behind the last whole word are
 *                            written one position per lane by the lanes behind the last word's.
 *   bsc_dbsnp_names_kernel   pos[k] | off[k + 1] | bytes of the range's entries e0 .. e0 + k - 1 — what bsc_dbsnp_names fills on the host,
 *                            in the layout the stream encoders search (recstream_dev.h).  One lane per entry: the offsets are differences
 *                            of the per-entry text offsets made at attach time, so no lane waits for another.
 *
 * The statements are csrc/dbsnpdev_core.h's, the ones tests/dbsnpdev/dbsnp_flat_host.c runs on the CPU.  The host (bscall_api.c) has
 * checked the range and sized both outputs (bsc_dbf_count) before either kernel is launched; neither reads anything back.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dbsnpdev_core.h"

#define BSC_DBF_BLOCK 256

__global__ __launch_bounds__(BSC_DBF_BLOCK) void bsc_dbsnp_flags_kernel(const bsc_dbsnp_flat f, const uint32_t x0, const uint32_t n, uint8_t *__restrict__ out,
                                                                        const uint32_t head, const uint32_t n_vec) {
  const uint32_t edge = n - 16u * n_vec; /* head + tail, < 32 */
  const uint32_t items = n_vec + edge;
  for (uint32_t i = blockIdx.x * BSC_DBF_BLOCK + threadIdx.x; i < items; i += gridDim.x * BSC_DBF_BLOCK) {
    if (i < n_vec) {
      const uint32_t k = head + 16u * i; /* k + 15 < n */
      uint64_t m, q;
      bsc_dbf_window(&f, (uint64_t)x0 + k, &m, &q);
      uint4 v;
      v.x = bsc_dbf_flags4((unsigned)m & 15u, (unsigned)q & 15u);
      v.y = bsc_dbf_flags4((unsigned)(m >> 4) & 15u, (unsigned)(q >> 4) & 15u);
      v.z = bsc_dbf_flags4((unsigned)(m >> 8) & 15u, (unsigned)(q >> 8) & 15u);
      v.w = bsc_dbf_flags4((unsigned)(m >> 12) & 15u, (unsigned)(q >> 12) & 15u);
      *reinterpret_cast<uint4 *>(out + k) = v; /* out + head is 16-byte aligned */
    } else {
      const uint32_t j = i - n_vec;                                 /* < edge */
      const uint32_t k = j < head ? j : head + 16u * n_vec + (j - head); /* < n */
      out[k] = (uint8_t)bsc_dbf_flag(&f, (uint64_t)x0 + k);
    }
  }
}

__global__ __launch_bounds__(BSC_DBF_BLOCK) void bsc_dbsnp_names_kernel(const bsc_dbsnp_flat f, const uint32_t e0, const uint32_t n_names, uint32_t *__restrict__ pos,
                                                                        uint32_t *__restrict__ off, char *__restrict__ bytes) {
  const uint32_t t0 = f.txt[e0];
  for (uint32_t k = blockIdx.x * BSC_DBF_BLOCK + threadIdx.x; k <= n_names; k += gridDim.x * BSC_DBF_BLOCK) {
    const uint32_t o = f.txt[e0 + k] - t0; /* e0 + n_names <= n_entries: txt has n_entries + 1 words */
    off[k] = o;
    if (k < n_names) {
      pos[k] = bsc_dbf_entry_pos(&f, e0 + k);
      bsc_dbf_entry_name(&f, e0 + k, bytes + o);
    }
  }
}

static unsigned bsc_dbf_grid(uint32_t items, int num_cus) {
  unsigned grid = (items + BSC_DBF_BLOCK - 1u) / BSC_DBF_BLOCK;
  const unsigned cap = (unsigned)(num_cus > 0 ? num_cus : 256) * 8u;
  return grid > cap ? cap : (grid ? grid : 1u);
}

/* d_out: n bytes, any alignment */
extern "C" int bsc_dev_launch_dbsnp_flags(const bsc_dbsnp_flat *f, uint32_t x0, uint32_t n, void *d_out, int num_cus, void *stream) {
  if (!n) return 0;
  uint32_t head = (uint32_t)((16u - ((uintptr_t)d_out & 15u)) & 15u);
  if (head > n) head = n;
  const uint32_t n_vec = (n - head) / 16u;
  hipLaunchKernelGGL(bsc_dbsnp_flags_kernel, dim3(bsc_dbf_grid(n_vec + (n - 16u * n_vec), num_cus)), dim3(BSC_DBF_BLOCK), 0, (hipStream_t)stream, *f, x0, n,
                     (uint8_t *)d_out, head, n_vec);
  return (int)hipGetLastError();
}

/* the entries e0 .. e0 + n_names - 1 (bsc_dbf_count): d_pos n_names words, d_off n_names + 1 words, d_bytes the range's name bytes */
extern "C" int bsc_dev_launch_dbsnp_names(const bsc_dbsnp_flat *f, uint32_t e0, uint32_t n_names, void *d_pos, void *d_off, void *d_bytes, int num_cus,
                                          void *stream) {
  hipLaunchKernelGGL(bsc_dbsnp_names_kernel, dim3(bsc_dbf_grid(n_names + 1u, num_cus)), dim3(BSC_DBF_BLOCK), 0, (hipStream_t)stream, *f, e0, n_names,
                     (uint32_t *)d_pos, (uint32_t *)d_off, (char *)d_bytes);
  return (int)hipGetLastError();
}
