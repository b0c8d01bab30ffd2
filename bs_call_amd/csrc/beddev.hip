/*
 * beddev.hip — what a tabix / CSI index needs of a block's methylation table (BED text), made where the table lies: the runs of consecutive
 * lines that share their windows (start >> min_shift, (end - 1) >> min_shift), each with its line count and the offset of its first line.
 * The twin of csidev.hip: the table is cut into intervals at line starts — the tile offsets the table encoders leave (methdev.hip: tile_off)
 * — and a lane walks one interval (bedidx_core.h: bed_walk).
 *
 *   bsc_bed_count_kernel   runs per interval -> cnt[i]; the lines walked (a wave-level sum, then one atomic per workgroup:
 *                          rs_flush_counts) -> totals[1]; the error bits -> totals[2]
 *   (exclusive scan)       cnt -> off (sort.hip), off[n_sync] the number of runs
 *   bsc_bed_write_kernel   the same walk, run k of interval i -> entries[off[i] + k] while that is below the capacity;
 *                          totals[0] = off[n_sync], whether the runs fitted or not
 *
 * The entries are in stream order whatever the launch geometry: a lane's slots come from the scan, not from the order the workgroups
 * arrive in.  A run that continues across an interval boundary comes out as adjacent entries with the same windows — one per interval it
 * touches; bsc_tbx_add joins their extents.  An empty interval writes nothing.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bedidx_core.h"
#include "recstream_dev.h"

#define BSC_BED_BLOCK 256

__device__ __forceinline__ bool bed_interval(const unsigned long long *__restrict__ sync, uint32_t i, uint64_t n_bytes, uint64_t &beg, uint64_t &end) {
  beg = sync ? sync[i] : 0ull;
  end = sync ? sync[i + 1u] : n_bytes;
  return beg <= end && end <= n_bytes;
}

__global__ __launch_bounds__(BSC_BED_BLOCK) void bsc_bed_count_kernel(const uint8_t *__restrict__ s, const uint64_t n_bytes, const unsigned long long *__restrict__ sync,
                                                                      const uint32_t n_sync, const int min_shift, unsigned long long *__restrict__ cnt,
                                                                      unsigned long long *__restrict__ totals) {
  uint32_t n_lines = 0, err = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[n_sync] = 0ull;
  for (uint32_t i = blockIdx.x * BSC_BED_BLOCK + threadIdx.x; i < n_sync; i += gridDim.x * BSC_BED_BLOCK) {
    uint64_t beg, end;
    uint32_t runs = 0;
    if (bed_interval(sync, i, n_bytes, beg, end)) runs = bed_walk(s, beg, end, min_shift, nullptr, 0, 0, &n_lines, &err);
    else err |= BED_ERR_INTERVAL;
    cnt[i] = runs;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    n_lines += __shfl_xor(n_lines, d);
    err |= __shfl_xor(err, d);
  }
  const unsigned c[1] = {n_lines};
  rs_flush_counts(c, totals + 1);
  if (err && (threadIdx.x & 63u) == 0) atomicOr(totals + 2, (unsigned long long)err);
}

__global__ __launch_bounds__(BSC_BED_BLOCK) void bsc_bed_write_kernel(const uint8_t *__restrict__ s, const uint64_t n_bytes, const unsigned long long *__restrict__ sync,
                                                                      const uint32_t n_sync, const int min_shift, const unsigned long long *__restrict__ off,
                                                                      bed_run *__restrict__ entries, const uint64_t cap, unsigned long long *__restrict__ totals) {
  if (blockIdx.x == 0 && threadIdx.x == 0) totals[0] = off[n_sync];
  for (uint32_t i = blockIdx.x * BSC_BED_BLOCK + threadIdx.x; i < n_sync; i += gridDim.x * BSC_BED_BLOCK) {
    uint64_t beg, end;
    uint32_t n_lines = 0, err = 0;
    if (off[i + 1u] == off[i] || !bed_interval(sync, i, n_bytes, beg, end)) continue; /* no run: an empty or a refused interval */
    bed_walk(s, beg, end, min_shift, entries, off[i], cap, &n_lines, &err);
  }
}

/*
 * s[0, n_bytes): the table; sync[n_sync + 1] ascending line starts with sync[0] = 0 and sync[n_sync] = n_bytes, or NULL with n_sync = 1: one
 * interval; cnt / off: n_sync + 1 u64 each; scan_tmp: bsc_dev_scan_tmp_bytes_u64(n_sync + 1); entries[cap]; totals: u64 {runs, lines, error
 * bits}, zeroed by the caller.
 */
extern "C" int bsc_dev_scan_u64(const void *in, void *out, uint32_t n, void *tmp, size_t tmp_bytes, void *stream); /* sort.hip */
extern "C" int bsc_dev_launch_bed_scan(const void *s, uint64_t n_bytes, const void *sync, uint32_t n_sync, int min_shift, void *cnt, void *off, void *scan_tmp,
                                       size_t scan_tmp_bytes, void *entries, uint64_t cap, void *totals, int num_cus, void *stream) {
  if (!n_sync) return 0;
  hipStream_t st = (hipStream_t)stream;
  unsigned grid = (n_sync + BSC_BED_BLOCK - 1u) / BSC_BED_BLOCK;
  const unsigned most = (unsigned)(num_cus > 0 ? num_cus : 256) * 8u;
  if (grid > most) grid = most;
  hipLaunchKernelGGL(bsc_bed_count_kernel, dim3(grid), dim3(BSC_BED_BLOCK), 0, st, (const uint8_t *)s, n_bytes, (const unsigned long long *)sync, n_sync, min_shift,
                     (unsigned long long *)cnt, (unsigned long long *)totals);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int rc = bsc_dev_scan_u64(cnt, off, n_sync + 1u, scan_tmp, scan_tmp_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(bsc_bed_write_kernel, dim3(grid), dim3(BSC_BED_BLOCK), 0, st, (const uint8_t *)s, n_bytes, (const unsigned long long *)sync, n_sync, min_shift,
                     (const unsigned long long *)off, (bed_run *)entries, cap, (unsigned long long *)totals);
  return (int)hipGetLastError();
}
