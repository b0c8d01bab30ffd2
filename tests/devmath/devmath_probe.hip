/*
 * devmath_probe.hip — TEST ONLY (tests/test_gpu_devmath.py): the device numeric primitives of the calling and statistics
 * kernels, one call per lane, on inputs the test chooses lane by lane.  The product headers are included unchanged, so
 * what runs here is the product's own text compiled with the product's flags (Makefile: devmath-probe); nothing of it
 * is part of libbscall_amd.so.
 *
 * Layout: case i (inputs in[i * k .. i * k + k), outputs out[i * m .. i * m + m)) is lane i % 64 of wave i / 64, in
 * 256-thread blocks, so the test decides which values share a wave.  n must be a multiple of 64: every lane of a wave
 * is a case, none is filler that could change a wave-uniform branch.  The exception is DM_SS_POSTERIOR, a whole-wave
 * operation: there case i is wave i (inputs a, b; outputs the 101 bins) and n may be anything.
 *
 * The tables sit in LDS as the product kernels keep them (kernels.hip, sitestats.hip): the double2 / ulonglong2 table
 * reads of log_main / exp_mid / exp_term_dev are LDS reads here too.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsmath.h"
#include "callmath.h"
#include "sitestats_dev.h"

enum {
  DM_LOG_DEV = 0,      /* log_dev(x)                                        k 1  m 1 */
  DM_LOG_MAIN = 1,     /* log_main(x): positive normal finite x only         k 1  m 1 */
  DM_LOG_NEAR1 = 2,    /* log_near1(x): 1 - 2^-4 <= x < 1 + 0x1.09p-4 only    k 1  m 1 */
  DM_BSM_LOG = 3,      /* bsm_log_t(x) on the device                         k 1  m 1 */
  DM_EXP_DEV = 4,      /* exp_dev(x)                                         k 1  m 1 */
  DM_EXP_MID = 5,      /* exp_mid(x): x == 0 or 2^-54 <= |x| < 512 only       k 1  m 1 */
  DM_BSM_EXP = 6,      /* bsm_exp_t(x) on the device                         k 1  m 1 */
  DM_EXP_TERM = 7,     /* exp_term_dev(x)                                    k 1  m 1 */
  DM_NORM_TAIL = 8,    /* ll - max -> gt_prob as call_body.inc composes it    k 10 m 10 */
  DM_DIV_LN10 = 9,     /* div_ln10_dev(x)                                    k 1  m 1 */
  DM_GET_Z = 10,       /* get_Z(x1, x2, k1, k2, l, t) -> Z0, Z1, Z2           k 6  m 3 */
  DM_PURE_LOG = 11,    /* pure_log_entry(idx, l, t) over kq[]                k 3  m 1 */
  DM_LFACT = 12,       /* lfact_dev(n)                                       k 1  m 1 */
  DM_SS_LFACT = 13,    /* ss_lfact(n)                                        k 1  m 1 */
  DM_FISHER = 14,      /* fisher_dev(c0, c1, c2, c3)                         k 4  m 1 */
  DM_STRAND = 15,      /* strand_table(mxi, f[8], r[8]) -> t0..t3            k 17 m 4 */
  DM_SS_POSTERIOR = 16, /* ss_posterior(a, b): one case per WAVE             k 2  m 101 */
  DM_COUNT = 17
};

/* doubles per case in and out */
__host__ __device__ constexpr int dm_k(int fn) {
  return fn == DM_NORM_TAIL ? 10 : fn == DM_GET_Z ? 6 : fn == DM_PURE_LOG ? 3 : fn == DM_FISHER ? 4 : fn == DM_STRAND ? 17
       : fn == DM_SS_POSTERIOR ? 2 : 1;
}
__host__ __device__ constexpr int dm_m(int fn) {
  return fn == DM_NORM_TAIL ? 10 : fn == DM_GET_Z ? 3 : fn == DM_STRAND ? 4 : fn == DM_SS_POSTERIOR ? 101 : 1;
}

#define DM_THREADS 256

template <int FN>
__global__ __launch_bounds__(DM_THREADS) void dm_kernel(const double *__restrict__ in, double *__restrict__ out, uint64_t n,
                                                        const double *__restrict__ lfact, const double *__restrict__ logp,
                                                        const double *__restrict__ kq, const double *__restrict__ logtab,
                                                        const unsigned long long *__restrict__ exptab) {
  __shared__ double s_logtab[256];
  __shared__ unsigned long long s_exptab[256];
  __shared__ double s_lf[256];
  __shared__ double s_logp[100];
  __shared__ double s_k[44];
  const unsigned tid = threadIdx.x;
  for (unsigned i = tid; i < 256; i += DM_THREADS) {
    s_logtab[i] = logtab[i];
    s_exptab[i] = exptab[i];
    s_lf[i] = lfact[i];
  }
  if (tid < 100) s_logp[tid] = logp[tid];
  if (tid < 44) s_k[tid] = kq[tid];
  __syncthreads();
  const uint64_t gid = (uint64_t)blockIdx.x * DM_THREADS + tid;
  const uint64_t wave = gid >> 6;
  const unsigned lane = tid & 63u;

  if (FN == DM_SS_POSTERIOR) {
    if (wave >= n) return; /* whole waves: the branch is wave-uniform */
    const uint32_t a = (uint32_t)in[wave * 2], b = (uint32_t)in[wave * 2 + 1];
    double z[2];
    ss_posterior(a, b, lane, s_lf, s_logtab, s_logp, s_exptab, z);
    out[wave * 101 + lane] = z[0];
    if (lane + 64u < 101u) out[wave * 101 + lane + 64u] = z[1];
    return;
  }
  if (wave >= n / 64) return; /* n is a multiple of 64 (checked on the host): whole waves again */
  const double *x = in + gid * dm_k(FN);
  double *y = out + gid * dm_m(FN);
  const double *lt = s_logtab;
  const uint64_t *et = (const uint64_t *)s_exptab;
  switch (FN) {
    case DM_LOG_DEV: y[0] = log_dev(x[0], lt); break;
    case DM_LOG_MAIN: y[0] = log_main(x[0], lt); break;
    case DM_LOG_NEAR1: y[0] = log_near1(x[0]); break;
    case DM_BSM_LOG: y[0] = bsm_log_t(x[0], lt); break;
    case DM_EXP_DEV: y[0] = exp_dev(x[0], et); break;
    case DM_EXP_MID: y[0] = exp_mid(x[0], et); break;
    case DM_BSM_EXP: y[0] = bsm_exp_t(x[0], et); break;
    case DM_EXP_TERM: y[0] = exp_term_dev(x[0], et); break;
    case DM_NORM_TAIL: { /* call_body.inc, the register form of the normalisation: index-order sum, log, quotients */
      double la[10];
#pragma unroll
      for (int g = 0; g < 10; g++) la[g] = x[g];
      double sum = 0.0;
#pragma unroll 1
      for (int g = 0; g < 10; g++) sum += exp_term_dev(la[g], et);
      const double lsum = log_dev(sum, lt);
#pragma unroll 1
      for (int g = 0; g < 10; g++) la[g] = div_ln10_dev(la[g] - lsum);
#pragma unroll
      for (int g = 0; g < 10; g++) y[g] = la[g];
      break;
    }
    case DM_DIV_LN10: y[0] = div_ln10_dev(x[0]); break;
    case DM_GET_Z: {
      double z0, z1, z2;
      get_Z(x[0], x[1], x[2], x[3], x[4], x[5], z0, z1, z2);
      y[0] = z0;
      y[1] = z1;
      y[2] = z2;
      break;
    }
    case DM_PURE_LOG: y[0] = pure_log_entry((unsigned)x[0], x[1], x[2], s_k, lt); break;
    case DM_LFACT: y[0] = lfact_dev((int)x[0], s_lf, lt); break;
    case DM_SS_LFACT: y[0] = ss_lfact((int)x[0], s_lf, lt); break;
    case DM_FISHER: y[0] = fisher_dev((int)x[0], (int)x[1], (int)x[2], (int)x[3], s_lf, lt, et); break;
    case DM_STRAND: {
      uint32_t f[8], r[8];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        f[j] = (uint32_t)x[1 + j];
        r[j] = (uint32_t)x[9 + j];
      }
      int t0, t1, t2, t3;
      strand_table((unsigned)x[0], f, r, t0, t1, t2, t3);
      y[0] = t0;
      y[1] = t1;
      y[2] = t2;
      y[3] = t3;
      break;
    }
    default: break;
  }
}

template <int FN>
static void dm_launch(unsigned blocks, const double *in, double *out, uint64_t n, const double *lf, const double *lp, const double *kq,
                      const double *lt, const unsigned long long *et) {
  dm_kernel<FN><<<blocks, DM_THREADS>>>(in, out, n, lf, lp, kq, lt, et);
}

typedef void (*dm_launcher)(unsigned, const double *, double *, uint64_t, const double *, const double *, const double *,
                            const double *, const unsigned long long *);
static const dm_launcher dm_launchers[DM_COUNT] = {
    dm_launch<0>,  dm_launch<1>,  dm_launch<2>,  dm_launch<3>,  dm_launch<4>,  dm_launch<5>,  dm_launch<6>,  dm_launch<7>, dm_launch<8>,
    dm_launch<9>, dm_launch<10>, dm_launch<11>, dm_launch<12>, dm_launch<13>, dm_launch<14>, dm_launch<15>, dm_launch<16>};

/* doubles in / out per case of fn, or 0 for an unknown fn */
extern "C" int devmath_probe_shape(int fn, int *k, int *m) {
  if (fn < 0 || fn >= DM_COUNT) return 0;
  *k = dm_k(fn);
  *m = dm_m(fn);
  return 1;
}

/*
 * Runs fn over n cases: in (host, n x k doubles) -> out (host, n x m doubles), with lfact[256] (lfact_store), logp[100]
 * (log(0.01 (i + 1))) and kq[44] (q_prob[q].k) as the tables the product kernels upload, and the log / exp tables of
 * bsmath_tables.h.  Allocation, copies, launch and synchronisation happen here; the first failing HIP call's status is
 * returned (hipSuccess = 0).
 */
extern "C" int devmath_probe_run(int fn, const double *in, double *out, uint64_t n, const double *lfact, const double *logp,
                                 const double *kq) {
  if (fn < 0 || fn >= DM_COUNT || !in || !out || !lfact || !logp || !kq) return (int)hipErrorInvalidValue;
  const bool per_wave = fn == DM_SS_POSTERIOR;
  if (n == 0) return (int)hipSuccess;
  if (!per_wave && n % 64u) return (int)hipErrorInvalidValue;
  const uint64_t threads = per_wave ? n * 64u : n;
  if (threads / DM_THREADS >= (1u << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((threads + DM_THREADS - 1) / DM_THREADS);
  const size_t in_b = (size_t)n * dm_k(fn) * 8, out_b = (size_t)n * dm_m(fn) * 8;
  double *d_in = nullptr, *d_out = nullptr, *d_tab = nullptr;
  hipError_t e = hipMalloc(&d_in, in_b);
  if (e == hipSuccess) e = hipMalloc(&d_out, out_b);
  /* one block of constants: lfact[256] logp[100] kq[44] log_tab[256] exp_tab[256] */
  if (e == hipSuccess) e = hipMalloc(&d_tab, (256 + 100 + 44 + 256 + 256) * 8);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0xff, out_b); /* NaN in every slot a kernel fails to write */
  if (e == hipSuccess) e = hipMemcpy(d_tab, lfact, 256 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_tab + 256, logp, 100 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_tab + 356, kq, 44 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_tab + 400, bsm_log_tab, 256 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_tab + 656, bsm_exp_tab, 256 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    dm_launchers[fn](blocks, d_in, d_out, n, d_tab, d_tab + 256, d_tab + 356, d_tab + 400, (const unsigned long long *)(d_tab + 656));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (d_tab) (void)hipFree(d_tab);
  return (int)e;
}
