/*
 * fmtg_dev.h — printf("%g", (double)f) for a float, in integer arithmetic, for device code (and, the same text, for a host
 * compiler: every function is __host__ __device__ under hipcc and plain C++ elsewhere).  The VCF text encoder (vcftextdev.hip)
 * prints FORMAT GL with it and bsc_fmt_g_device probes it value by value; the checker is the C library's own snprintf
 * (bsc_fmt_g).
 *
 * The contract is glibc's: six significant digits, correctly rounded from the exact binary value, ties to even; fixed notation
 * when the decimal exponent X of the ROUNDED value has -4 <= X < 6, d.ddddde+XX otherwise; trailing zeros and a bare point
 * removed; "0" / "-0", "inf" / "-inf", "nan" / "-nan" by the sign bit.  At most 12 characters.
 *
 * How.  f = m * 2^e (m < 2^24, -149 <= e <= 104).  With b = floor(log2 f), Xe = floor(b * log10 2) is X or X - 1, so
 * T = f * 10^(5 - Xe) lies in [10^5, 2 * 10^6): its integer part I and how its fraction compares with 1/2 are all that
 * rounding needs, and both come out of exact integers — no division or logarithm whose last bit would decide a digit:
 *   k = 5 - Xe >= 0 (f < 10^6):  T = m * 5^k / 2^s, s = -(e + k).  5^k is exact in 128 bits up to k = 55 (the smallest
 *       subnormal needs k = 50).  k <= 17: the product fits 64 bits (5^17 < 2^40) — one multiply and a shift: every value
 *       of 1e-12 .. 1e6, which is where log10 likelihoods live.  Beyond: a 152-bit product in three words.
 *   k < 0 (f >= 10^6), j = -k <= 33:  T = (m * 2^(e - j)) / 5^j: numerator and denominator fit 128 bits; 24 steps of
 *       restoring division give I and the remainder, 2 * remainder against 5^j gives the comparison.
 * I >= 10^6 means X = Xe + 1: the last digit of I joins the fraction (exactly: digit > 5, < 5, or = 5 and the old fraction
 * zero or not).  Then round half to even; a carry to 10^6 makes it 10^5 with X + 1 — the notation is chosen AFTER that
 * (999999.5f prints 1e+06).
 */
#ifndef BSC_FMTG_DEV_H
#define BSC_FMTG_DEV_H
#include <stdint.h>

#if defined(__HIPCC__)
#define FMTG_FN __host__ __device__ inline
#else
#define FMTG_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define FMTG_TABLE static __device__ const
#else
#define FMTG_TABLE static const
#endif

/* 5^k, k = 0 .. 55, low and high 64 bits */
FMTG_TABLE uint64_t FMTG_POW5[56][2] = {
    {0x0000000000000001ull, 0x0000000000000000ull}, {0x0000000000000005ull, 0x0000000000000000ull}, {0x0000000000000019ull, 0x0000000000000000ull},
    {0x000000000000007dull, 0x0000000000000000ull}, {0x0000000000000271ull, 0x0000000000000000ull}, {0x0000000000000c35ull, 0x0000000000000000ull},
    {0x0000000000003d09ull, 0x0000000000000000ull}, {0x000000000001312dull, 0x0000000000000000ull}, {0x000000000005f5e1ull, 0x0000000000000000ull},
    {0x00000000001dcd65ull, 0x0000000000000000ull}, {0x00000000009502f9ull, 0x0000000000000000ull}, {0x0000000002e90eddull, 0x0000000000000000ull},
    {0x000000000e8d4a51ull, 0x0000000000000000ull}, {0x0000000048c27395ull, 0x0000000000000000ull}, {0x000000016bcc41e9ull, 0x0000000000000000ull},
    {0x000000071afd498dull, 0x0000000000000000ull}, {0x0000002386f26fc1ull, 0x0000000000000000ull}, {0x000000b1a2bc2ec5ull, 0x0000000000000000ull},
    {0x000003782dace9d9ull, 0x0000000000000000ull}, {0x00001158e460913dull, 0x0000000000000000ull}, {0x000056bc75e2d631ull, 0x0000000000000000ull},
    {0x0001b1ae4d6e2ef5ull, 0x0000000000000000ull}, {0x000878678326eac9ull, 0x0000000000000000ull}, {0x002a5a058fc295edull, 0x0000000000000000ull},
    {0x00d3c21bcecceda1ull, 0x0000000000000000ull}, {0x0422ca8b0a00a425ull, 0x0000000000000000ull}, {0x14adf4b7320334b9ull, 0x0000000000000000ull},
    {0x6765c793fa10079dull, 0x0000000000000000ull}, {0x04fce5e3e2502611ull, 0x0000000000000002ull}, {0x18f07d736b90be55ull, 0x000000000000000aull},
    {0x7cb2734119d3b7a9ull, 0x0000000000000032ull}, {0x6f7c40458122964dull, 0x00000000000000fcull}, {0x2d6d415b85acef81ull, 0x00000000000004eeull},
    {0xe32246c99c60ad85ull, 0x00000000000018a6ull}, {0x6fab61f00de36399ull, 0x0000000000007b42ull}, {0x2e58e9b04570f1fdull, 0x000000000002684cull},
    {0xe7bc90715b34b9f1ull, 0x00000000000c097cull}, {0x86aed236c807a1b5ull, 0x00000000003c2f70ull}, {0xa16a1b11e8262889ull, 0x00000000012ced32ull},
    {0x2712875988becaadull, 0x0000000005e0a1fdull}, {0xc35ca4bfabb9f561ull, 0x000000001d6329f1ull}, {0xd0cf37be5aa1cae5ull, 0x0000000092efd1b8ull},
    {0x140c16b7c528f679ull, 0x00000002deaf189cull}, {0x643c7196d9ccd05dull, 0x0000000e596b7b0cull}, {0xf52e37f2410011d1ull, 0x00000047bf19673dull},
    {0xc9e717bb45005915ull, 0x00000166bb7f0435ull}, {0xf18376a85901bd69ull, 0x00000701a97b150cull}, {0xb7915149bd08b30dull, 0x000023084f676940ull},
    {0x95d69670b12b7f41ull, 0x0000af298d050e43ull}, {0xed30f03375d97c45ull, 0x00036bcfc1194751ull}, {0xa1f4b1014d3f6d59ull, 0x00111b0ec57e6499ull},
    {0x29c77506823d22bdull, 0x00558749db77f700ull}, {0xd0e549208b31adb1ull, 0x01aba4714957d300ull}, {0x147a6da2b7f86475ull, 0x085a36366eb71f04ull},
    {0x6664242d97d9f649ull, 0x29c30f1029939b14ull}, {0xfff4b4e3f741cf6dull, 0xd0cf4b50cfe20765ull}};

/* up to 16 characters, the first in the lowest byte of lo; bytes behind the n-th are 0 */
struct fmtg_str {
  uint64_t lo, hi;
  uint32_t n;
};

/* appends the low n (<= 8) bytes of chars, which must be 0 above them */
FMTG_FN void fmtg_cat(fmtg_str &s, uint64_t chars, unsigned n) {
  if (!n) return;
  const unsigned p = s.n;
  if (p < 8u) {
    s.lo |= chars << (8u * p);
    if (p + n > 8u) s.hi |= chars >> (8u * (8u - p)); /* (p >= 1 here) */
  } else
    s.hi |= chars << (8u * (p - 8u));
  s.n = p + n;
}

FMTG_FN uint64_t fmtg_low_bytes(uint64_t v, unsigned n) { return n >= 8u ? v : (v & ((1ull << (8u * n)) - 1ull)); }

enum { FMTG_LT = 0, FMTG_EQ = 1, FMTG_GT = 2 }; /* the fraction of T against 1/2 */

FMTG_FN fmtg_str fmtg_format(uint32_t bits) {
  fmtg_str out = {0ull, 0ull, 0u};
  if (bits >> 31) fmtg_cat(out, (uint64_t)'-', 1u);
  const uint32_t ex = (bits >> 23) & 255u, fr = bits & 0x7fffffu;
  if (ex == 255u) {
    fmtg_cat(out, fr ? ((uint64_t)'n' | (uint64_t)'a' << 8 | (uint64_t)'n' << 16) : ((uint64_t)'i' | (uint64_t)'n' << 8 | (uint64_t)'f' << 16), 3u);
    return out;
  }
  if (ex == 0u && fr == 0u) {
    fmtg_cat(out, (uint64_t)'0', 1u);
    return out;
  }
  const uint32_t m = ex ? (fr | 0x800000u) : fr;
  const int e = ex ? (int)ex - 150 : -149;
  const int b = (31 - __builtin_clz(m)) + e;        /* floor(log2 f) */
  const int xe = (b * 78913) >> 18;                 /* floor(b * log10 2) for |b| <= 1650 (arithmetic shift) */
  const int k = 5 - xe;
  uint32_t I;
  int cmp;
  bool nz; /* the fraction is not 0 */
  if (k >= 0 && k <= 17) {
    const uint64_t P = (uint64_t)m * FMTG_POW5[k][0];
    const int s = -(e + k);
    if (s <= 0) {
      I = (uint32_t)(P << (unsigned)(-s));
      cmp = FMTG_LT;
      nz = false;
    } else {
      I = (uint32_t)(P >> (unsigned)s);
      const uint64_t rem = P & ((1ull << (unsigned)s) - 1ull), half = 1ull << (unsigned)(s - 1);
      cmp = rem > half ? FMTG_GT : (rem == half ? FMTG_EQ : FMTG_LT);
      nz = rem != 0ull;
    }
  } else if (k >= 0) { /* below 1e-12: m * 5^k in three words, shifted right by s (s > 20 here) */
    const unsigned __int128 a = (unsigned __int128)FMTG_POW5[k][0] * m;
    const unsigned __int128 c = (unsigned __int128)FMTG_POW5[k][1] * m + (uint64_t)(a >> 64);
    const uint64_t w0 = (uint64_t)a, w1 = (uint64_t)c, w2 = (uint64_t)(c >> 64);
    const unsigned s = (unsigned)(-(e + k));
    {
      const unsigned ws = s >> 6, bs = s & 63u;
      const uint64_t x0 = ws == 0u ? w0 : (ws == 1u ? w1 : w2), x1 = ws == 0u ? w1 : (ws == 1u ? w2 : 0ull);
      I = (uint32_t)(bs ? (x0 >> bs | x1 << (64u - bs)) : x0);
    }
    const unsigned p = s - 1u, wp = p >> 6, bp = p & 63u;
    const uint64_t xp = wp == 0u ? w0 : (wp == 1u ? w1 : w2);
    const bool half_bit = (xp >> bp) & 1ull;
    const bool below = (xp & ((1ull << bp) - 1ull)) != 0ull || (wp >= 1u && w0 != 0ull) || (wp >= 2u && w1 != 0ull);
    cmp = half_bit ? (below ? FMTG_GT : FMTG_EQ) : FMTG_LT;
    nz = half_bit || below;
  } else { /* 1e6 and above: (m * 2^(e - j)) / 5^j */
    const int j = -k, t = e - j;
    unsigned __int128 A = (unsigned __int128)m << (unsigned)(t > 0 ? t : 0);
    const unsigned __int128 den = ((unsigned __int128)FMTG_POW5[j][1] << 64 | FMTG_POW5[j][0]) << (unsigned)(t < 0 ? -t : 0);
    uint32_t q = 0u;
    for (int i = 23; i >= 0; i--) {
      const unsigned __int128 d = den << (unsigned)i; /* < 2^107 */
      if (d <= A) {
        A -= d;
        q |= 1u << i;
      }
    }
    I = q;
    const unsigned __int128 twice = A << 1;
    cmp = twice > den ? FMTG_GT : (twice == den ? FMTG_EQ : FMTG_LT);
    nz = A != 0;
  }
  int X = xe;
  if (I >= 1000000u) { /* X = Xe + 1: the last digit joins the fraction */
    const uint32_t r = I % 10u;
    I /= 10u;
    X++;
    cmp = r > 5u ? FMTG_GT : (r < 5u ? FMTG_LT : (nz ? FMTG_GT : FMTG_EQ));
  }
  if (cmp == FMTG_GT || (cmp == FMTG_EQ && (I & 1u))) I++; /* half to even */
  if (I == 1000000u) {
    I = 100000u;
    X++;
  }
  /* six digits, the first in the lowest byte; nd = how many are left without the trailing zeros */
  uint64_t dig = 0ull;
  unsigned nd = 6u;
  {
    bool tail = true;
    uint32_t v = I;
    for (int i = 0; i < 6; i++) {
      const uint32_t d = v % 10u;
      v /= 10u;
      dig = dig << 8 | (uint64_t)('0' + d);
      if (tail && d == 0u && i < 5) nd--;
      else tail = false;
    }
  }
  if (X < -4 || X >= 6) {
    uint64_t body = dig & 0xffull;
    if (nd > 1u) body |= (uint64_t)'.' << 8 | fmtg_low_bytes(dig >> 8, nd - 1u) << 16;
    fmtg_cat(out, body, nd > 1u ? nd + 1u : 1u);
    const unsigned ax = (unsigned)(X < 0 ? -X : X); /* <= 45 */
    fmtg_cat(out, (uint64_t)'e' | (uint64_t)(X < 0 ? '-' : '+') << 8 | (uint64_t)('0' + ax / 10u) << 16 | (uint64_t)('0' + ax % 10u) << 24, 4u);
  } else if (X >= 0) {
    const unsigned ni = (unsigned)X + 1u; /* digits before the point: 1 .. 6 */
    fmtg_cat(out, fmtg_low_bytes(dig, ni), ni);
    if (nd > ni) fmtg_cat(out, (uint64_t)'.' | fmtg_low_bytes(dig >> (8u * ni), nd - ni) << 8, nd - ni + 1u);
  } else {
    const unsigned nz0 = (unsigned)(-X) + 1u; /* "0." and -X - 1 zeros: 2 .. 5 characters */
    fmtg_cat(out, fmtg_low_bytes(0x303030302e30ull, nz0), nz0);
    fmtg_cat(out, fmtg_low_bytes(dig, nd), nd);
  }
  return out;
}

#endif
