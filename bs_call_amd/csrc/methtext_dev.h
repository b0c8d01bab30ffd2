/*
 * methtext_dev.h — the text forms of a bedMethyl line on the device, shared by the per-cytosine table's encoder (methdev.hip) and the
 * bigBed item encoder (bigbeddev.hip): the two sinks an emitter runs over (one counts, one writes), the decimal conversion, the
 * percentage, and columns 4 .. 15 of the line (include/bscall_amd.h has the columns).  All arithmetic is integer: the decimal
 * conversion divides by constants, the percentage is found by bisection over 0 .. 100 (a 64-bit division by a variable would be
 * expanded through a floating-point reciprocal).  Device code only.
 */
#ifndef BSC_METHTEXT_DEV_H
#define BSC_METHTEXT_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

/* what a line is made of */
struct mb_site {
  uint32_t pos, a, b;
  unsigned minus, label, flt, phred; /* label: 0 CG, 1 CHG, 2 CHH, 3 CHN */
};

struct mb_count_sink {
  unsigned len;
  __device__ __forceinline__ void u8(unsigned) { len++; }
  __device__ __forceinline__ void bytes(uint64_t, unsigned n) { len += n; }
  __device__ __forceinline__ void words(const uint32_t *, unsigned n_bytes) { len += n_bytes; }
};
struct mb_write_sink {
  uint8_t *p;
  unsigned len;
  __device__ __forceinline__ void u8(unsigned v) { p[len++] = (uint8_t)v; }
  /* the low n (<= 8) bytes of bits, the lowest first, and not one more */
  __device__ __forceinline__ void bytes(uint64_t bits, unsigned n) {
    for (unsigned k = 0; k < n; k++) p[len + k] = (uint8_t)(bits >> (8u * k));
    len += n;
  }
  /* n_bytes of w, rounded up to whole dwords: up to 3 bytes behind them are garbage until the line's next column lands on them (a
   * line goes on for 30 bytes at least behind its contig) */
  __device__ __forceinline__ void words(const uint32_t *w, unsigned n_bytes) {
    for (unsigned k = 0u; 4u * k < n_bytes; k++) __builtin_memcpy(p + len + 4u * k, &w[k], 4);
    len += n_bytes;
  }
};

/* v < 10^8 in decimal, the first digit in the lowest byte */
__device__ __forceinline__ uint64_t mb_dec8(uint32_t v, unsigned &n) {
  uint64_t acc = 0ull;
  n = 0u;
  do {
    const uint32_t q = v / 10u;
    acc = acc << 8 | (uint64_t)('0' + (v - q * 10u));
    v = q;
    n++;
  } while (v);
  return acc;
}

/* v < 10^16 in decimal and sep behind it */
template <class S>
__device__ __forceinline__ void mb_put_dec(S &s, uint64_t v, unsigned sep) {
  unsigned n;
  if (v >= 100000000ull) {
    const uint64_t top = v / 100000000ull;
    uint32_t low = (uint32_t)(v - top * 100000000ull);
    const uint64_t c = mb_dec8((uint32_t)top, n);
    s.bytes(c, n);
    uint64_t acc = 0ull;
    for (int i = 0; i < 8; i++) {
      const uint32_t q = low / 10u;
      acc = acc << 8 | (uint64_t)('0' + (low - q * 10u));
      low = q;
    }
    s.bytes(acc, 8u);
  } else {
    const uint64_t c = mb_dec8((uint32_t)v, n);
    s.bytes(c, n);
  }
  s.u8(sep);
}

/* (200 a + n) / (2 n), n = a + b > 0: the largest q of 0 .. 100 with 2 n q <= 200 a + n */
__device__ __forceinline__ unsigned mb_pct(uint64_t a, uint64_t n) {
  const uint64_t num = 200ull * a + n, den = 2ull * n;
  unsigned lo = 0u, hi = 100u;
  while (lo < hi) {
    const unsigned mid = (lo + hi + 1u) >> 1;
    if (den * mid <= num) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

#define MB_STR4(a, b, c, d) ((uint64_t)(a) | (uint64_t)(b) << 8 | (uint64_t)(c) << 16 | (uint64_t)(d) << 24)

/* columns 4 .. 15 of the site's line — name, score, strand, thickStart, thickEnd, itemRgb, coverage, pct, a, b, GQ, FILTER — with the
 * tabs between them, and LAST behind the FILTER: '\n' in the table, NUL in a bigBed item (a template argument: a constant in
 * either encoder).  start = m.pos - 1, cov = m.a + m.b, pct = mb_pct(m.a, cov): the caller has them */
template <unsigned LAST, class S>
__device__ __forceinline__ void mb_emit_cols(S &s, const mb_site &m, uint32_t start, uint64_t cov, unsigned pct) {
  if (m.label == 0u) s.bytes(MB_STR4('C', 'G', '\t', 0), 3u);
  else s.bytes(MB_STR4('C', 'H', m.label == 1u ? 'G' : (m.label == 2u ? 'H' : 'N'), '\t'), 4u);
  mb_put_dec(s, cov < 1000ull ? cov : 1000ull, '\t');
  s.bytes((uint64_t)(m.minus ? '-' : '+') | (uint64_t)'\t' << 8, 2u);
  mb_put_dec(s, start, '\t');
  mb_put_dec(s, m.pos, '\t');
  { /* itemRgb: green up to 50 %, red from there */
    const unsigned k = pct / 10u;
    const unsigned r = k < 5u ? (k ? 5u + 50u * k : 0u) : 255u, g = k <= 5u ? 255u : (k < 10u ? 5u + 50u * (10u - k) : 0u);
    mb_put_dec(s, r, ',');
    mb_put_dec(s, g, ',');
    s.bytes((uint64_t)'0' | (uint64_t)'\t' << 8, 2u);
  }
  mb_put_dec(s, cov, '\t');
  mb_put_dec(s, pct, '\t');
  mb_put_dec(s, m.a, '\t');
  mb_put_dec(s, m.b, '\t');
  mb_put_dec(s, m.phred, '\t');
  s.bytes((m.flt == 0u ? MB_STR4('P', 'A', 'S', 'S') : ((m.flt & 128u) ? MB_STR4('m', 'a', 'c', '1') : MB_STR4('f', 'a', 'i', 'l'))) | (uint64_t)LAST << 32, 5u);
}

#endif
