/*
 * vcftext_emit.h — one packed record (bsc_vcf_rec: 32 dwords) as the VCF data line bsc_vcf_format_rec writes for it, plus '\n':
 * the emitter of vcftextdev.hip.  Statement for statement csrc/vcf_format.c (the checker), for ANY record contents:
 * gt > 9 formats as genotype 0, at most 6 GL values, "%.5s" of the context strings stops at a NUL, "%c" prints the byte
 * whatever it is, FT names the first failed filter only, AMQ only for covered classes, FS only for heterozygous calls.
 * Plain C++ without device builtins (the same text compiles for the host: that is how it was checked against the host
 * formatter on millions of random records before it ever ran on a device).
 *
 * The emitter runs over a sink that counts (the size pass) and a sink that writes (into the wave's LDS image).  The writing
 * sink composes TOKENS in registers — a number and its separator are one word — and stores whole dwords: a token of n bytes
 * writes n rounded up to 4, so up to 3 bytes behind it are garbage until the line's next token lands on them.  The line's
 * LAST tokens (CS, CG, CX, FS and the newline: at least 5 bytes) are stored exactly, so nothing is ever written behind a
 * line's end and neighbouring lanes need no ordering between them.
 *
 * Longest line: contig (<= 255) + 410:
 *   "\t" POS 10 "\t" ID 63 "\t" REF 1 "\t" ALT 3 "\t" QUAL 3 "\t" FILTER 4 "\t" "CX=" 5 "\t"          = 99
 *   "GT:FT:DP:MQ:GQ:QD:GL:MC8:AMQ:CS:CG:CX:FS" 39 "\t"                                                   = 40
 *   GT 5 ":" FT 4 ":" DP 10 ":" MQ 11 ":" GQ 3 ":" QD 10 ":" GL 6 x 12 + 5 ":" MC8 8 x 10 + 7 ":" AMQ 8 x 3 + 7 ":"
 *   CS 2 ":" CG 1 ":" CX 5 ":" FS 11 "\n"                                                                = 271
 */
#ifndef BSC_VCFTEXT_EMIT_H
#define BSC_VCFTEXT_EMIT_H
#include <stdint.h>

#include "fmtg_dev.h"
#include "recstream_dev.h"

#define VT_FN FMTG_FN
#if defined(__HIPCC__)
#define VT_MFN __host__ __device__ inline
#else
#define VT_MFN inline
#endif
#define VT_ID_MAX 63u      /* as the BCF encoder (bsc_bcf_block's rs[64]) */
#define VT_CONTIG_MAX 255u
#define VT_LINE_MAX (VT_CONTIG_MAX + 410u)

typedef rs_rec vt_rec; /* the record's fields as the emitter reads them */

struct vt_count_sink {
  unsigned len;
  VT_MFN void u8(unsigned) { len++; }
  VT_MFN void put8(uint64_t, unsigned n) { len += n; }
  VT_MFN void put16(uint64_t, uint64_t, unsigned n) { len += n; }
  VT_MFN void put_exact(uint64_t, uint64_t, unsigned n) { len += n; }
  VT_MFN void words(const uint32_t *, unsigned n_bytes) { len += n_bytes; }
};
struct vt_write_sink {
  uint8_t *p;
  unsigned len;
  VT_MFN void u8(unsigned v) { p[len++] = (uint8_t)v; }
  VT_MFN void dword(unsigned at, uint32_t v) { __builtin_memcpy(p + len + at, &v, 4); }
  /* the low n (<= 8) bytes of bits: one dword, two when n > 4 */
  VT_MFN void put8(uint64_t bits, unsigned n) {
    dword(0u, (uint32_t)bits);
    if (n > 4u) dword(4u, (uint32_t)(bits >> 32));
    len += n;
  }
  VT_MFN void put16(uint64_t lo, uint64_t hi, unsigned n) { /* n <= 16 */
    dword(0u, (uint32_t)lo);
    if (n > 4u) dword(4u, (uint32_t)(lo >> 32));
    if (n > 8u) dword(8u, (uint32_t)hi);
    if (n > 12u) dword(12u, (uint32_t)(hi >> 32));
    len += n;
  }
  /* n (<= 16) bytes and not one more: whole dwords, then the last 1 .. 3 singly */
  VT_MFN void put_exact(uint64_t lo, uint64_t hi, unsigned n) {
    unsigned k = 0u;
    for (; k + 4u <= n; k += 4u) dword(k, (uint32_t)((k < 8u ? lo : hi) >> (8u * (k & 4u))));
    for (; k < n; k++) p[len + k] = (uint8_t)((k < 8u ? lo : hi) >> (8u * (k & 7u)));
    len += n;
  }
  /* n_bytes of w, rounded up to whole dwords */
  VT_MFN void words(const uint32_t *w, unsigned n_bytes) {
    for (unsigned k = 0u; 4u * k < n_bytes; k++) dword(4u * k, w[k]);
    len += n_bytes;
  }
};

/* v < 10^8 in decimal, the first digit in the lowest byte */
VT_FN uint64_t vt_dec8(uint32_t v, unsigned &n) {
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

/* a decimal number and the separator behind it */
template <class S>
VT_FN void vt_put_dec(S &s, uint32_t v, bool neg, unsigned sep) {
  if (neg) s.put8((uint64_t)'-', 1u);
  unsigned n;
  if (v >= 100000000u) { /* 9 or 10 digits: the leading one or two, then eight */
    const uint32_t top = v / 100000000u;
    uint32_t low = v - top * 100000000u;
    const uint64_t c = vt_dec8(top, n);
    s.put8(c, n);
    uint64_t acc = 0ull;
    for (int i = 0; i < 8; i++) {
      const uint32_t q = low / 10u;
      acc = acc << 8 | (uint64_t)('0' + (low - q * 10u));
      low = q;
    }
    s.put8(acc, 8u);
    s.put8((uint64_t)sep, 1u);
    return;
  }
  const uint64_t c = vt_dec8(v, n);
  if (n < 8u)
    s.put8(c | (uint64_t)sep << (8u * n), n + 1u);
  else {
    s.put8(c, 8u);
    s.put8((uint64_t)sep, 1u);
  }
}
template <class S>
VT_FN void vt_put_int(S &s, int32_t v, unsigned sep) {
  vt_put_dec(s, v < 0 ? (uint32_t)(-(int64_t)v) : (uint32_t)v, v < 0, sep);
}

/* strnlen(five characters in the low 40 bits, 5) */
VT_FN unsigned vt_len5(uint64_t c) {
  return !(c & 0xffull) ? 0u : (!(c & 0xff00ull) ? 1u : (!(c & 0xff0000ull) ? 2u : (!(c & 0xff000000ull) ? 3u : (!(c & 0xff00000000ull) ? 4u : 5u))));
}

/* w[i] of six / eight dwords without an indexed register file (i is a loop counter that is not unrolled: one copy of the formatter) */
VT_FN uint32_t vt_pick8(const uint32_t *w, unsigned i) {
  const uint32_t a = (i & 1u) ? w[1] : w[0], b = (i & 1u) ? w[3] : w[2], c = (i & 1u) ? w[5] : w[4], d = (i & 1u) ? w[7] : w[6];
  const uint32_t ab = (i & 2u) ? b : a, cd = (i & 2u) ? d : c;
  return (i & 4u) ? cd : ab;
}

#define VT_STR4(a, b, c, d) ((uint64_t)(a) | (uint64_t)(b) << 8 | (uint64_t)(c) << 16 | (uint64_t)(d) << 24)
#define VT_STR8(a, b, c, d, e, f, g, h) (VT_STR4(a, b, c, d) | VT_STR4(e, f, g, h) << 32)

/* contig_w: the contig's name and the tab behind it, clen1 bytes.  id / id_len: the record's name, or 0.  clamped: a genotype
 * beyond 9 or more than 6 likelihoods (written as the host formatter writes them: genotype 0, six values). */
template <class S>
VT_FN void vt_emit_line(S &s, const vt_rec &r, const uint32_t *contig_w, unsigned clen1, const uint8_t *id, unsigned id_len, bool &clamped) {
  const unsigned gt_raw = r.byte(5), n_gl_raw = r.byte(10);
  clamped = gt_raw > 9u || n_gl_raw > 6u;
  const unsigned gt = gt_raw > 9u ? 0u : gt_raw, n_gl = n_gl_raw > 6u ? 6u : n_gl_raw;
  const unsigned flt = r.byte(8), phred = r.byte(9), gt_enc = r.byte(7);
  const unsigned alt0 = r.byte(12), alt1 = r.byte(13);
  const bool het = (0x16Eu >> gt) & 1u; /* AC AG AT CG CT GT */
  unsigned n_amq = 0u;
  for (int k = 0; k < 8; k++) n_amq += r.w[16 + k] > 0u ? 1u : 0u;
  /* CHROM POS ID REF */
  s.words(contig_w, clen1);
  vt_put_dec(s, r.w[0], false, '\t');
  if (id_len) {
    for (unsigned k = 0; k < id_len; k++) s.u8(id[k]);
    s.put8((uint64_t)'\t' | (uint64_t)r.byte(16) << 8 | (uint64_t)'\t' << 16, 3u);
  } else
    s.put8(VT_STR4('.', '\t', r.byte(16), '\t'), 4u);
  { /* ALT QUAL */
    uint64_t bits;
    unsigned n;
    if (alt0) {
      bits = (uint64_t)alt0;
      n = 1u;
      if (alt1) {
        bits |= (uint64_t)',' << 8 | (uint64_t)alt1 << 16;
        n = 3u;
      }
    } else {
      bits = (uint64_t)'.';
      n = 1u;
    }
    bits |= (uint64_t)'\t' << (8u * n);
    n++;
    unsigned nq;
    const uint64_t q = vt_dec8(phred, nq);
    bits |= (q | (uint64_t)'\t' << (8u * nq)) << (8u * n);
    s.put8(bits, n + nq + 1u); /* <= 8 */
  }
  /* FILTER INFO */
  s.put8((flt == 0u ? VT_STR4('P', 'A', 'S', 'S') : ((flt & 128u) ? VT_STR4('m', 'a', 'c', '1') : VT_STR4('f', 'a', 'i', 'l'))) | VT_STR4('\t', 'C', 'X', '=') << 32, 8u);
  {
    const uint64_t cx = (uint64_t)(r.w[3] >> 16) | (uint64_t)(r.w[4] & 0xffffffu) << 16; /* bytes 14 .. 18 */
    const unsigned l = vt_len5(cx);
    s.put8(fmtg_low_bytes(cx, l) | (uint64_t)'\t' << (8u * l), l + 1u);
  }
  /* FORMAT */
  s.put8(VT_STR8('G', 'T', ':', 'F', 'T', ':', 'D', 'P'), 8u);
  s.put8(VT_STR8(':', 'M', 'Q', ':', 'G', 'Q', ':', 'Q'), 8u);
  s.put8(VT_STR8('D', ':', 'G', 'L', ':', 'M', 'C', '8'), 8u);
  if (n_amq) s.put8(VT_STR4(':', 'A', 'M', 'Q'), 4u);
  s.put8(VT_STR8(':', 'C', 'S', ':', 'C', 'G', ':', 'C'), 8u);
  if (het)
    s.put8((uint64_t)'X' | VT_STR4(':', 'F', 'S', '\t') << 8, 5u);
  else
    s.put8((uint64_t)'X' | (uint64_t)'\t' << 8, 2u);
  /* GT FT */
  {
    const int a0 = (int)((gt_enc >> 4) >> 1) - 1, a1 = (int)((gt_enc & 15u) >> 1) - 1; /* -1 .. 6 */
    uint64_t bits;
    unsigned n;
    if (a0 < 0) {
      bits = (uint64_t)'-' | (uint64_t)'1' << 8;
      n = 2u;
    } else {
      bits = (uint64_t)('0' + a0);
      n = 1u;
    }
    bits |= (uint64_t)'/' << (8u * n);
    n++;
    if (a1 < 0) {
      bits |= ((uint64_t)'-' | (uint64_t)'1' << 8) << (8u * n);
      n += 2u;
    } else {
      bits |= (uint64_t)('0' + a1) << (8u * n);
      n++;
    }
    bits |= (uint64_t)':' << (8u * n);
    s.put8(bits, n + 1u); /* <= 6 */
  }
  {
    const uint64_t ft = (flt & 1u)   ? VT_STR4('q', '2', '0', ':')
                        : (flt & 2u) ? VT_STR4('q', 'd', '2', ':')
                        : (flt & 4u) ? (VT_STR4('f', 's', '6', '0') | (uint64_t)':' << 32)
                        : (flt & 8u) ? (VT_STR4('m', 'q', '4', '0') | (uint64_t)':' << 32)
                                     : (VT_STR4('P', 'A', 'S', 'S') | (uint64_t)':' << 32);
    s.put8(ft, (flt & 3u) ? 4u : 5u);
  }
  vt_put_dec(s, r.w[8], false, ':');    /* dp */
  vt_put_int(s, (int32_t)r.w[26], ':'); /* mq */
  vt_put_dec(s, phred, false, ':');
  vt_put_dec(s, r.w[7], false, ':'); /* qd */
  /* GL */
  if (n_gl == 0u) s.put8((uint64_t)':', 1u);
#pragma nounroll
  for (unsigned i = 0; i < n_gl; i++) {
    fmtg_str g = fmtg_format(vt_pick8(&r.w[9], i)); /* (i < 6: the two dwords behind gl[5] are never picked) */
    fmtg_cat(g, (uint64_t)(i + 1u == n_gl ? ':' : ','), 1u);
    s.put16(g.lo, g.hi, g.n);
  }
  /* MC8 [AMQ] */
#pragma nounroll
  for (unsigned k = 0; k < 8u; k++) vt_put_dec(s, vt_pick8(&r.w[16], k), false, k == 7u ? ':' : ',');
  if (n_amq) {
    unsigned left = n_amq;
    const uint64_t quals = (uint64_t)r.w[24] | (uint64_t)r.w[25] << 32; /* bytes 96 .. 103 */
#pragma nounroll
    for (unsigned k = 0; k < 8u; k++)
      if (vt_pick8(&r.w[16], k) > 0u) {
        left--;
        unsigned nq;
        const uint64_t q = vt_dec8((uint32_t)(quals >> (8u * k)) & 0xffu, nq);
        s.put8(q | (uint64_t)(left ? ',' : ':') << (8u * nq), nq + 1u);
      }
  }
  /* CS CG CX [FS] and the newline: exact stores */
  {
    const bool has_c = (0x72u >> gt) & 1u, has_g = (0x1A4u >> gt) & 1u; /* AC CC CG CT / AG CG GG GT */
    fmtg_str t = {0ull, 0ull, 0u};
    if (has_c) fmtg_cat(t, (uint64_t)'+', 1u);
    if (has_g) fmtg_cat(t, (uint64_t)'-', 1u);
    if (!has_c && !has_g) fmtg_cat(t, (uint64_t)'N' | (uint64_t)'A' << 8, 2u);
    fmtg_cat(t, (uint64_t)':' | (uint64_t)r.byte(11) << 8 | (uint64_t)':' << 16, 3u);
    const uint64_t cx = (uint64_t)(r.w[4] >> 24) | (uint64_t)r.w[5] << 8; /* bytes 19 .. 23 */
    const unsigned l = vt_len5(cx);
    fmtg_cat(t, fmtg_low_bytes(cx, l), l);
    if (!het) fmtg_cat(t, (uint64_t)'\n', 1u); /* <= 11 */
    s.put_exact(t.lo, t.hi, t.n);
  }
  if (het) {
    const int32_t fs = (int32_t)r.w[6];
    const uint32_t v = fs < 0 ? (uint32_t)(-(int64_t)fs) : (uint32_t)fs;
    fmtg_str t = {0ull, 0ull, 0u};
    fmtg_cat(t, fs < 0 ? ((uint64_t)':' | (uint64_t)'-' << 8) : (uint64_t)':', fs < 0 ? 2u : 1u);
    unsigned n;
    if (v >= 100000000u) {
      const uint32_t top = v / 100000000u;
      const uint64_t c = vt_dec8(top, n);
      fmtg_cat(t, c, n);
      uint32_t low = v - top * 100000000u;
      uint64_t acc = 0ull;
      for (int i = 0; i < 8; i++) {
        const uint32_t q = low / 10u;
        acc = acc << 8 | (uint64_t)('0' + (low - q * 10u));
        low = q;
      }
      fmtg_cat(t, acc, 8u);
    } else {
      const uint64_t c = vt_dec8(v, n);
      fmtg_cat(t, c, n);
    }
    fmtg_cat(t, (uint64_t)'\n', 1u); /* <= 13 */
    s.put_exact(t.lo, t.hi, t.n);
  }
}

#endif
