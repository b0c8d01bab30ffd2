/*
 * bgzfdev.hip — BGZF compression of a byte stream in HBM (SAM specification section 4.1): every 0xFF00 bytes of the logical stream
 * become one gzip member (FEXTRA, XLEN 6, the 'BC' subfield holding BSIZE - 1), its payload ONE final DEFLATE block (RFC 1951) with
 * dynamic Huffman codes, or a stored block where that would not be smaller than the input, and the payload's CRC-32 and ISIZE.
 *
 * One workgroup of 256 lanes per member, the member's bytes in LDS:
 *   candidates   position p's match candidate is the most recent earlier position with the same 4-byte hash that lies in an EARLIER
 *                round (round r = positions 256 r .. 256 r + 255): the rounds insert with atomicMax, so the table holds the same
 *                positions whatever the order of the lanes' adds; the candidates go to a per-workgroup scratch in HBM.  The lane's
 *                last two match distances are two more candidates (the longest match wins)
 *   parse        lane l parses bytes [255 l, 255 l + 255) greedily with one step of lookahead (matches clipped at the segment's end; 3 .. 258 bytes, distance
 *                <= 32768, never outside the member), counting symbols into LDS histograms and leaving one token per parse step
 *                in the scratch, so the bit-count and the emit pass walk tokens and compare no bytes
 *   codes        length-limited (15 bits; the code-length code 7) canonical codes: symbols ranked by (frequency, symbol) by all
 *                lanes, then Moffat and Katajainen's in-place minimum-redundancy lengths and the usual over-length fix-up on one lane
 *   bits         each lane's bit count, an exclusive prefix sum, then each lane ORs its bits into the member image in LDS
 *                (ds_or_b32: only the words at segment boundaries are shared, and OR does not depend on order)
 *   CRC-32       per lane over its segment with a table in LDS, the lanes' values combined pairwise with x^(8 len) mod P
 * The member image (header, payload, trailer) goes to a fixed 64 KiB slot with its size; bsc_bgzf_scan_kernel sums the sizes and
 * bsc_bgzf_gather_kernel packs the slots end to end.  Everything is a function of the member's bytes alone: same bytes out whatever
 * the launch geometry, the number of CUs or the way the caller split its writes.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BGZF_MEMBER 0xFF00u /* bytes of input per member (htslib's BGZF_BLOCK_SIZE) */
#define BGZF_SLOT 65536u    /* bytes of a member's slot: 18 + 5 + 0xFF00 + 8 at the most */
#define LANES 256u
#define SEG 255u /* BGZF_MEMBER / LANES */
#ifndef HBITS
#define HBITS 14u /* 16 K candidates: 64 KiB of LDS */
#endif
#define NLIT 286
#define NDIST 30
#define NCL 19
#define BUF_WORDS (16384u + 8u)

__constant__ uint16_t c_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t c_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t c_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t c_clorder[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t len_sym(uint32_t len) { /* 3 .. 258 -> 0 .. 28 (lit/len symbol - 257) */
  if (len == 258u) return 28u;
  const uint32_t v = len - 3u;
  if (v < 8u) return v;
  const uint32_t e = 29u - __builtin_clz(v); /* extra bits: floor(log2 v) - 2 */
  return 4u * (e + 1u) + ((v >> e) & 3u);
}
__device__ __forceinline__ uint32_t dist_sym(uint32_t d) { /* 1 .. 32768 -> 0 .. 29 */
  const uint32_t v = d - 1u;
  if (v < 4u) return v;
  const uint32_t nb = 31u - __builtin_clz(v);
  return 2u * nb + ((v >> (nb - 1u)) & 1u);
}
__device__ __forceinline__ uint32_t rev_bits(uint32_t code, uint32_t len) { return __builtin_bitreverse32(code) >> (32u - len); }

/* CRC-32 (reflected, polynomial 0xEDB88320) algebra: a * b mod P, and x^(8 n) mod P from x^(2^k) mod P (zlib's crc32_combine) */
__device__ uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1u)) == 0) break;
    }
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
__device__ uint32_t crc_x8n(const uint32_t *x2n, uint32_t n) {
  uint32_t p = 1u << 31, k = 3;
  while (n) {
    if (n & 1u) p = crc_mulmod(x2n[k & 31u], p);
    n >>= 1;
    k++;
  }
  return p;
}

__device__ __forceinline__ uint32_t lds_u32_at(const uint32_t *w, uint32_t p) { /* 4 bytes at byte p, any alignment */
  const uint64_t v = ((uint64_t)w[(p >> 2) + 1u] << 32) | w[p >> 2];
  return (uint32_t)(v >> ((p & 3u) * 8u));
}

__device__ __forceinline__ uint32_t match_len(const uint32_t *w, uint32_t c, uint32_t p, uint32_t maxl) { /* common prefix of c.. and p.., <= maxl */
  uint32_t l = 0;
  while (l < maxl) {
    const uint32_t x = lds_u32_at(w, c + l) ^ lds_u32_at(w, p + l);
    if (x) {
      l += __builtin_ctz(x) >> 3;
      break;
    }
    l += 4u;
  }
  return l < maxl ? l : maxl;
}

/* the longest match at p (0: none worth a match) among the hash candidate scratch[p] and the distances rep[0..1]; never beyond the
 * segment's end s1, at most 258 bytes, at most 32768 back; ties go to the earlier candidate */
__device__ __forceinline__ uint32_t find_match(const uint32_t *w, const uint32_t *scratch, uint32_t p, uint32_t s1, uint32_t len, const uint32_t *rep,
                                               uint32_t *dist) {
  if (p >= s1 || p + 4u > len) return 0;
  const uint32_t maxl = s1 - p < 258u ? s1 - p : 258u, c1 = scratch[p];
  uint32_t l = 0, d = 0;
  if (c1 && p - (c1 - 1u) <= 32768u) {
    d = p - (c1 - 1u);
    l = match_len(w, c1 - 1u, p, maxl);
  }
  for (int k = 0; k < 2; k++) {
    const uint32_t r = rep[k];
    if (r && r != d && r <= p) {
      const uint32_t lr = match_len(w, p - r, p, maxl);
      if (lr > l) {
        l = lr;
        d = r;
      }
    }
  }
  if (l < 3u || (l == 3u && d > 4096u)) return 0;
  *dist = d;
  return l;
}

/* member bytes [0, n) of src (any alignment) -> LDS bytes [dst_off, dst_off + n): aligned words only, never a word without a byte of
 * the member in it (the source may end anywhere) */
__device__ void load_member(const uint8_t *src, uint32_t n, uint32_t *buf, uint32_t dst_off) {
  const uintptr_t a0 = (uintptr_t)src, a_end = a0 + n;
  const uint32_t sh = (uint32_t)(a0 & 3u);
  const uint32_t *wsrc = (const uint32_t *)(a0 - sh);
  uint8_t *b = (uint8_t *)buf;
  for (uint32_t j = threadIdx.x; j * 4u < n; j += LANES) {
    const uint32_t w0 = wsrc[j];
    const uint32_t w1 = (uintptr_t)(wsrc + j + 1u) < a_end ? wsrc[j + 1u] : 0u;
    const uint32_t v = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (sh * 8u));
    const uint32_t at = dst_off + 4u * j, k = n - 4u * j < 4u ? n - 4u * j : 4u;
    if ((dst_off & 3u) == 0 && k == 4u) buf[at >> 2] = v;
    else
      for (uint32_t i = 0; i < k; i++) b[at + i] = (uint8_t)(v >> (8u * i));
  }
}

/* Huffman code lengths in two steps: rank_symbols (all lanes) puts the used symbols in (frequency, symbol) order into key / sym;
 * huff_lengths (one lane, after a barrier) turns them into the lengths of a code for freq[0 .. n) limited to `limit` bits.  A lone used
 * symbol gets length 1. */
__device__ void rank_symbols(const uint32_t *freq, int n, uint32_t *key, uint16_t *sym) {
  for (int s = threadIdx.x; s < n; s += LANES) {
    const uint32_t f = freq[s];
    if (!f) continue;
    int r = 0;
    for (int t = 0; t < n; t++) {
      const uint32_t g = freq[t];
      r += g && (g < f || (g == f && t < s));
    }
    key[r] = f;
    sym[r] = (uint16_t)s;
  }
}
__device__ void huff_lengths(const uint32_t *freq, int n, int limit, uint32_t *key, const uint16_t *sym, uint8_t *lens) {
  int used = 0;
  for (int s = 0; s < n; s++) {
    lens[s] = 0;
    used += freq[s] != 0;
  }
  if (used == 0) return;
  if (used == 1) {
    lens[sym[0]] = 1;
    return;
  }
  /* Moffat & Katajainen, in place over the ascending frequencies key[0 .. used) */
  uint32_t *A = key;
  const int nn = used;
  A[0] += A[1];
  int root = 0, leaf = 2, next;
  for (next = 1; next < nn - 1; next++) {
    if (leaf >= nn || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else A[next] = A[leaf++];
    if (leaf >= nn || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else A[next] += A[leaf++];
  }
  A[nn - 2] = 0;
  for (next = nn - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
  int avbl = 1, usedn = 0, dpth = 0;
  root = nn - 2;
  next = nn - 1;
  while (avbl > 0) {
    while (root >= 0 && (int)A[root] == dpth) {
      usedn++;
      root--;
    }
    while (avbl > usedn) {
      A[next--] = (uint32_t)dpth;
      avbl--;
    }
    avbl = 2 * usedn;
    dpth++;
    usedn = 0;
  }
  /* A[i]: the code length of the i-th least frequent symbol.  Over-long codes: fold them into `limit` and restore Kraft's equality */
  int num[33];
  for (int i = 0; i <= 32; i++) num[i] = 0;
  for (int i = 0; i < nn; i++) num[A[i] > 32u ? 32 : A[i]]++;
  for (int i = limit + 1; i <= 32; i++) {
    num[limit] += num[i];
    num[i] = 0;
  }
  uint32_t total = 0;
  for (int i = limit; i > 0; i--) total += (uint32_t)num[i] << (limit - i);
  while (total != (1u << limit)) {
    num[limit]--;
    for (int i = limit - 1; i > 0; i--)
      if (num[i]) {
        num[i]--;
        num[i + 1] += 2;
        break;
      }
    total--;
  }
  int j = nn;
  for (int l = 1; l <= limit; l++)
    for (int k = num[l]; k > 0; k--) lens[sym[--j]] = (uint8_t)l;
}
/* canonical codes, bit-reversed for an LSB-first writer: code | length << 16 */
__device__ void canon_codes(const uint8_t *lens, int n, uint32_t *code) {
  uint32_t cnt[16], nxt[16];
  for (int i = 0; i < 16; i++) cnt[i] = 0;
  for (int s = 0; s < n; s++) cnt[lens[s]]++;
  cnt[0] = 0;
  uint32_t c = 0;
  for (int l = 1; l < 16; l++) {
    c = (c + cnt[l - 1]) << 1;
    nxt[l] = c;
  }
  for (int s = 0; s < n; s++) code[s] = lens[s] ? rev_bits(nxt[lens[s]]++, lens[s]) | ((uint32_t)lens[s] << 16) : 0u;
}

struct hdr_writer { /* one lane's plain writer into the zeroed member image */
  uint32_t *buf;
  uint32_t at;
  __device__ void put(uint32_t v, uint32_t k) {
    if (!k) return;
    const uint32_t w = at >> 5, s = at & 31u;
    buf[w] |= v << s;
    if (s + k > 32u) buf[w + 1u] |= v >> (32u - s);
    at += k;
  }
};
struct lane_writer { /* a lane's bits, ORed in: its first and last words are shared with its neighbours' */
  uint32_t *buf;
  uint32_t w, nb;
  uint64_t acc;
  __device__ void put(uint32_t v, uint32_t k) {
    acc |= (uint64_t)v << nb;
    nb += k;
    if (nb >= 32u) {
      atomicOr(&buf[w], (uint32_t)acc);
      w++;
      acc >>= 32;
      nb -= 32u;
    }
  }
  __device__ void flush() {
    if (nb) atomicOr(&buf[w], (uint32_t)acc);
  }
};

__device__ __forceinline__ void put_gzip_header(uint8_t *b, uint32_t size) {
  const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
  for (int i = 0; i < 16; i++) b[i] = h[i];
  b[16] = (uint8_t)((size - 1u) & 0xffu);
  b[17] = (uint8_t)((size - 1u) >> 8);
}
__device__ __forceinline__ void put_u32le(uint8_t *b, uint32_t v) {
  for (int i = 0; i < 4; i++) b[i] = (uint8_t)(v >> (8 * i));
}

/*
 * src[0 .. n): the members' bytes, member m = [m 0xFF00, min((m + 1) 0xFF00, n)); slots[n_members][64 KiB]; sizes[n_members];
 * scratch[gridDim.x][0xFF00] u32.  Workgroups loop over the members.
 */
extern "C" __global__ __launch_bounds__(256) void bsc_bgzf_deflate_kernel(const uint8_t *__restrict__ src, uint64_t n, uint32_t n_members,
                                                                         uint8_t *__restrict__ slots, unsigned long long *__restrict__ sizes,
                                                                         uint32_t *__restrict__ scratch_all) {
  __shared__ __attribute__((aligned(16))) uint32_t s_buf[BUF_WORDS]; /* the member's bytes, then its image */
  __shared__ uint32_t s_head[1u << HBITS];
  __shared__ uint32_t s_crctab[256];
  __shared__ uint32_t s_x2n[32];
  __shared__ uint32_t s_crc[LANES];
  __shared__ uint32_t s_bits[LANES];
  __shared__ uint32_t s_lhist[NLIT], s_dhist[NDIST], s_chist[NCL];
  __shared__ uint32_t s_lcode[NLIT], s_dcode[NDIST], s_ccode[NCL];
  __shared__ uint8_t s_llen[NLIT], s_dlen[NDIST], s_clen[NCL];
  __shared__ uint32_t s_lkey[NLIT], s_dkey[NDIST], s_ckey[NCL];
  __shared__ uint16_t s_lsym[NLIT], s_dsym[NDIST], s_csym[NCL];
  __shared__ uint16_t s_rle[NLIT + NDIST]; /* code-length symbol | extra value << 5 */
  __shared__ uint32_t s_meta[4];           /* n_rle, header bits, HLIT, HDIST */
  const uint32_t tid = threadIdx.x;
  uint32_t *scratch = scratch_all + (size_t)blockIdx.x * BGZF_MEMBER;
  uint8_t *s_bytes = (uint8_t *)s_buf;

  for (uint32_t i = tid; i < 256u; i += LANES) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    s_crctab[i] = c;
  }
  if (tid == 0) {
    uint32_t p = 1u << 30; /* x^1 */
    s_x2n[0] = p;
    for (int k = 1; k < 32; k++) s_x2n[k] = p = crc_mulmod(p, p);
  }

  for (uint32_t m = blockIdx.x; m < n_members; m += gridDim.x) {
    const uint64_t base = (uint64_t)m * BGZF_MEMBER;
    const uint32_t len = (uint32_t)(n - base < BGZF_MEMBER ? n - base : BGZF_MEMBER);
    __syncthreads(); /* the previous member's image is out */
    load_member(src + base, len, s_buf, 0);
    for (uint32_t w = ((len + 3u) >> 2) + tid; w < BUF_WORDS; w += LANES) s_buf[w] = 0;
    for (uint32_t i = tid; i < (1u << HBITS); i += LANES) s_head[i] = 0;
    __syncthreads();
    if (tid == 0 && (len & 3u)) s_buf[len >> 2] &= (1u << (8u * (len & 3u))) - 1u; /* the bytes behind the member: zero */
    const uint32_t s0 = tid * SEG, s1 = s0 + SEG < len ? s0 + SEG : len, seg_n = s0 < len ? s1 - s0 : 0u;
    __syncthreads();
    { /* CRC-32 of this lane's segment */
      uint32_t c = 0xFFFFFFFFu;
      for (uint32_t p = s0; p < s0 + seg_n; p++) c = s_crctab[(c ^ s_bytes[p]) & 0xffu] ^ (c >> 8);
      s_crc[tid] = c ^ 0xFFFFFFFFu;
    }
    __syncthreads();
    for (uint32_t st = 1; st < LANES; st <<= 1) { /* crc(A B) = crc(A) x^(8 |B|) + crc(B) */
      if ((tid & (2u * st - 1u)) == 0) {
        const uint32_t r0 = (tid + st) * SEG;
        const uint32_t rn = r0 >= len ? 0u : (len - r0 < st * SEG ? len - r0 : st * SEG);
        if (rn) s_crc[tid] = crc_mulmod(crc_x8n(s_x2n, rn), s_crc[tid]) ^ s_crc[tid + st];
      }
      __syncthreads();
    }
    const uint32_t crc = s_crc[0];

    /* candidates: round r's positions see the table as the rounds before r left it */
    const uint32_t n_rounds = (len + LANES - 1u) / LANES;
    for (uint32_t r = 0; r < n_rounds; r++) {
      const uint32_t p = r * LANES + tid;
      uint32_t h = 0;
      const bool ok = p + 4u <= len;
      if (ok) {
        h = (lds_u32_at(s_buf, p) * 2654435761u) >> (32u - HBITS);
        scratch[p] = s_head[h];
      }
      __syncthreads();
      if (ok) atomicMax(&s_head[h], p + 1u);
      __syncthreads();
    }
    for (uint32_t i = tid; i < NLIT; i += LANES) s_lhist[i] = 0;
    if (tid < NDIST) s_dhist[tid] = 0;
    if (tid < NCL) s_chist[tid] = 0;
    __syncthreads();

    /* parse over the lane's segment, greedy with one step of lookahead (a longer match at p + 1 turns p into a literal); a token per
     * step (literal: the byte; match: length << 16 | distance - 1) */
    uint32_t rep[2] = {0, 0}; /* the lane's last two match distances: more candidates (BCF records repeat their neighbours' layout) */
    for (uint32_t p = s0; p < s0 + seg_n;) {
      uint32_t d = 0, d1 = 0;
      uint32_t l = find_match(s_buf, scratch, p, s1, len, rep, &d);
      if (l && l < 32u && find_match(s_buf, scratch, p + 1u, s1, len, rep, &d1) > l) l = 0;
      if (l) {
        atomicAdd(&s_lhist[257u + len_sym(l)], 1u);
        atomicAdd(&s_dhist[dist_sym(d)], 1u);
        scratch[p] = (l << 16) | (d - 1u);
        if (d != rep[0]) {
          rep[1] = rep[0];
          rep[0] = d;
        }
        p += l;
      } else {
        const uint32_t b = s_bytes[p];
        atomicAdd(&s_lhist[b], 1u);
        scratch[p] = b;
        p++;
      }
    }
    if (tid == 0) atomicAdd(&s_lhist[256], 1u);
    __syncthreads();

    /* the codes */
    rank_symbols(s_lhist, NLIT, s_lkey, s_lsym);
    rank_symbols(s_dhist, NDIST, s_dkey, s_dsym);
    __syncthreads();
    if (tid == 0) {
      huff_lengths(s_lhist, NLIT, 15, s_lkey, s_lsym, s_llen);
      canon_codes(s_llen, NLIT, s_lcode);
    } else if (tid == 64) {
      uint32_t any = 0;
      for (int s = 0; s < NDIST; s++) any |= s_dhist[s];
      if (any) huff_lengths(s_dhist, NDIST, 15, s_dkey, s_dsym, s_dlen);
      else { /* no match: one distance code of one bit, the one incomplete tree inflaters take */
        for (int s = 0; s < NDIST; s++) s_dlen[s] = 0;
        s_dlen[0] = 1;
      }
      canon_codes(s_dlen, NDIST, s_dcode);
    }
    __syncthreads();
    if (tid == 0) { /* the code lengths as code-length symbols (16: repeat the last 3-6 times, 17: 3-10 zeros, 18: 11-138 zeros) */
      int hlit = NLIT, hdist = NDIST;
      while (hlit > 257 && !s_llen[hlit - 1]) hlit--;
      while (hdist > 1 && !s_dlen[hdist - 1]) hdist--;
      const int tot = hlit + hdist;
      int nr = 0, i = 0;
#define LEN_AT(k) ((k) < hlit ? s_llen[(k)] : s_dlen[(k) - hlit])
#define RLE(sym, ext)                                         \
  do {                                                        \
    s_rle[nr++] = (uint16_t)((sym) | ((uint32_t)(ext) << 5)); \
    s_chist[(sym)]++;                                         \
  } while (0)
      while (i < tot) {
        const uint32_t v = LEN_AT(i);
        int run = 1;
        while (i + run < tot && LEN_AT(i + run) == v) run++;
        if (v == 0) {
          while (run >= 11) {
            const int r = run < 138 ? run : 138;
            RLE(18, r - 11);
            run -= r;
            i += r;
          }
          if (run >= 3) {
            RLE(17, run - 3);
            i += run;
            run = 0;
          }
        } else {
          RLE(v, 0);
          i++;
          run--;
          while (run >= 3) {
            const int r = run < 6 ? run : 6;
            RLE(16, r - 3);
            run -= r;
            i += r;
          }
        }
        for (; run > 0; run--, i++) RLE(v, 0);
      }
#undef RLE
#undef LEN_AT
      int used = 0, only = 0;
      for (int s = 0; s < NCL; s++)
        if (s_chist[s]) used++, only = s;
      if (used == 1) s_chist[only == 0 ? 1 : 0] = 1; /* the code-length code must be complete: two symbols at least */
      s_meta[0] = (uint32_t)nr;
      s_meta[2] = (uint32_t)hlit;
      s_meta[3] = (uint32_t)hdist;
    }
    __syncthreads();
    rank_symbols(s_chist, NCL, s_ckey, s_csym);
    for (uint32_t w = tid; w < BUF_WORDS; w += LANES) s_buf[w] = 0; /* the image: the member's bytes are in the tokens now */
    __syncthreads();
    if (tid == 0) {
      huff_lengths(s_chist, NCL, 7, s_ckey, s_csym, s_clen);
      canon_codes(s_clen, NCL, s_ccode);
      int hclen = NCL;
      while (hclen > 4 && !s_clen[c_clorder[hclen - 1]]) hclen--;
      hdr_writer hw{s_buf, 18u * 8u};
      hw.put(5u, 3u); /* BFINAL 1, BTYPE 10 */
      hw.put(s_meta[2] - 257u, 5u);
      hw.put(s_meta[3] - 1u, 5u);
      hw.put((uint32_t)hclen - 4u, 4u);
      for (int k = 0; k < hclen; k++) hw.put(s_clen[c_clorder[k]], 3u);
      for (uint32_t k = 0; k < s_meta[0]; k++) {
        const uint32_t sy = s_rle[k] & 31u, ex = s_rle[k] >> 5, cc = s_ccode[sy];
        hw.put(cc & 0xffffu, cc >> 16);
        if (sy == 16) hw.put(ex, 2u);
        else if (sy == 17) hw.put(ex, 3u);
        else if (sy == 18) hw.put(ex, 7u);
      }
      s_meta[1] = hw.at;
    }
    /* this lane's bits */
    uint32_t bits = 0;
    for (uint32_t p = s0; p < s0 + seg_n;) {
      const uint32_t t = scratch[p];
      if (t >> 16) {
        const uint32_t l = t >> 16, d = (t & 0xffffu) + 1u, ls = len_sym(l), ds = dist_sym(d);
        bits += (s_lcode[257u + ls] >> 16) + c_lext[ls] + (s_dcode[ds] >> 16) + c_dext[ds];
        p += l;
      } else {
        bits += s_lcode[t] >> 16;
        p++;
      }
    }
    s_bits[tid] = bits;
    __syncthreads();
    if (tid == 0) {
      uint32_t at = s_meta[1];
      for (uint32_t k = 0; k < LANES; k++) {
        const uint32_t b = s_bits[k];
        s_bits[k] = at;
        at += b;
      }
      s_meta[1] = at; /* where end-of-block goes */
    }
    __syncthreads();
    const uint32_t eob_at = s_meta[1], dyn_end = eob_at + (s_lcode[256] >> 16), dyn_bytes = (dyn_end + 7u) / 8u - 18u;
    uint32_t size;
    if (dyn_bytes < len) {
      lane_writer lw{s_buf, s_bits[tid] >> 5, s_bits[tid] & 31u, 0};
      for (uint32_t p = s0; p < s0 + seg_n;) {
        const uint32_t t = scratch[p];
        if (t >> 16) {
          const uint32_t l = t >> 16, d = (t & 0xffffu) + 1u, ls = len_sym(l), ds = dist_sym(d);
          const uint32_t lc = s_lcode[257u + ls], dc = s_dcode[ds];
          lw.put(lc & 0xffffu, lc >> 16);
          lw.put(l - c_lbase[ls], c_lext[ls]);
          lw.put(dc & 0xffffu, dc >> 16);
          lw.put(d - c_dbase[ds], c_dext[ds]);
          p += l;
        } else {
          const uint32_t lc = s_lcode[t];
          lw.put(lc & 0xffffu, lc >> 16);
          p++;
        }
      }
      if (tid == LANES - 1u) {
        const uint32_t lc = s_lcode[256];
        lw.put(lc & 0xffffu, lc >> 16);
      }
      lw.flush();
      size = 18u + dyn_bytes + 8u;
      __syncthreads();
      if (tid == 0) {
        put_gzip_header(s_bytes, size);
        put_u32le(s_bytes + 18u + dyn_bytes, crc);
        put_u32le(s_bytes + 22u + dyn_bytes, len);
      }
    } else { /* stored: the member's bytes once more, from HBM */
      size = 18u + 5u + len + 8u;
      __syncthreads();
      for (uint32_t w = tid; w < BUF_WORDS; w += LANES) s_buf[w] = 0;
      __syncthreads();
      load_member(src + base, len, s_buf, 23u);
      if (tid == 0) {
        put_gzip_header(s_bytes, size);
        s_bytes[18] = 1; /* BFINAL 1, BTYPE 00 */
        s_bytes[19] = (uint8_t)(len & 0xffu);
        s_bytes[20] = (uint8_t)(len >> 8);
        s_bytes[21] = (uint8_t)(~len & 0xffu);
        s_bytes[22] = (uint8_t)((~len >> 8) & 0xffu);
        put_u32le(s_bytes + 23u + len, crc);
        put_u32le(s_bytes + 27u + len, len);
      }
    }
    __syncthreads();
    uint4 *dst = (uint4 *)(slots + (size_t)m * BGZF_SLOT);
    const uint4 *img = (const uint4 *)s_buf;
    for (uint32_t i = tid; i * 16u < size; i += LANES) dst[i] = img[i];
    if (tid == 0) sizes[m] = size;
  }
}

/* offs[i] = sizes[0] + ... + sizes[i - 1], offs[n] = the total; one workgroup */
extern "C" __global__ __launch_bounds__(256) void bsc_bgzf_scan_kernel(const unsigned long long *__restrict__ sizes, unsigned long long *__restrict__ offs,
                                                                      uint32_t n) {
  __shared__ unsigned long long s_part[LANES];
  const uint32_t per = (n + LANES - 1u) / LANES, a = threadIdx.x * per, b = a + per < n ? a + per : n;
  unsigned long long t = 0;
  for (uint32_t i = a; i < b; i++) t += sizes[i];
  s_part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long at = 0;
    for (uint32_t k = 0; k < LANES; k++) {
      const unsigned long long v = s_part[k];
      s_part[k] = at;
      at += v;
    }
    offs[n] = at;
  }
  __syncthreads();
  unsigned long long at = s_part[threadIdx.x];
  for (uint32_t i = a; i < b; i++) {
    offs[i] = at;
    at += sizes[i];
  }
}

/* member m's slot -> out[offs[m], offs[m] + sizes[m]): whole words inside the member, single bytes where a word is shared with a
 * neighbour */
extern "C" __global__ __launch_bounds__(256) void bsc_bgzf_gather_kernel(const uint8_t *__restrict__ slots, const unsigned long long *__restrict__ offs,
                                                                        const unsigned long long *__restrict__ sizes, uint8_t *__restrict__ out) {
  const uint32_t m = blockIdx.x, size = (uint32_t)sizes[m];
  const uint8_t *s = slots + (size_t)m * BGZF_SLOT;
  const uint32_t *sw = (const uint32_t *)s;
  uint8_t *d = out + offs[m];
  const uint32_t lead = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u), h = lead < size ? lead : size;
  const uint32_t nw = (size - h) / 4u, tail = h + 4u * nw;
  if (threadIdx.x < h) d[threadIdx.x] = s[threadIdx.x];
  if (threadIdx.x < size - tail) d[tail + threadIdx.x] = s[tail + threadIdx.x];
  uint32_t *dw = (uint32_t *)(d + h);
  const uint32_t sh = h & 3u;
  for (uint32_t j = threadIdx.x; j < nw; j += LANES) {
    const uint32_t q = (h >> 2) + j; /* source word of byte h + 4 j; its neighbour lies inside the 64 KiB slot */
    const uint64_t v = ((uint64_t)sw[q + 1u] << 32) | sw[q];
    dw[j] = (uint32_t)(v >> (8u * sh));
  }
}

extern "C" int bsc_dev_launch_bgzf(const void *src, uint64_t n, uint32_t n_members, void *slots, void *sizes, void *offs, void *scratch, uint32_t grid,
                                   void *stream) {
  if (!n_members) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bsc_bgzf_deflate_kernel, dim3(grid), dim3(LANES), 0, s, (const uint8_t *)src, n, n_members, (uint8_t *)slots,
                     (unsigned long long *)sizes, (uint32_t *)scratch);
  hipLaunchKernelGGL(bsc_bgzf_scan_kernel, dim3(1), dim3(LANES), 0, s, (const unsigned long long *)sizes, (unsigned long long *)offs, n_members);
  return (int)hipGetLastError();
}

extern "C" int bsc_dev_launch_bgzf_gather(const void *slots, const void *offs, const void *sizes, uint32_t n_members, void *out, void *stream) {
  if (!n_members) return 0;
  hipLaunchKernelGGL(bsc_bgzf_gather_kernel, dim3(n_members), dim3(LANES), 0, (hipStream_t)stream, (const uint8_t *)slots,
                     (const unsigned long long *)offs, (const unsigned long long *)sizes, (uint8_t *)out);
  return (int)hipGetLastError();
}
