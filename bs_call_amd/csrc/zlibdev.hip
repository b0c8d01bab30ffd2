/*
 * zlibdev.hip — zlib streams (RFC 1950) of the fixed-stride pieces of a byte stream in HBM: piece k = bytes [k piece, min((k + 1) piece, n))
 * becomes the two header bytes 78 9C, ONE final DEFLATE block (RFC 1951) with dynamic Huffman codes — or a stored block where that would
 * not be smaller than the piece — and the piece's Adler-32, big-endian: at most the piece + 11 bytes.  The bigWig track's sections (8 KB by
 * default, 24 + 8 S bytes of {start u32, value f32} items) are what it is shaped for; csrc/bgzfdev.hip is the encoder for 0xFF00-byte BGZF
 * members, and the stages are its stages, sized for small pieces:
 *
 * One workgroup of 256 lanes per piece, the piece's bytes in LDS (two instances: pieces up to ZL_SMALL_PIECE bytes in 8 KiB, several
 * workgroups a CU; the rest in 64 KiB):
 *   candidates   position p's hash candidate is the most recent position with the same 3-byte hash in an EARLIER phase (round r = positions
 *                256 r .. 256 r + 255, inserted in ZL_PHASES phases of 64 lanes; atomicMax, so the table does not depend on the lanes'
 *                order), 2^12 entries.  Beside it: the distances 8, 16 .. 8 ZL_NPER (the item period: the same byte of the items before)
 *                and the lane's last two match distances.  The longest match wins, the nearer candidate on a tie
 *   parse        lane l parses bytes [l seg, (l + 1) seg), seg = max(ceil(len / 256), ZL_SEG_MIN): every lane works on an 8 KB piece;
 *                greedy with one step of lookahead, matches clipped at the segment's end; a token per step in a per-workgroup scratch in HBM
 *   codes        ranked symbols, Moffat and Katajainen's lengths limited to 15 (7) bits, canonical codes
 *   bits         each lane's bit count, an exclusive prefix sum, the lanes OR their bits into the image in LDS
 *   Adler-32     (a, b) per lane over its segment, combined pairwise: a = aL + aR - 1, b = bL + bR + lenR (aL - 1) mod 65521, in 64 bits
 * The image goes to a slot of round16(piece + 11) + 16 bytes with its size; bsc_zlib_scan_kernel sums the sizes and leaves the totals;
 * bsc_zlib_gather_kernel packs the slots end to end and copies the sizes — each only if its room holds all of it.  A stream is a function
 * of its piece's bytes alone.  (The helpers from the tables to the two writers are bgzfdev.hip's, restated here so that file stays as it is.)
 *
 * Pieces of varying length (the bigBed blocks: bsc_zlib_ranges_device): the same body, bsc_zlib_deflate_ranges_small_kernel / _large_kernel,
 * with a piece's base and length taken from n_pieces + 1 ascending offsets instead of a stride; slots and scratch are sized for the longest
 * piece the caller allows.  A range of no byte reads nothing and gets size 0, a longer one is cut at that length, and both are counted: no
 * offset, whatever it holds, makes a workgroup touch memory outside its buffers or outside the range it names.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

#define ZL_MAX_PIECE 0xFF00u
#define ZL_SMALL_PIECE 8224u /* the default section of 1024 sites is 8216 bytes */
#define ZL_LANES 256u
#define ZL_SEG_MIN 32u
#ifndef ZL_HBITS
#define ZL_HBITS 12u
#endif
/* the matcher's three knobs, as measured on the sections of a 30x synthetic block (DESIGN.md section 6 has the table) */
#ifndef ZL_NPER
#define ZL_NPER 12 /* item-period candidates: distances 8, 16, .. 96 */
#endif
#ifndef ZL_PHASES
#define ZL_PHASES 4u /* insert phases a round: a position sees the earlier phases' positions of its own round too */
#endif
#ifndef ZL_LEN3_FAR
#define ZL_LEN3_FAR 512u /* a 3-byte match farther back than this is dearer than three literals */
#endif
#define ZL_NLIT 286
#define ZL_NDIST 30
#define ZL_NCL 19
/* words of the LDS buffer: the piece or its image (piece + 11 bytes), rounded up to 16 bytes, and 8 words behind it for the unaligned reads;
 * never less than the longest header of a dynamic block (14 + 57 + 316 * 14 bits behind the two zlib bytes: 564 bytes) */
#define ZL_WORDS(piece) ((((piece) + 11u + 15u) / 16u) * 4u + 8u)

__constant__ uint16_t z_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t z_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t z_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t z_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t z_clorder[ZL_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t len_sym(uint32_t len) { /* 3 .. 258 -> 0 .. 28 (lit/len symbol - 257) */
  if (len == 258u) return 28u;
  const uint32_t v = len - 3u;
  if (v < 8u) return v;
  const uint32_t e = 29u - __builtin_clz(v);
  return 4u * (e + 1u) + ((v >> e) & 3u);
}
__device__ __forceinline__ uint32_t dist_sym(uint32_t d) { /* 1 .. 32768 -> 0 .. 29 */
  const uint32_t v = d - 1u;
  if (v < 4u) return v;
  const uint32_t nb = 31u - __builtin_clz(v);
  return 2u * nb + ((v >> (nb - 1u)) & 1u);
}
__device__ __forceinline__ uint32_t rev_bits(uint32_t code, uint32_t len) { return __builtin_bitreverse32(code) >> (32u - len); }

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

/* the longest match at p (0: none worth a match) among the distances 8 .. 8 ZL_NPER, rep[0..1] and the hash candidate scratch[p]; never beyond
 * the segment's end s1 (s1 <= the piece's length), at most 258 bytes; ties go to the nearer candidate */
__device__ __forceinline__ uint32_t find_match(const uint32_t *w, const uint32_t *scratch, uint32_t p, uint32_t s1, const uint32_t *rep, uint32_t *dist) {
  if (p + 3u > s1) return 0;
  const uint32_t maxl = s1 - p < 258u ? s1 - p : 258u, c1 = scratch[p];
  uint32_t l = 0, d = 0;
  /* the near candidates first — a short distance is the cheaper code —, a later one wins only by being longer */
#pragma unroll
  for (uint32_t r = 8u; r <= 8u * ZL_NPER; r += 8u) {
    if (r <= p) {
      const uint32_t lr = match_len(w, p - r, p, maxl);
      if (lr > l) {
        l = lr;
        d = r;
      }
    }
  }
  for (int k = 0; k < 2; k++) {
    const uint32_t r = rep[k];
    if (r && r <= p && !((r & 7u) == 0 && r <= 8u * ZL_NPER)) {
      const uint32_t lr = match_len(w, p - r, p, maxl);
      if (lr > l) {
        l = lr;
        d = r;
      }
    }
  }
  if (c1 && p - (c1 - 1u) <= 32768u) { /* c1 - 1 < p: an earlier position; a piece may be longer than the window */
    const uint32_t lr = match_len(w, c1 - 1u, p, maxl);
    if (lr > l) {
      l = lr;
      d = p - (c1 - 1u);
    }
  }
  if (l < 3u || (l == 3u && d > ZL_LEN3_FAR)) return 0;
  *dist = d;
  return l;
}

/* piece bytes [0, n) of src (any alignment) -> LDS bytes [dst_off, dst_off + n): aligned words only, never a word without a byte of the
 * piece in it (the source may end anywhere) */
__device__ void load_piece(const uint8_t *src, uint32_t n, uint32_t *buf, uint32_t dst_off) {
  const uintptr_t a0 = (uintptr_t)src, a_end = a0 + n;
  const uint32_t sh = (uint32_t)(a0 & 3u);
  const uint32_t *wsrc = (const uint32_t *)(a0 - sh);
  uint8_t *b = (uint8_t *)buf;
  for (uint32_t j = threadIdx.x; j * 4u < n; j += ZL_LANES) {
    const uint32_t w0 = wsrc[j];
    const uint32_t w1 = (uintptr_t)(wsrc + j + 1u) < a_end ? wsrc[j + 1u] : 0u;
    const uint32_t v = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (sh * 8u));
    const uint32_t at = dst_off + 4u * j, k = n - 4u * j < 4u ? n - 4u * j : 4u;
    if ((dst_off & 3u) == 0 && k == 4u) buf[at >> 2] = v;
    else
      for (uint32_t i = 0; i < k; i++) b[at + i] = (uint8_t)(v >> (8u * i));
  }
}

/* rank_symbols (all lanes): the used symbols in (frequency, symbol) order into key / sym; huff_lengths (one lane, after a barrier): the
 * lengths of a code for freq[0 .. n) limited to `limit` bits.  A lone used symbol gets length 1. */
__device__ void rank_symbols(const uint32_t *freq, int n, uint32_t *key, uint16_t *sym) {
  for (int s = threadIdx.x; s < n; s += ZL_LANES) {
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

struct hdr_writer { /* one lane's plain writer into the zeroed image */
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

__device__ __forceinline__ void put_u32be(uint8_t *b, uint32_t v) {
  for (int i = 0; i < 4; i++) b[i] = (uint8_t)(v >> (24 - 8 * i));
}

/*
 * src[0 .. n): piece k = [k piece, min((k + 1) piece, n)); slots[n_pieces][slot]; sizes[n_pieces]; scratch[gridDim.x][piece] u32.
 * PIECE_MAX: the longest piece of this instance (piece <= PIECE_MAX).  Workgroups loop over the pieces.
 */
template <uint32_t PIECE_MAX, bool RANGES = false>
__device__ __forceinline__ void zlib_deflate_body(const uint8_t *__restrict__ src, uint64_t n, uint32_t piece, uint32_t n_pieces, uint8_t *__restrict__ slots,
                                                  uint32_t slot, uint32_t *__restrict__ sizes, uint32_t *__restrict__ scratch_all,
                                                  const unsigned long long *__restrict__ range_offs = nullptr, unsigned long long *bad = nullptr) {
  constexpr uint32_t WORDS = ZL_WORDS(PIECE_MAX) < 160u ? 160u : ZL_WORDS(PIECE_MAX);
  __shared__ __attribute__((aligned(16))) uint32_t s_buf[WORDS]; /* the piece's bytes, then its image */
  __shared__ uint32_t s_head[1u << ZL_HBITS];
  __shared__ uint32_t s_ada[ZL_LANES], s_adb[ZL_LANES];
  __shared__ uint32_t s_bits[ZL_LANES];
  __shared__ uint32_t s_lhist[ZL_NLIT], s_dhist[ZL_NDIST], s_chist[ZL_NCL];
  __shared__ uint32_t s_lcode[ZL_NLIT], s_dcode[ZL_NDIST], s_ccode[ZL_NCL];
  __shared__ uint8_t s_llen[ZL_NLIT], s_dlen[ZL_NDIST], s_clen[ZL_NCL];
  __shared__ uint32_t s_lkey[ZL_NLIT], s_dkey[ZL_NDIST], s_ckey[ZL_NCL];
  __shared__ uint16_t s_lsym[ZL_NLIT], s_dsym[ZL_NDIST], s_csym[ZL_NCL];
  __shared__ uint16_t s_rle[ZL_NLIT + ZL_NDIST]; /* code-length symbol | extra value << 5 */
  __shared__ uint32_t s_meta[4];                 /* n_rle, header bits, HLIT, HDIST */
  const uint32_t tid = threadIdx.x;
  uint32_t *scratch = scratch_all + (size_t)blockIdx.x * piece;
  uint8_t *s_bytes = (uint8_t *)s_buf;

  for (uint32_t m = blockIdx.x; m < n_pieces; m += gridDim.x) {
    uint64_t base;
    uint32_t len;
    if (RANGES) { /* piece m = [offs[m], offs[m + 1]): its length clamped to what the buffers of this launch are sized for */
      const unsigned long long o0 = range_offs[m], o1 = range_offs[m + 1u];
      const bool none = o1 <= o0, over = !none && o1 - o0 > piece;
      if ((none || over) && tid == 0) atomicAdd(bad, 1ull); /* an integer count: no order can change it */
      if (none) { /* (block-uniform) nothing of the source is read, nothing but the size is written */
        if (tid == 0) sizes[m] = 0u;
        continue;
      }
      base = o0;
      len = over ? piece : (uint32_t)(o1 - o0);
    } else {
      base = (uint64_t)m * piece;
      len = (uint32_t)(n - base < piece ? n - base : piece);
    }
    __syncthreads(); /* the previous piece's image is out */
    load_piece(src + base, len, s_buf, 0);
    for (uint32_t w = ((len + 3u) >> 2) + tid; w < WORDS; w += ZL_LANES) s_buf[w] = 0;
    for (uint32_t i = tid; i < (1u << ZL_HBITS); i += ZL_LANES) s_head[i] = 0;
    __syncthreads();
    if (tid == 0 && (len & 3u)) s_buf[len >> 2] &= (1u << (8u * (len & 3u))) - 1u; /* the bytes behind the piece: zero */
    uint32_t seg = (len + ZL_LANES - 1u) / ZL_LANES; /* <= 255 */
    if (seg < ZL_SEG_MIN) seg = ZL_SEG_MIN;
    const uint32_t s0 = tid * seg, s1 = s0 + seg < len ? s0 + seg : len, seg_n = s0 < len ? s1 - s0 : 0u;
    __syncthreads();
    { /* Adler-32 of this lane's segment: at most 255 bytes, so a <= 65026 and b < 2^24 before the one reduction */
      uint32_t a = 1u, b = 0u;
      for (uint32_t p = s0; p < s0 + seg_n; p++) {
        a += s_bytes[p];
        b += a;
      }
      s_ada[tid] = a % 65521u;
      s_adb[tid] = b % 65521u;
    }
    __syncthreads();
    for (uint32_t st = 1; st < ZL_LANES; st <<= 1) { /* adler(L R): a = aL + aR - 1, b = bL + bR + |R| (aL - 1) */
      if ((tid & (2u * st - 1u)) == 0) {
        const uint32_t r0 = (tid + st) * seg;
        const uint32_t rn = r0 >= len ? 0u : (len - r0 < st * seg ? len - r0 : st * seg);
        if (rn) {
          const uint32_t al = s_ada[tid], ar = s_ada[tid + st];
          const uint64_t b = (uint64_t)s_adb[tid] + s_adb[tid + st] + (uint64_t)rn * ((al + 65520u) % 65521u);
          s_ada[tid] = (al + ar + 65520u) % 65521u;
          s_adb[tid] = (uint32_t)(b % 65521u);
        }
      }
      __syncthreads();
    }
    const uint32_t adler = (s_adb[0] << 16) | s_ada[0];

    /* candidates: round r's positions see the table as the rounds before r left it */
    const uint32_t n_rounds = (len + ZL_LANES - 1u) / ZL_LANES;
    for (uint32_t r = 0; r < n_rounds; r++) {
      const uint32_t p = r * ZL_LANES + tid;
      uint32_t h = 0;
      const bool ok = p + 3u <= len;
      if (ok) h = ((lds_u32_at(s_buf, p) & 0xFFFFFFu) * 2654435761u) >> (32u - ZL_HBITS);
      for (uint32_t q = 0; q < ZL_PHASES; q++) {
        const bool mine = ok && tid / (ZL_LANES / ZL_PHASES) == q;
        if (mine) scratch[p] = s_head[h];
        __syncthreads();
        if (mine) atomicMax(&s_head[h], p + 1u);
        __syncthreads();
      }
    }
    for (uint32_t i = tid; i < ZL_NLIT; i += ZL_LANES) s_lhist[i] = 0;
    if (tid < ZL_NDIST) s_dhist[tid] = 0;
    if (tid < ZL_NCL) s_chist[tid] = 0;
    __syncthreads();

    /* parse over the lane's segment, greedy with one step of lookahead; a token per step (literal: the byte; match: length << 16 |
     * distance - 1) */
    uint32_t rep[2] = {0, 0};
    for (uint32_t p = s0; p < s0 + seg_n;) {
      uint32_t d = 0, d1 = 0;
      uint32_t l = find_match(s_buf, scratch, p, s1, rep, &d);
      if (l && l < 32u && find_match(s_buf, scratch, p + 1u, s1, rep, &d1) > l) l = 0;
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
    rank_symbols(s_lhist, ZL_NLIT, s_lkey, s_lsym);
    rank_symbols(s_dhist, ZL_NDIST, s_dkey, s_dsym);
    __syncthreads();
    if (tid == 0) {
      huff_lengths(s_lhist, ZL_NLIT, 15, s_lkey, s_lsym, s_llen);
      canon_codes(s_llen, ZL_NLIT, s_lcode);
    } else if (tid == 64) {
      uint32_t any = 0;
      for (int s = 0; s < ZL_NDIST; s++) any |= s_dhist[s];
      if (any) huff_lengths(s_dhist, ZL_NDIST, 15, s_dkey, s_dsym, s_dlen);
      else { /* no match: one distance code of one bit, the one incomplete tree inflaters take */
        for (int s = 0; s < ZL_NDIST; s++) s_dlen[s] = 0;
        s_dlen[0] = 1;
      }
      canon_codes(s_dlen, ZL_NDIST, s_dcode);
    }
    __syncthreads();
    if (tid == 0) { /* the code lengths as code-length symbols (16: repeat the last 3-6 times, 17: 3-10 zeros, 18: 11-138 zeros) */
      int hlit = ZL_NLIT, hdist = ZL_NDIST;
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
      for (int s = 0; s < ZL_NCL; s++)
        if (s_chist[s]) used++, only = s;
      if (used == 1) s_chist[only == 0 ? 1 : 0] = 1; /* the code-length code must be complete: two symbols at least */
      s_meta[0] = (uint32_t)nr;
      s_meta[2] = (uint32_t)hlit;
      s_meta[3] = (uint32_t)hdist;
    }
    __syncthreads();
    rank_symbols(s_chist, ZL_NCL, s_ckey, s_csym);
    for (uint32_t w = tid; w < WORDS; w += ZL_LANES) s_buf[w] = 0; /* the image: the piece's bytes are in the tokens now */
    __syncthreads();
    if (tid == 0) { /* the block's header: at most 564 bytes with the two zlib bytes, whatever the piece (WORDS >= 160) */
      huff_lengths(s_chist, ZL_NCL, 7, s_ckey, s_csym, s_clen);
      canon_codes(s_clen, ZL_NCL, s_ccode);
      int hclen = ZL_NCL;
      while (hclen > 4 && !s_clen[z_clorder[hclen - 1]]) hclen--;
      hdr_writer hw{s_buf, 2u * 8u};
      hw.put(5u, 3u); /* BFINAL 1, BTYPE 10 */
      hw.put(s_meta[2] - 257u, 5u);
      hw.put(s_meta[3] - 1u, 5u);
      hw.put((uint32_t)hclen - 4u, 4u);
      for (int k = 0; k < hclen; k++) hw.put(s_clen[z_clorder[k]], 3u);
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
        bits += (s_lcode[257u + ls] >> 16) + z_lext[ls] + (s_dcode[ds] >> 16) + z_dext[ds];
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
      for (uint32_t k = 0; k < ZL_LANES; k++) {
        const uint32_t b = s_bits[k];
        s_bits[k] = at;
        at += b;
      }
      s_meta[1] = at; /* where end-of-block goes */
    }
    __syncthreads();
    const uint32_t eob_at = s_meta[1], dyn_end = eob_at + (s_lcode[256] >> 16), dyn_bytes = (dyn_end + 7u) / 8u - 2u;
    uint32_t size;
    if (dyn_bytes < len) { /* every bit lies below byte 2 + len of the buffer */
      lane_writer lw{s_buf, s_bits[tid] >> 5, s_bits[tid] & 31u, 0};
      for (uint32_t p = s0; p < s0 + seg_n;) {
        const uint32_t t = scratch[p];
        if (t >> 16) {
          const uint32_t l = t >> 16, d = (t & 0xffffu) + 1u, ls = len_sym(l), ds = dist_sym(d);
          const uint32_t lc = s_lcode[257u + ls], dc = s_dcode[ds];
          lw.put(lc & 0xffffu, lc >> 16);
          lw.put(l - z_lbase[ls], z_lext[ls]);
          lw.put(dc & 0xffffu, dc >> 16);
          lw.put(d - z_dbase[ds], z_dext[ds]);
          p += l;
        } else {
          const uint32_t lc = s_lcode[t];
          lw.put(lc & 0xffffu, lc >> 16);
          p++;
        }
      }
      if (tid == ZL_LANES - 1u) { /* (the last lane's bits end at eob_at, with or without a segment of its own) */
        const uint32_t lc = s_lcode[256];
        lw.put(lc & 0xffffu, lc >> 16);
      }
      lw.flush();
      size = 2u + dyn_bytes + 4u;
      __syncthreads();
      if (tid == 0) {
        s_bytes[0] = 0x78;
        s_bytes[1] = 0x9C;
        put_u32be(s_bytes + 2u + dyn_bytes, adler);
      }
    } else { /* stored: the piece's bytes once more, from HBM */
      size = 2u + 5u + len + 4u;
      __syncthreads();
      for (uint32_t w = tid; w < WORDS; w += ZL_LANES) s_buf[w] = 0;
      __syncthreads();
      load_piece(src + base, len, s_buf, 7u);
      if (tid == 0) {
        s_bytes[0] = 0x78;
        s_bytes[1] = 0x9C;
        s_bytes[2] = 1; /* BFINAL 1, BTYPE 00 */
        s_bytes[3] = (uint8_t)(len & 0xffu);
        s_bytes[4] = (uint8_t)(len >> 8);
        s_bytes[5] = (uint8_t)(~len & 0xffu);
        s_bytes[6] = (uint8_t)((~len >> 8) & 0xffu);
        put_u32be(s_bytes + 7u + len, adler);
      }
    }
    __syncthreads();
    uint4 *dst = (uint4 *)(slots + (size_t)m * slot); /* size <= len + 11 <= slot - 16, slot a multiple of 16 */
    const uint4 *img = (const uint4 *)s_buf;
    for (uint32_t i = tid; i * 16u < size; i += ZL_LANES) dst[i] = img[i];
    if (tid == 0) sizes[m] = size;
  }
}

} /* namespace */

extern "C" __global__ __launch_bounds__(256) void bsc_zlib_deflate_small_kernel(const uint8_t *__restrict__ src, uint64_t n, uint32_t piece, uint32_t n_pieces,
                                                                               uint8_t *__restrict__ slots, uint32_t slot, uint32_t *__restrict__ sizes,
                                                                               uint32_t *__restrict__ scratch_all) {
  zlib_deflate_body<ZL_SMALL_PIECE>(src, n, piece, n_pieces, slots, slot, sizes, scratch_all);
}
extern "C" __global__ __launch_bounds__(256) void bsc_zlib_deflate_large_kernel(const uint8_t *__restrict__ src, uint64_t n, uint32_t piece, uint32_t n_pieces,
                                                                               uint8_t *__restrict__ slots, uint32_t slot, uint32_t *__restrict__ sizes,
                                                                               uint32_t *__restrict__ scratch_all) {
  zlib_deflate_body<ZL_MAX_PIECE>(src, n, piece, n_pieces, slots, slot, sizes, scratch_all);
}

/* the same body over ranges: piece m = src[offs[m], offs[m + 1]), 1 .. piece bytes each (piece: the longest the caller allows, what slots and
 * scratch are sized for).  A range of no byte, or whose end lies before its start, gives size 0 and reads nothing; a longer one is cut at
 * `piece` bytes; *bad counts both. */
extern "C" __global__ __launch_bounds__(256) void bsc_zlib_deflate_ranges_small_kernel(const uint8_t *__restrict__ src, const unsigned long long *__restrict__ offs,
                                                                                      uint32_t piece, uint32_t n_pieces, uint8_t *__restrict__ slots,
                                                                                      uint32_t slot, uint32_t *__restrict__ sizes,
                                                                                      uint32_t *__restrict__ scratch_all, unsigned long long *bad) {
  zlib_deflate_body<ZL_SMALL_PIECE, true>(src, 0ull, piece, n_pieces, slots, slot, sizes, scratch_all, offs, bad);
}
extern "C" __global__ __launch_bounds__(256) void bsc_zlib_deflate_ranges_large_kernel(const uint8_t *__restrict__ src, const unsigned long long *__restrict__ offs,
                                                                                      uint32_t piece, uint32_t n_pieces, uint8_t *__restrict__ slots,
                                                                                      uint32_t slot, uint32_t *__restrict__ sizes,
                                                                                      uint32_t *__restrict__ scratch_all, unsigned long long *bad) {
  zlib_deflate_body<ZL_MAX_PIECE, true>(src, 0ull, piece, n_pieces, slots, slot, sizes, scratch_all, offs, bad);
}

/* offs[i] = sizes[0] + ... + sizes[i - 1], offs[n] = the total; totals = {the total, n}; one workgroup */
extern "C" __global__ __launch_bounds__(256) void bsc_zlib_scan_kernel(const uint32_t *__restrict__ sizes, unsigned long long *__restrict__ offs, uint32_t n,
                                                                      unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long s_part[ZL_LANES];
  const uint32_t per = (n + ZL_LANES - 1u) / ZL_LANES;
  const uint64_t a64 = (uint64_t)threadIdx.x * per;
  const uint32_t a = a64 < n ? (uint32_t)a64 : n, b = n - a < per ? n : a + per;
  unsigned long long t = 0;
  for (uint32_t i = a; i < b; i++) t += sizes[i];
  s_part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long at = 0;
    for (uint32_t k = 0; k < ZL_LANES; k++) {
      const unsigned long long v = s_part[k];
      s_part[k] = at;
      at += v;
    }
    offs[n] = at;
    totals[0] = at;
    totals[1] = n;
  }
  __syncthreads();
  unsigned long long at = s_part[threadIdx.x];
  for (uint32_t i = a; i < b; i++) {
    offs[i] = at;
    at += sizes[i];
  }
}

/* piece m's slot -> out[offs[m], offs[m] + sizes[m]) if out_cap holds the total; sizes -> sizes_out if sizes_cap holds n: one wave a
 * piece, whole words inside the stream, single bytes where a word is shared with a neighbour */
extern "C" __global__ __launch_bounds__(256) void bsc_zlib_gather_kernel(const uint8_t *__restrict__ slots, uint32_t slot, const unsigned long long *__restrict__ offs,
                                                                        const uint32_t *__restrict__ sizes, uint32_t n, uint8_t *__restrict__ out,
                                                                        uint64_t out_cap, uint32_t *__restrict__ sizes_out, uint64_t sizes_cap) {
  const bool out_ok = offs[n] <= out_cap, sizes_ok = n <= sizes_cap;
  const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * 4u;
  for (uint32_t m = blockIdx.x * 4u + (threadIdx.x >> 6); m < n; m += waves) {
    const uint32_t size = sizes[m];
    if (sizes_ok && lane == 0) sizes_out[m] = size;
    if (!out_ok) continue;
    const uint8_t *s = slots + (size_t)m * slot;
    const uint32_t *sw = (const uint32_t *)s;
    uint8_t *d = out + offs[m];
    const uint32_t lead = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u), h = lead < size ? lead : size;
    const uint32_t nw = (size - h) / 4u, tail = h + 4u * nw;
    if (lane < h) d[lane] = s[lane];
    if (lane < size - tail) d[tail + lane] = s[tail + lane];
    uint32_t *dw = (uint32_t *)(d + h);
    for (uint32_t j = lane; j < nw; j += 64u) {
      const uint32_t q = (h >> 2) + j; /* source word of byte h + 4 j; its neighbour lies inside the slot (16 spare bytes) */
      const uint64_t v = ((uint64_t)sw[q + 1u] << 32) | sw[q];
      dw[j] = (uint32_t)(v >> (8u * (h & 3u)));
    }
  }
}

extern "C" uint32_t bsc_dev_zlib_slot(uint32_t piece) { return ((piece + 11u + 15u) / 16u) * 16u + 16u; }
extern "C" uint32_t bsc_dev_zlib_grid(uint32_t piece, uint32_t n_pieces, int num_cus) { /* workgroups: what a CU's LDS holds at once */
  const uint64_t g = (uint64_t)(num_cus > 0 ? num_cus : 1) * (piece <= ZL_SMALL_PIECE ? 4u : 1u);
  return (uint32_t)(g < n_pieces ? g : n_pieces);
}

/* n_pieces >= 1.  scratch: grid * piece u32; slots: n_pieces * bsc_dev_zlib_slot(piece); sizes: n_pieces u32; offs: n_pieces + 1 u64 */
/* range_offs: NULL — the fixed-stride pieces of src[0 .. n) —, or n_pieces + 1 ascending device u64 — piece m = src[range_offs[m],
 * range_offs[m + 1]), `piece` the longest allowed; then totals has a third word, the count of bad ranges, zeroed here. */
static int zlib_launch(const void *src, uint64_t n, const void *range_offs, uint32_t piece, uint32_t n_pieces, void *slots, void *sizes, void *offs,
                       void *scratch, uint32_t grid, void *out, uint64_t out_cap, void *sizes_out, uint64_t sizes_cap, void *totals, int num_cus,
                       void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const uint32_t slot = bsc_dev_zlib_slot(piece);
  if (range_offs) {
    unsigned long long *bad = (unsigned long long *)totals + 2;
    const hipError_t e = hipMemsetAsync(bad, 0, sizeof *bad, s);
    if (e != hipSuccess) return (int)e;
    if (piece <= ZL_SMALL_PIECE)
      hipLaunchKernelGGL(bsc_zlib_deflate_ranges_small_kernel, dim3(grid), dim3(ZL_LANES), 0, s, (const uint8_t *)src, (const unsigned long long *)range_offs,
                         piece, n_pieces, (uint8_t *)slots, slot, (uint32_t *)sizes, (uint32_t *)scratch, bad);
    else
      hipLaunchKernelGGL(bsc_zlib_deflate_ranges_large_kernel, dim3(grid), dim3(ZL_LANES), 0, s, (const uint8_t *)src, (const unsigned long long *)range_offs,
                         piece, n_pieces, (uint8_t *)slots, slot, (uint32_t *)sizes, (uint32_t *)scratch, bad);
  } else if (piece <= ZL_SMALL_PIECE)
    hipLaunchKernelGGL(bsc_zlib_deflate_small_kernel, dim3(grid), dim3(ZL_LANES), 0, s, (const uint8_t *)src, n, piece, n_pieces, (uint8_t *)slots, slot,
                       (uint32_t *)sizes, (uint32_t *)scratch);
  else
    hipLaunchKernelGGL(bsc_zlib_deflate_large_kernel, dim3(grid), dim3(ZL_LANES), 0, s, (const uint8_t *)src, n, piece, n_pieces, (uint8_t *)slots, slot,
                       (uint32_t *)sizes, (uint32_t *)scratch);
  hipLaunchKernelGGL(bsc_zlib_scan_kernel, dim3(1), dim3(ZL_LANES), 0, s, (const uint32_t *)sizes, (unsigned long long *)offs, n_pieces,
                     (unsigned long long *)totals);
  uint32_t gg = (n_pieces + 3u) / 4u;
  const uint32_t gmax = (uint32_t)(num_cus > 0 ? num_cus : 1) * 8u;
  if (gg > gmax) gg = gmax;
  hipLaunchKernelGGL(bsc_zlib_gather_kernel, dim3(gg), dim3(ZL_LANES), 0, s, (const uint8_t *)slots, slot, (const unsigned long long *)offs,
                     (const uint32_t *)sizes, n_pieces, (uint8_t *)out, out_cap, (uint32_t *)sizes_out, sizes_cap);
  return (int)hipGetLastError();
}

extern "C" int bsc_dev_launch_zlib(const void *src, uint64_t n, uint32_t piece, uint32_t n_pieces, void *slots, void *sizes, void *offs, void *scratch,
                                   uint32_t grid, void *out, uint64_t out_cap, void *sizes_out, uint64_t sizes_cap, void *totals, int num_cus, void *stream) {
  return zlib_launch(src, n, NULL, piece, n_pieces, slots, sizes, offs, scratch, grid, out, out_cap, sizes_out, sizes_cap, totals, num_cus, stream);
}

/* as bsc_dev_launch_zlib with piece = max_piece for the workspaces; range_offs: n_pieces + 1 device u64; totals: three u64 */
extern "C" int bsc_dev_launch_zlib_ranges(const void *src, const void *range_offs, uint32_t max_piece, uint32_t n_pieces, void *slots, void *sizes, void *offs,
                                          void *scratch, uint32_t grid, void *out, uint64_t out_cap, void *sizes_out, uint64_t sizes_cap, void *totals,
                                          int num_cus, void *stream) {
  if (!range_offs) return (int)hipErrorInvalidValue;
  return zlib_launch(src, 0ull, range_offs, max_piece, n_pieces, slots, sizes, offs, scratch, grid, out, out_cap, sizes_out, sizes_cap, totals, num_cus, stream);
}
