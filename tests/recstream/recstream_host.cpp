/*
 * TEST ONLY: the index arithmetic of csrc/recstream_dev.h on the host (tests/test_recstream_host.py builds this with the host compiler
 * under AddressSanitizer + UndefinedBehaviorSanitizer and runs it).  The copy-out's ranges for every phase and span; the parts picker on
 * inclusive-prefix vectors against a plain restatement.  vcftext_emit.h is included to see that it still compiles for a host.
 */
#include <stdio.h>
#include <string.h>

#include "recstream_dev.h"
#include "vcftext_emit.h"

static int fails = 0;
#define CHECK(c, ...)                   \
  do {                                  \
    if (!(c)) {                         \
      if (fails++ < 20) {               \
        printf("FAIL %s: ", #c);        \
        printf(__VA_ARGS__);            \
        printf("\n");                   \
      }                                 \
    }                                   \
  } while (0)

/* head, body and tail are disjoint, lie inside [ph, ph + t), cover it exactly; the body is whole pieces, each touched by one lane once */
static void check_ranges(unsigned ph, unsigned t) {
  const rs_ranges c = rs_copy_ranges(ph, t);
  static unsigned char hits[16 + 2100 + 64];
  memset(hits, 0, sizeof hits);
  const unsigned room = (unsigned)sizeof hits;
  CHECK(c.end == ph + t && c.head0 == ph, "ph %u t %u", ph, t);
  CHECK(c.body0 % RS_PIECE == 0 && c.body1 % RS_PIECE == 0, "ph %u t %u: body [%u, %u)", ph, t, c.body0, c.body1);
  for (unsigned lane = 0; lane < RS_LANES; lane++) { /* rs_copy_out's three statements, a lane at a time */
    if (lane >= c.head0 && lane < c.head_end) hits[lane]++;
    for (unsigned o = c.body0 + RS_PIECE * lane; o < c.body1; o += RS_PIECE * RS_LANES) {
      CHECK(o + RS_PIECE <= room, "ph %u t %u: piece at %u", ph, t, o);
      if (o + RS_PIECE <= room)
        for (unsigned k = 0; k < RS_PIECE; k++) hits[o + k]++;
    }
    if (c.tail0 + lane < c.end) hits[c.tail0 + lane]++;
  }
  for (unsigned o = 0; o < room; o++) {
    const unsigned want = (o >= ph && o < ph + t) ? 1u : 0u;
    if (hits[o] != want) {
      CHECK(hits[o] == want, "ph %u t %u: byte %u written %u times", ph, t, o, (unsigned)hits[o]);
      break;
    }
  }
  /* the ranges as intervals: in order, no overlap, nothing missing (an empty range may stand anywhere) */
  unsigned at = ph;
  const unsigned iv[3][2] = {{c.head0, c.head_end}, {c.body0, c.body1}, {c.tail0, c.end}};
  for (int k = 0; k < 3; k++) {
    if (iv[k][0] >= iv[k][1]) continue;
    CHECK(iv[k][0] == at, "ph %u t %u: range %d starts at %u, expected %u", ph, t, k, iv[k][0], at);
    at = iv[k][1];
  }
  CHECK(at == ph + t, "ph %u t %u: the ranges end at %u", ph, t, at);
  CHECK(c.end - c.tail0 < RS_LANES || c.tail0 >= c.end, "ph %u t %u: a tail of %u bytes, a byte per lane", ph, t, c.end - c.tail0);
}

struct inc_of {
  const unsigned *inc;
  unsigned operator()(unsigned l) const { return inc[l]; }
};

/* the fewest power-of-two part count whose every part fits, MAX_PARTS when none below it does */
static unsigned plain_parts(const unsigned *len, unsigned img, unsigned max_parts, bool *all_fit) {
  for (unsigned parts = 1;; parts <<= 1) {
    bool fits = true;
    for (unsigned q = 0; q < parts; q++) {
      unsigned sum = 0;
      for (unsigned l = q * (64u / parts); l < (q + 1u) * (64u / parts); l++) sum += len[l];
      fits = fits && sum <= img;
    }
    if (fits || parts == max_parts) {
      *all_fit = fits;
      return parts;
    }
  }
}

template <unsigned IMG, unsigned MAX_PARTS>
static void check_pick(const unsigned *len, unsigned rec_max, const char *what) {
  unsigned inc[64], sum = 0, longest = 0;
  for (unsigned l = 0; l < 64u; l++) {
    inc[l] = (sum += len[l]);
    longest = len[l] > longest ? len[l] : longest;
  }
  bool all_fit;
  const unsigned want = plain_parts(len, IMG, MAX_PARTS, &all_fit);
  const unsigned got = rs_pick_parts_at<IMG, MAX_PARTS>(inc_of{inc});
  CHECK(got == want, "%s, image %u, at most %u parts: %u parts, expected %u", what, IMG, MAX_PARTS, got, want);
  if (longest <= rec_max && (64u / MAX_PARTS) * rec_max <= IMG) CHECK(all_fit, "%s, image %u: a part of %u parts exceeds the image", what, IMG, want);
}

template <unsigned IMG, unsigned MAX_PARTS>
static void check_picker(unsigned rec_max) {
  unsigned len[64];
  for (unsigned v = 0; v <= rec_max; v++) { /* all equal */
    for (unsigned l = 0; l < 64u; l++) len[l] = v;
    check_pick<IMG, MAX_PARTS>(len, rec_max, "all equal");
  }
  for (unsigned base = 0; base <= rec_max; base += rec_max / 7u) /* one long lane */
    for (unsigned at = 0; at < 64u; at++) {
      for (unsigned l = 0; l < 64u; l++) len[l] = l == at ? rec_max : base;
      check_pick<IMG, MAX_PARTS>(len, rec_max, "one long lane");
    }
  for (unsigned lng = 0; lng <= rec_max; lng += 5u) /* long first half, short second half — and the other way round */
    for (unsigned sht = 0; sht <= lng; sht += 37u) {
      for (unsigned l = 0; l < 64u; l++) len[l] = l < 32u ? lng : sht;
      check_pick<IMG, MAX_PARTS>(len, rec_max, "long first half");
      for (unsigned l = 0; l < 64u; l++) len[l] = l < 32u ? sht : lng;
      check_pick<IMG, MAX_PARTS>(len, rec_max, "long second half");
    }
}

int main(void) {
  for (unsigned ph = 0; ph < 16u; ph++)
    for (unsigned t = 0; t <= 2100u; t++) check_ranges(ph, t);
  check_picker<8192u, 8u>(336u);   /* the BCF encoder's image and longest record */
  check_picker<12288u, 16u>(665u); /* the text encoder's image and longest line */
  check_picker<2688u, 8u>(336u);   /* the smallest images the encoders' static_asserts allow: the last rung is reached */
  check_picker<2672u, 16u>(665u);
  { /* vcftext_emit.h on the host: one emitter over its two sinks */
    vt_rec r;
    memset(&r, 0, sizeof r);
    r.w[0] = 123456789u;
    r.w[1] = 0x00002401u; /* emit, gt 0x24 >> .. : any record will do */
    uint32_t contig_w[64] = {0};
    memcpy(contig_w, "chr1\t", 5);
    bool clamped;
    vt_count_sink c = {0u};
    vt_emit_line(c, r, contig_w, 5u, nullptr, 0u, clamped);
    uint8_t line[VT_LINE_MAX + 16];
    vt_write_sink w = {line, 0u};
    vt_emit_line(w, r, contig_w, 5u, nullptr, 0u, clamped);
    CHECK(c.len == w.len && w.len > 40u && line[w.len - 1u] == '\n' && !memcmp(line, "chr1\t123456789\t.\t", 17), "the emitter on the host: %u / %u bytes", c.len, w.len);
  }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
