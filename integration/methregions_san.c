/*
 * methregions_san.c — the BED reader and the formatter of the per-region methylation summary (bs_call_amd/csrc/methregions.c) under
 * AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program of that one file, on the CPU (make methregions-san).  The reader
 * takes untrusted text; every case is handed over in a heap block of exactly its length, so that a read one byte beyond it is seen.
 * Prints "ok" and returns 0, or names the case that went wrong.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bscall_amd.h>

static char errbuf[512];
int bsc_set_error(int code, const char *fmt, ...) { /* the library's own lives in bscall_api.c */
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(errbuf, sizeof errbuf, fmt, ap);
  va_end(ap);
  return code;
}

static int failures;
#define EXPECT(cond, what)                                        \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "FAILED: %s (%s:%d)\n", what, __FILE__, __LINE__); \
      failures++;                                                 \
    }                                                             \
  } while (0)

static int parse(const char *text, size_t len, bsc_meth_bed **out) {
  char *exact = malloc(len ? len : 1); /* no terminator behind it */
  memcpy(exact, text, len);
  errbuf[0] = 0;
  const int rc = bsc_meth_regions_parse_bed(len ? exact : NULL, len, out);
  free(exact);
  return rc;
}

static void refused(const char *text, const char *line_tag, const char *what) {
  bsc_meth_bed *bed = (bsc_meth_bed *)1;
  const int rc = parse(text, strlen(text), &bed);
  EXPECT(rc == BSC_ERR_ARG && bed == NULL, what);
  EXPECT(strstr(errbuf, line_tag) != NULL, what);
}

int main(void) {
  /* well-formed: comment, track and browser lines, CRLF, space separation, a missing name, more than four columns, duplicates */
  static const char good[] =
      "# a comment\n"
      "track name=x\n"
      "browser position chr1:1-100\r\n"
      "\n"
      "\r\n"
      "chr1\t100\t200\tsecond\t0\t+\n"
      "chr2 5 9 spaced\n"
      "chr1\t100\t200\tthird\r\n"
      "chr1\t0\t4294967295\n"
      "chr1\t100\t150\t\n"
      "chr2\t7\t7\tempty region\textra\tcolumns\there\n"
      "chr1\t100\t200\tfourth\n";
  bsc_meth_bed *bed = NULL;
  EXPECT(parse(good, sizeof good - 1, &bed) == BSC_OK && bed, "the well-formed file");
  if (bed) {
    EXPECT(bed->n_contigs == 2 && bed->n_regions == 7, "counts");
    EXPECT(!strcmp(bed->contigs[0], "chr1") && !strcmp(bed->contigs[1], "chr2"), "contigs in order of first appearance");
    EXPECT(bed->first[0] == 0 && bed->first[1] == 5 && bed->first[2] == 7, "first");
    static const uint32_t st[7] = {0, 100, 100, 100, 100, 5, 7}, en[7] = {4294967295u, 150, 200, 200, 200, 9, 7};
    static const char *const nm[7] = {".", ".", "second", "third", "fourth", "spaced", "empty region"};
    for (int k = 0; k < 7; k++)
      EXPECT(bed->regions[k].start == st[k] && bed->regions[k].end == en[k] && !strcmp(bed->names[k], nm[k]), "sorted stably by (start, end)");
    /* the formatter over the first contig: sites == 0, sums above 2^32 */
    uint64_t acc[5][4] = {{0, 0, 0, 0}, {1, 1, 0, 100}, {3, 3ull * 4294967295ull, 5, 250}, {2, 0, 9, 0}, {7, 1ull << 40, 1ull << 41, 231}};
    const long need = bsc_meth_regions_format("chr1", bed->regions, (const char *const *)bed->names, &acc[0][0], 5, NULL, 0);
    EXPECT(need > 0, "the length");
    char *buf = malloc((size_t)need);
    EXPECT(bsc_meth_regions_format("chr1", bed->regions, (const char *const *)bed->names, &acc[0][0], 5, buf, (size_t)need - 1) == need, "too little room");
    EXPECT(bsc_meth_regions_format("chr1", bed->regions, (const char *const *)bed->names, &acc[0][0], 5, buf, (size_t)need) == need, "the bytes");
    static const char want[] =
        "chr1\t0\t4294967295\t.\t0\t0\t0\t0\t.\t.\n"
        "chr1\t100\t150\t.\t1\t1\t1\t0\t100\t100\n"
        "chr1\t100\t200\tsecond\t3\t12884901890\t12884901885\t5\t100\t83\n"
        "chr1\t100\t200\tthird\t2\t9\t0\t9\t0\t0\n"
        "chr1\t100\t200\tfourth\t7\t3298534883328\t1099511627776\t2199023255552\t33\t33\n";
    EXPECT((size_t)need == sizeof want - 1 && !memcmp(buf, want, (size_t)need), "the formatter's lines");
    free(buf);
    EXPECT(bsc_meth_regions_format("chr1", bed->regions, NULL, &acc[0][0], 1, NULL, 0) == (long)strlen("chr1\t0\t4294967295\t.\t0\t0\t0\t0\t.\t.\n"), "no names");
    EXPECT(bsc_meth_regions_format("", bed->regions, NULL, &acc[0][0], 1, NULL, 0) < 0, "an empty contig");
    EXPECT(bsc_meth_regions_format("a\tb", bed->regions, NULL, &acc[0][0], 1, NULL, 0) < 0, "a tab in the contig");
    /* the sum over packed records */
    bsc_vcf_rec recs[3];
    memset(recs, 0, sizeof recs);
    for (int i = 0; i < 3; i++) {
      recs[i].core.pos = (uint32_t)(100 + i * 50);
      recs[i].core.emit = 1;
      recs[i].core.gt = i == 1 ? 7 : 4;
      recs[i].core.cg = 'C';
      recs[i].counts[5] = 0xffffffffu;
      recs[i].counts[6] = 3;
      recs[i].counts[4] = 1;
    }
    const bsc_meth_params par = {BSC_METH_CPG, 1, 0, 0};
    uint64_t sum[5][4];
    memset(sum, 0, sizeof sum);
    EXPECT(bsc_meth_regions_sum_recs(recs, 3, &par, bed->regions, 5, &sum[0][0]) == BSC_OK, "the sum");
    EXPECT(sum[0][0] == 3 && sum[0][1] == 2ull * 0xffffffffull + 3 && sum[0][2] == 1 && sum[0][3] == 275, "the whole-contig region");
    EXPECT(sum[1][0] == 1 && sum[1][1] == 3 && sum[2][0] == 2 && sum[2][1] == 0xffffffffull + 3, "(100, 150] and (100, 200]");
    bsc_meth_bed_free(bed);
  }
  /* empty input, and input that is skipped whole */
  bed = NULL;
  EXPECT(parse("", 0, &bed) == BSC_OK && bed && bed->n_regions == 0 && bed->n_contigs == 0, "empty text");
  bsc_meth_bed_free(bed);
  bed = NULL;
  EXPECT(parse("#x\n\ntrack\n", 10, &bed) == BSC_OK && bed && bed->n_regions == 0, "comments only");
  bsc_meth_bed_free(bed);
  bsc_meth_bed_free(NULL);
  /* malformed, each with its line number */
  refused("chr1\t1\t2\nchr1\t5\n", "line 2", "fewer than three columns");
  refused("chr1\n", "line 1", "one column");
  refused("#c\nchr1\t1x\t2\n", "line 2", "a coordinate that is not all digits");
  refused("chr1\t-1\t2\n", "line 1", "a sign");
  refused("chr1\t1\t\n", "line 1", "an empty coordinate");
  refused("chr1\t1\t2\n\nchr1\t1\t4294967296\n", "line 3", "a coordinate of 2^32");
  refused("chr1\t1\t99999999999999999999999\n", "line 1", "a coordinate of many digits");
  refused("chr1\t9\t8\n", "line 1", "start > end");
  refused("\t1\t2\n", "line 1", "an empty contig name");
  refused(" 1 2\n", "line 1", "an empty contig name, spaces");
  refused("chr1\t1\t2\nchr1\t3\t4", "line 2", "a final line without a newline");
  refused("chr1  1 2\n", "line 1", "two spaces are an empty column");
  EXPECT(bsc_meth_regions_parse_bed(NULL, 5, &bed) == BSC_ERR_ARG && bsc_meth_regions_parse_bed("x", 1, NULL) == BSC_ERR_ARG, "NULL arguments");
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
