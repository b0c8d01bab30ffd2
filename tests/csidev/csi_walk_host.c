/*
 * csi_walk_host.c — TEST ONLY: the record walk of the CSI scan (csrc/csidev_core.h) on the CPU, the way the kernels of csrc/csidev.hip run
 * it: a counting pass per interval, an exclusive prefix sum, a writing pass into entries[cap].  Built stand-alone under AddressSanitizer +
 * UndefinedBehaviorSanitizer (make csi-walk-host; tests/test_csi_host.py builds its own copy): the stream and the entries live in heap
 * blocks of exactly their size, so a read behind the stream or an entry behind the capacity stops the program.
 *
 *   csi_walk_host bcf|vcf min_shift cap stream-file offsets-file|-
 *
 * offsets-file: the interval offsets, one decimal number a line (n_sync + 1 of them); "-": one interval, the whole stream.
 * Prints "window n_records u_beg" per entry written, then "entries E records R err B".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "csidev_core.h"

int main(int argc, char **argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s bcf|vcf min_shift cap stream-file offsets-file|-\n", argv[0]);
    return 2;
  }
  const int format = !strcmp(argv[1], "vcf") ? CSI_FMT_VCF : CSI_FMT_BCF, min_shift = atoi(argv[2]);
  const uint64_t cap = strtoull(argv[3], NULL, 10);
  FILE *f = fopen(argv[4], "rb");
  if (!f) {
    perror(argv[4]);
    return 1;
  }
  fseek(f, 0, SEEK_END);
  const uint64_t n_bytes = (uint64_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *s = malloc(n_bytes ? n_bytes : 1);
  if (n_bytes && fread(s, 1, n_bytes, f) != n_bytes) return 1;
  fclose(f);
  uint64_t *sync = NULL, n_sync = 1;
  if (strcmp(argv[5], "-")) {
    FILE *g = fopen(argv[5], "r");
    if (!g) {
      perror(argv[5]);
      return 1;
    }
    uint64_t capo = 16, n = 0;
    unsigned long long v;
    sync = malloc(capo * 8);
    while (fscanf(g, "%llu", &v) == 1) {
      if (n == capo) sync = realloc(sync, (capo *= 2) * 8);
      sync[n++] = v;
    }
    fclose(g);
    n_sync = n ? n - 1 : 0;
    if (n_sync) { /* exactly its size, so that sync[n_sync + 1] is caught */
      uint64_t *t = malloc((n_sync + 1) * 8);
      memcpy(t, sync, (n_sync + 1) * 8);
      free(sync);
      sync = t;
    }
  }
  uint64_t *off = calloc(n_sync + 1, 8);
  uint32_t records = 0, err = 0;
  for (uint64_t i = 0; i < n_sync; i++) {
    const uint64_t beg = sync ? sync[i] : 0, end = sync ? sync[i + 1] : n_bytes;
    uint32_t runs = 0;
    if (beg <= end && end <= n_bytes) runs = csi_walk(format, s, beg, end, min_shift, NULL, 0, 0, &records, &err);
    else err |= CSI_ERR_INTERVAL;
    off[i + 1] = off[i] + runs;
  }
  csi_run *ent = malloc(cap ? cap * sizeof *ent : 1);
  for (uint64_t i = 0; i < n_sync; i++) {
    const uint64_t beg = sync ? sync[i] : 0, end = sync ? sync[i + 1] : n_bytes;
    uint32_t r2 = 0, e2 = 0;
    if (off[i + 1] == off[i] || !(beg <= end && end <= n_bytes)) continue;
    if (csi_walk(format, s, beg, end, min_shift, ent, off[i], cap, &r2, &e2) != off[i + 1] - off[i]) {
      printf("the two passes disagree on interval %llu\n", (unsigned long long)i);
      return 1;
    }
  }
  const uint64_t total = off[n_sync];
  for (uint64_t k = 0; k < total && k < cap; k++) printf("%u %u %llu\n", ent[k].window, ent[k].n_records, (unsigned long long)ent[k].u_beg);
  printf("entries %llu records %u err %u\n", (unsigned long long)total, records, err);
  free(ent);
  free(off);
  free(sync);
  free(s);
  return 0;
}
