/*
 * tabix_int.h — the seam between the index writer (tabix.c: host code alone, so that it builds stand-alone under the sanitizers) and the
 * BGZF writer (bscall_api.c), whose fields the index of a file that is being compressed on the device needs: its logical length when a
 * block is added, its members' sizes when it closes.  Not part of the C ABI.
 */
#ifndef BSC_TABIX_INT_H
#define BSC_TABIX_INT_H
#include <stdint.h>

#include "../../include/bscall_amd.h"

int bsc_tbx_make_(const char *who, int kind, int min_shift, int n_refs, const char *const *names, const uint32_t *lens, bsc_tbx **out);
/* writer: passed back to logical (the writer's logical length now) and to unbind (bsc_tbx_close while the writer is open) */
void bsc_tbx_bind_(bsc_tbx *ix, void *writer, uint64_t (*logical)(void *), void (*unbind)(void *));
void bsc_tbx_writer_closed_(bsc_tbx *ix, int rc, const uint64_t *msize, uint64_t n_msize, uint64_t logical);

#endif
