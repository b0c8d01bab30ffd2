/*
 * ref_stub_sam.h — what the reference's sources need of <htslib/sam.h>, written by us from the BAM record's field list (SAM
 * specification 4.2).  *** TEST INFRASTRUCTURE. ***  oracle/Makefile (target `ref`) copies this file to
 * _ref/stub/htslib/sam.h, where the reference's unchanged files find it; there is no htslib on the machines this is built on.
 *
 * The calc path uses htslib for pointer types only: those stay opaque.  src/input_sam.c reads one alignment record: the record
 * type is complete, with the fields, flag values and accessors that file names and nothing else.  sam_read1 / sam_itr_next are
 * declared here and DEFINED by oracle/ref_driver.c, which hands over the records of a caller's buffer.
 */
#ifndef BSC_REF_STUB_SAM_H
#define BSC_REF_STUB_SAM_H

#include <stdint.h>

typedef struct bam_hdr_t bam_hdr_t;
typedef struct htsFile htsFile;
typedef struct hts_idx_t hts_idx_t;
typedef struct hts_itr_t hts_itr_t;

#define FT_UNKN 0
#define FT_GZ 1
#define FT_VCF 2
#define FT_VCF_GZ 3
#define FT_BCF 4
#define FT_BCF_GZ 5

/* the 32 fixed bytes of an alignment record: refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID,
 * next_pos, tlen */
typedef struct {
  int32_t tid;
  int32_t pos;
  uint16_t bin;
  uint8_t qual;
  uint8_t l_qname;
  uint16_t flag;
  uint16_t n_cigar;
  int32_t l_qseq;
  int32_t mtid;
  int32_t mpos;
  int32_t isize;
} bam1_core_t;

/* data: read name (l_qname bytes), CIGAR (n_cigar dwords), 4-bit bases ((l_qseq + 1) / 2 bytes), qualities (l_qseq bytes),
 * optional fields up to l_data */
typedef struct {
  bam1_core_t core;
  int l_data;
  uint32_t m_data;
  uint8_t *data;
} bam1_t;

#define BAM_FPAIRED 1
#define BAM_FPROPER_PAIR 2
#define BAM_FUNMAP 4
#define BAM_FMUNMAP 8
#define BAM_FREVERSE 16
#define BAM_FREAD2 128
#define BAM_FSECONDARY 256
#define BAM_FQCFAIL 512
#define BAM_FDUP 1024
#define BAM_FSUPPLEMENTARY 2048

#define bam_get_cigar(b) ((uint32_t *)((b)->data + (b)->core.l_qname))
#define bam_get_seq(b) ((b)->data + ((b)->core.n_cigar << 2) + (b)->core.l_qname)
#define bam_get_qual(b) ((b)->data + ((b)->core.n_cigar << 2) + (b)->core.l_qname + (((b)->core.l_qseq + 1) >> 1))
#define bam_get_aux(b) ((b)->data + ((b)->core.n_cigar << 2) + (b)->core.l_qname + (((b)->core.l_qseq + 1) >> 1) + (b)->core.l_qseq)

/* operation codes 0..8 are M I D N S H P = X, 9 is B (SAM specification 4.2); 10..15 are not assigned */
#define bam_cigar_op(c) ((c) & 0xfu)
#define bam_cigar_oplen(c) ((c) >> 4)
#define bam_cigar_opchr(c) ("MIDNSHP=XB??????"[bam_cigar_op(c)])

int sam_read1(htsFile *fp, bam_hdr_t *h, bam1_t *b);
int sam_itr_next(htsFile *fp, hts_itr_t *itr, bam1_t *b);

#endif
