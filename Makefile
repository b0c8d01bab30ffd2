# Builds libbscall_amd.so (gfx950 kernels + C host code) in-tree, and the CPU oracle used by the tests.
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
CC ?= gcc
ARCH ?= gfx950
CSRC = bs_call_amd/csrc
LIBDIR = bs_call_amd/lib

# -ffp-contract=off: the reference's arithmetic has no fused operations (x86-64 baseline build); every
# fused multiply-add in the kernels is an explicit __builtin_fma in bsmath.h.
HIPFLAGS = -O3 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -fno-fast-math -std=c++17 -Wall -Wno-unused-function -Wno-inline-asm
CFLAGS = -O2 -fPIC -Wall -ffp-contract=off -std=gnu11 -I$(ROCM)/include -D__HIP_PLATFORM_AMD__

all: $(LIBDIR)/libbscall_amd.so oracle demo devmath-probe

$(LIBDIR)/kernels.o: $(CSRC)/kernels.hip $(CSRC)/callmath.h $(CSRC)/call_body.inc $(CSRC)/call_summary.inc $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h $(CSRC)/devtables.h $(CSRC)/synth.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/bscall_api.o: $(CSRC)/bscall_api.c $(CSRC)/dbsnpdev_core.h $(CSRC)/tabix_int.h include/bscall_amd.h $(CSRC)/bsmath_tables.h $(CSRC)/devtables.h $(CSRC)/synth.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/accumulate.o: $(CSRC)/accumulate.hip $(CSRC)/accdev.h $(CSRC)/devtables.h $(CSRC)/call_summary.inc
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# rocPRIM's device radix sort (ROCm's primitive library): orders a block's templates by leftmost position
$(LIBDIR)/sort.o: $(CSRC)/sort.hip
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Wno-deprecated-declarations -c $< -o $@

$(LIBDIR)/vcfcore.o: $(CSRC)/vcfcore.hip $(CSRC)/devtables.h $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/sitestats.o: $(CSRC)/sitestats.hip $(CSRC)/sitestats_dev.h $(CSRC)/devtables.h $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/fused.o: $(CSRC)/fused.hip $(CSRC)/accdev.h $(CSRC)/callmath.h $(CSRC)/call_body.inc $(CSRC)/call_summary.inc $(CSRC)/sitestats_dev.h $(CSRC)/devtables.h $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Wno-unused-variable -c $< -o $@

$(LIBDIR)/prepdev.o: $(CSRC)/prepdev.hip include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/bcfdev.o: $(CSRC)/bcfdev.hip $(CSRC)/recstream_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/vcftextdev.o: $(CSRC)/vcftextdev.hip $(CSRC)/vcftext_emit.h $(CSRC)/fmtg_dev.h $(CSRC)/recstream_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/methdev.o: $(CSRC)/methdev.hip $(CSRC)/recstream_dev.h $(CSRC)/methtext_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/methregionsdev.o: $(CSRC)/methregionsdev.hip include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/bigwigdev.o: $(CSRC)/bigwigdev.hip $(CSRC)/bigwig_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/bwcovdev.o: $(CSRC)/bwcovdev.hip $(CSRC)/bigwig_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/bigbeddev.o: $(CSRC)/bigbeddev.hip $(CSRC)/recstream_dev.h $(CSRC)/methtext_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/bgzfdev.o: $(CSRC)/bgzfdev.hip
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/zlibdev.o: $(CSRC)/zlibdev.hip
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/dbsnpdev.o: $(CSRC)/dbsnpdev.hip $(CSRC)/dbsnpdev_core.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/csidev.o: $(CSRC)/csidev.hip $(CSRC)/csidev_core.h $(CSRC)/recstream_dev.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/beddev.o: $(CSRC)/beddev.hip $(CSRC)/bedidx_core.h $(CSRC)/recstream_dev.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/variantsdev.o: $(CSRC)/variantsdev.hip include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/cpgreadsdev.o: $(CSRC)/cpgreadsdev.hip $(CSRC)/cpgreads_dev.h $(CSRC)/recstream_dev.h $(CSRC)/methtext_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/mbiasdev.o: $(CSRC)/mbiasdev.hip include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/epidev.o: $(CSRC)/epidev.hip $(CSRC)/cpgreads_dev.h $(CSRC)/recstream_dev.h $(CSRC)/methtext_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/patdev.o: $(CSRC)/patdev.hip $(CSRC)/cpgreads_dev.h $(CSRC)/recstream_dev.h $(CSRC)/methtext_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/fragdev.o: $(CSRC)/fragdev.hip $(CSRC)/cpgreads_dev.h $(CSRC)/recstream_dev.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/asmdev.o: $(CSRC)/asmdev.hip $(CSRC)/cpgreads_dev.h $(CSRC)/recstream_dev.h $(CSRC)/methtext_dev.h $(CSRC)/callmath.h $(CSRC)/devtables.h $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/probe.o: $(CSRC)/probe.hip
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/compact.o: $(CSRC)/compact.hip include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/vcf_format.o: $(CSRC)/vcf_format.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/methbed.o: $(CSRC)/methbed.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/methcpg.o: $(CSRC)/methcpg.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/methregions.o: $(CSRC)/methregions.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/bigwig.o: $(CSRC)/bigwig.c $(CSRC)/bbi_trees.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/bigbed.o: $(CSRC)/bigbed.c $(CSRC)/bbi_trees.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/variants.o: $(CSRC)/variants.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/epi.o: $(CSRC)/epi.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/pat.o: $(CSRC)/pat.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/frag.o: $(CSRC)/frag.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/cpgreads.o: $(CSRC)/cpgreads.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/mbias.o: $(CSRC)/mbias.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/asm.o: $(CSRC)/asm.c $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/tabix.o: $(CSRC)/tabix.c $(CSRC)/tabix_int.h $(CSRC)/bedidx_core.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/dbsnp.o: $(CSRC)/dbsnp.c $(CSRC)/dbsnpdev_core.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/prep.o: $(CSRC)/prep.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/report.o: $(CSRC)/report.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/bcf.o: $(CSRC)/bcf.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/bamio.o: $(CSRC)/bamio.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/bamstream.o: $(CSRC)/bamstream.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/inflate_fast.o: $(CSRC)/inflate_fast.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -O3 -c $< -o $@

$(LIBDIR)/bamdev.o: $(CSRC)/bamdev.hip $(CSRC)/bamdev_core.h include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -Wno-deprecated-declarations -c $< -o $@

$(LIBDIR)/refseq.o: $(CSRC)/refseq.c include/bscall_amd.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/synth_reads.o: $(CSRC)/synth_reads.c include/bscall_amd.h $(CSRC)/synth.h
	@mkdir -p $(LIBDIR)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIBDIR)/libbscall_amd.so: $(LIBDIR)/kernels.o $(LIBDIR)/fused.o $(LIBDIR)/accumulate.o $(LIBDIR)/sort.o $(LIBDIR)/vcfcore.o $(LIBDIR)/sitestats.o $(LIBDIR)/compact.o $(LIBDIR)/probe.o $(LIBDIR)/prepdev.o $(LIBDIR)/bcfdev.o $(LIBDIR)/vcftextdev.o $(LIBDIR)/methdev.o $(LIBDIR)/methregionsdev.o $(LIBDIR)/bigwigdev.o $(LIBDIR)/bwcovdev.o $(LIBDIR)/bigbeddev.o $(LIBDIR)/bgzfdev.o $(LIBDIR)/zlibdev.o $(LIBDIR)/bamdev.o $(LIBDIR)/dbsnpdev.o $(LIBDIR)/csidev.o $(LIBDIR)/beddev.o $(LIBDIR)/variantsdev.o $(LIBDIR)/cpgreadsdev.o $(LIBDIR)/asmdev.o $(LIBDIR)/mbiasdev.o $(LIBDIR)/epidev.o $(LIBDIR)/patdev.o $(LIBDIR)/fragdev.o $(LIBDIR)/bscall_api.o $(LIBDIR)/bamstream.o $(LIBDIR)/inflate_fast.o $(LIBDIR)/synth_reads.o $(LIBDIR)/vcf_format.o $(LIBDIR)/methbed.o $(LIBDIR)/methcpg.o $(LIBDIR)/methregions.o $(LIBDIR)/bigwig.o $(LIBDIR)/bigbed.o $(LIBDIR)/tabix.o $(LIBDIR)/variants.o $(LIBDIR)/cpgreads.o $(LIBDIR)/asm.o $(LIBDIR)/mbias.o $(LIBDIR)/epi.o $(LIBDIR)/pat.o $(LIBDIR)/frag.o $(LIBDIR)/dbsnp.o $(LIBDIR)/prep.o $(LIBDIR)/report.o $(LIBDIR)/bcf.o $(LIBDIR)/bamio.o $(LIBDIR)/refseq.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lm -lz -lpthread

oracle:
	$(MAKE) -C oracle liboracle.so

# TEST ONLY: the device numeric primitives (callmath.h, bsmath.h, sitestats_dev.h) one call per lane, for
# tests/test_gpu_devmath.py.  The product's own headers and exactly the product's $(HIPFLAGS) (-ffp-contract=off is part of
# what is tested); nothing of it goes into libbscall_amd.so.  DEVMATH_INC: where the headers are taken from (a mutated copy,
# to see that the tests catch a change); DEVMATH_SO: where the library goes.
DEVMATH_INC ?= $(CSRC)
DEVMATH_SO ?= tests/devmath/libdevmath_probe.so
devmath-probe: $(DEVMATH_SO)
$(DEVMATH_SO): tests/devmath/devmath_probe.hip $(CSRC)/callmath.h $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h $(CSRC)/sitestats_dev.h $(CSRC)/devtables.h include/bscall_amd.h
	$(HIPCC) $(HIPFLAGS) -I$(DEVMATH_INC) -shared -o $@ $<

# TEST ONLY: the flat form of a loaded dbSNP contig and the statements the kernels of dbsnpdev.hip read it with (dbsnpdev_core.h), on the CPU —
# a stand-alone program of csrc/dbsnp.c under AddressSanitizer + UndefinedBehaviorSanitizer; tests/test_dbsnp_flat_host.py builds its own copy
# and runs it on indexes it writes: $(DBSNP_FLAT_EXE) index contig...
DBSNP_FLAT_EXE ?= tests/dbsnpdev/dbsnp_flat_host
dbsnp-flat-host: $(DBSNP_FLAT_EXE)
$(DBSNP_FLAT_EXE): tests/dbsnpdev/dbsnp_flat_host.c $(CSRC)/dbsnp.c $(CSRC)/dbsnpdev_core.h include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -I$(CSRC) $< $(CSRC)/dbsnp.c -lz -o $@

# TEST ONLY: the record walk of the CSI scan (csidev_core.h: the statements the kernels of csidev.hip run per interval) on the CPU, a stand-alone
# program under AddressSanitizer + UndefinedBehaviorSanitizer; tests/test_csi_host.py builds its own copy and runs it on streams it writes:
# $(CSI_WALK_EXE) bcf|vcf min_shift stream-file offsets-file  ->  the entries, the records and the error bits as text
CSI_WALK_EXE ?= tests/csidev/csi_walk_host
csi-walk-host: $(CSI_WALK_EXE)
$(CSI_WALK_EXE): tests/csidev/csi_walk_host.c $(CSRC)/csidev_core.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) $< -o $@

# TEST ONLY: the BED reader and the formatter of the per-region methylation summary (csrc/methregions.c) — untrusted text in — as a stand-alone
# program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU; tests/test_methregions_host.py builds its own copy and runs it:
# $(METHREGIONS_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
METHREGIONS_SAN_EXE ?= $(LIBDIR)/methregions_san
methregions-san: $(METHREGIONS_SAN_EXE)
$(METHREGIONS_SAN_EXE): integration/methregions_san.c $(CSRC)/methregions.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/methregions.c -o $@

# TEST ONLY: the writer of the bigWig file (csrc/bigwig.c: bsc_bigwig_open / _add / _finish over crafted entries — 0, 1, 256, 257 and 65 537
# sections; 1, 2, 256, 257 and 300 contigs) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU;
# tests/test_bigwig_host.py builds its own copy and runs it: $(BIGWIG_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
BIGWIG_SAN_EXE ?= $(LIBDIR)/bigwig_san
bigwig-san: $(BIGWIG_SAN_EXE)
$(BIGWIG_SAN_EXE): integration/bigwig_san.c $(CSRC)/bigwig.c $(CSRC)/bbi_trees.h include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/bigwig.c -lpthread -lz -o $@

# TEST ONLY: the compressed writer (bsc_bigwig_add_z, and bsc_bigwig_finish deflating the zoom blocks) as a stand-alone program under
# AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU; tests/test_bigwig_z_host.py builds its own copy and runs it:
# $(BIGWIG_Z_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
BIGWIG_Z_SAN_EXE ?= $(LIBDIR)/bigwig_z_san
bigwig-z-san: $(BIGWIG_Z_SAN_EXE)
$(BIGWIG_Z_SAN_EXE): integration/bigwig_z_san.c $(CSRC)/bigwig.c $(CSRC)/bbi_trees.h include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/bigwig.c -lpthread -lz -o $@

# TEST ONLY: the coverage track on the host (csrc/bigwig.c: bsc_bigwig_cov_sections_recs with its rooms, a coverage writer over crafted entries,
# plain and compressed, sums of squares beyond 2^64, the integer-to-float roundings, every refusal) as a stand-alone program under
# AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU; tests/test_bigwig_cov_host.py builds its own copy and runs it:
# $(BIGWIG_COV_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
BIGWIG_COV_SAN_EXE ?= $(LIBDIR)/bigwig_cov_san
bigwig-cov-san: $(BIGWIG_COV_SAN_EXE)
$(BIGWIG_COV_SAN_EXE): integration/bigwig_cov_san.c $(CSRC)/bigwig.c $(CSRC)/bbi_trees.h include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/bigwig.c -lpthread -lz -o $@

# TEST ONLY: the host form of the bigBed items (csrc/bigbed.c over csrc/methbed.c: the shortest and the longest item, rooms one short, block and
# window borders) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU; tests/test_bigbed_host.py builds
# its own copy and runs it: $(BIGBED_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
BIGBED_SAN_EXE ?= $(LIBDIR)/bigbed_san
bigbed-san: $(BIGBED_SAN_EXE)
$(BIGBED_SAN_EXE): integration/bigbed_san.c $(CSRC)/bigbed.c $(CSRC)/bbi_trees.h $(CSRC)/methbed.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/bigbed.c $(CSRC)/methbed.c -lz -o $@

# TEST ONLY: the writer of the tables' index and the host form of the device scan (csrc/tabix.c over csrc/bedidx_core.h: crafted and damaged
# streams in heap blocks of exactly their size, every refusal, both kinds of file) as a stand-alone program under AddressSanitizer +
# UndefinedBehaviorSanitizer, on the CPU; tests/test_tabix_host.py builds its own copy and runs it: $(TABIX_SAN_EXE)  ->  "ok" and exit 0
TABIX_SAN_EXE ?= $(LIBDIR)/tabix_san
tabix-san: $(TABIX_SAN_EXE)
$(TABIX_SAN_EXE): integration/tabix_san.c $(CSRC)/tabix.c $(CSRC)/tabix_int.h $(CSRC)/bedidx_core.h include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/tabix.c -lpthread -o $@

# TEST ONLY: the host form of the variant-only call set (csrc/variants.c: seeded random records in heap blocks of exactly their size, every
# room, NULL totals, the refusals) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU;
# tests/test_variants_host.py builds its own copy and runs it: $(VARIANTS_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
VARIANTS_SAN_EXE ?= $(LIBDIR)/variants_san
variants-san: $(VARIANTS_SAN_EXE)
$(VARIANTS_SAN_EXE): integration/variants_san.c $(CSRC)/variants.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/variants.c -o $@

# TEST ONLY: the host form of the read-level CpG table (csrc/cpgreads.c: seeded random templates in heap blocks of exactly their size, every
# room, NULL totals, the formatter's rooms, the refusals) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU;
# tests/test_cpg_reads_host.py builds its own copy and runs it: $(CPG_READS_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
CPG_READS_SAN_EXE ?= $(LIBDIR)/cpg_reads_san
cpg-reads-san: $(CPG_READS_SAN_EXE)
$(CPG_READS_SAN_EXE): integration/cpg_reads_san.c $(CSRC)/cpgreads.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/cpgreads.c -o $@

# TEST ONLY: the host form of the allele-specific methylation table (csrc/asm.c: seeded random blocks in heap blocks of exactly their size, every
# room, NULL totals and emit bytes, the formatter's rooms, Fisher's test at its limits, the refusals) as a stand-alone program under
# AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU; tests/test_asm_host.py builds its own copy and runs it: $(ASM_SAN_EXE)  ->  "ok" and
# exit 0, or the case that failed
ASM_SAN_EXE ?= $(LIBDIR)/asm_san
asm-san: $(ASM_SAN_EXE)
$(ASM_SAN_EXE): integration/asm_san.c $(CSRC)/asm.c $(CSRC)/bsmath.h $(CSRC)/bsmath_tables.h include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/asm.c -lm -o $@

# TEST ONLY: the host form of the M-bias table (csrc/mbias.c: seeded random raw blocks in heap blocks of exactly their size, every malformed-list
# form, reads and lists one beyond their buffers, the formatter's rooms, the refusals) as a stand-alone program under AddressSanitizer +
# UndefinedBehaviorSanitizer, on the CPU; tests/test_mbias_host.py builds its own copy and runs it: $(MBIAS_SAN_EXE)  ->  "ok" and exit 0, or the
# case that failed
MBIAS_SAN_EXE ?= $(LIBDIR)/mbias_san
mbias-san: $(MBIAS_SAN_EXE)
$(MBIAS_SAN_EXE): integration/mbias_san.c $(CSRC)/mbias.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/mbias.c -o $@

# TEST ONLY: the host form of the epiallele table (csrc/epi.c: seeded random templates in heap blocks of exactly their size, every room, NULL
# totals, the formatter's rooms, the refusals) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU;
# tests/test_epi_host.py builds its own copy and runs it: $(EPI_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
EPI_SAN_EXE ?= $(LIBDIR)/epi_san
epi-san: $(EPI_SAN_EXE)
$(EPI_SAN_EXE): integration/epi_san.c $(CSRC)/epi.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/epi.c -o $@

# TEST ONLY: the host form of the per-read CpG pattern table (csrc/pat.c: seeded random templates in heap blocks of exactly their size, every room,
# NULL totals, the formatter's rooms, the site count, the refusals) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer,
# on the CPU; tests/test_pat_host.py builds its own copy and runs it: $(PAT_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
PAT_SAN_EXE ?= $(LIBDIR)/pat_san
pat-san: $(PAT_SAN_EXE)
$(PAT_SAN_EXE): integration/pat_san.c $(CSRC)/pat.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/pat.c -o $@

# TEST ONLY: the host form of the per-region fragment summary (csrc/frag.c: seeded random templates and regions in heap blocks of exactly their
# size, NULL totals, the formatter's rooms, the refusals) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, on the
# CPU: $(FRAG_SAN_EXE)  ->  "ok" and exit 0, or the case that failed
FRAG_SAN_EXE ?= $(LIBDIR)/frag_san
frag-san: $(FRAG_SAN_EXE)
$(FRAG_SAN_EXE): integration/frag_san.c $(CSRC)/frag.c include/bscall_amd.h
	$(CC) -std=gnu11 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude $< $(CSRC)/frag.c -o $@

# The library with its HOST C files under AddressSanitizer + UndefinedBehaviorSanitizer (gcc's runtimes; the device objects
# are the ordinary ones): what tests/test_host_sanitizers.py and tools/fuzz_host_inputs.py run the readers and the host
# logic under, on the CPU.  Load it with LD_PRELOAD=<libasan.so>:<libubsan.so> BSCALL_AMD_LIB=$(LIBDIR)/san/libbscall_amd_san.so.
SANFLAGS = -O1 -g -fPIC -Wall -ffp-contract=off -std=gnu11 -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
HOST_C = bscall_api synth_reads vcf_format methbed methcpg methregions bigwig bigbed tabix variants cpgreads asm mbias epi pat frag dbsnp prep report bcf bamio bamstream inflate_fast refseq
san: $(LIBDIR)/libbscall_amd.so
	@mkdir -p $(LIBDIR)/san
	for f in $(HOST_C); do $(CC) $(SANFLAGS) -c $(CSRC)/$$f.c -o $(LIBDIR)/san/$$f.o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(LIBDIR)/san/libbscall_amd_san.so $(LIBDIR)/kernels.o $(LIBDIR)/fused.o $(LIBDIR)/accumulate.o $(LIBDIR)/sort.o $(LIBDIR)/vcfcore.o $(LIBDIR)/sitestats.o $(LIBDIR)/compact.o $(LIBDIR)/probe.o $(LIBDIR)/prepdev.o $(LIBDIR)/bcfdev.o $(LIBDIR)/vcftextdev.o $(LIBDIR)/methdev.o $(LIBDIR)/methregionsdev.o $(LIBDIR)/bigwigdev.o $(LIBDIR)/bwcovdev.o $(LIBDIR)/bigbeddev.o $(LIBDIR)/bgzfdev.o $(LIBDIR)/zlibdev.o $(LIBDIR)/bamdev.o $(LIBDIR)/dbsnpdev.o $(LIBDIR)/csidev.o $(LIBDIR)/beddev.o $(LIBDIR)/variantsdev.o $(LIBDIR)/cpgreadsdev.o $(LIBDIR)/asmdev.o $(LIBDIR)/mbiasdev.o $(LIBDIR)/epidev.o $(LIBDIR)/patdev.o $(LIBDIR)/fragdev.o $(addprefix $(LIBDIR)/san/,$(addsuffix .o,$(HOST_C))) -L$(dir $(shell $(CC) -print-file-name=libasan.so)) -lasan -lubsan -lm -lz -lpthread

# a plain-C host program against the C ABI: gcc only, links the shared library like bs_call would
demo: $(LIBDIR)/demo_block $(LIBDIR)/bam2bcf
$(LIBDIR)/demo_block: integration/demo_block.c integration/mock_work.h integration/amd_overlap_protocol.h integration/amd_bcf_protocol.h include/bscall_amd.h $(LIBDIR)/libbscall_amd.so
	$(CC) -O2 -Wall -std=gnu11 -Iinclude -Iintegration $< -o $@ -L$(LIBDIR) -lbscall_amd -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,$(ROCM)/lib
# BAM + FASTA -> BCF + JSON report with nothing but the C ABI (the C twin of bs_call_amd/pipeline.py)
bam2bcf: $(LIBDIR)/bam2bcf
$(LIBDIR)/bam2bcf: integration/bam2bcf.c include/bscall_amd.h $(LIBDIR)/libbscall_amd.so
	$(CC) -O2 -Wall -std=gnu11 -Iinclude $< -o $@ -L$(LIBDIR) -lbscall_amd -lpthread -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,$(ROCM)/lib

# Compile check of the two replacement translation units against the reference's own headers.  Only in a
# container that has /root/reference; the reference's bs_call.h includes three htslib headers for POINTER TYPES only, so
# the check gives the compiler opaque typedefs for them (generated under /tmp, never committed).  It checks OUR files'
# syntax and types against the reference's declarations; it claims nothing about the oracle or about the reference.
REF ?= /root/reference
glue-check:
	@if [ -d $(REF)/include ]; then \
	  d=$$(mktemp -d /tmp/bsc_glue.XXXXXX); mkdir -p $$d/htslib; \
	  printf 'typedef struct bam_hdr_t bam_hdr_t; typedef struct htsFile htsFile; typedef struct hts_idx_t hts_idx_t; typedef struct hts_itr_t hts_itr_t; typedef struct bam1_t bam1_t;\n#define FT_UNKN 0\n#define FT_GZ 1\n#define FT_VCF 2\n#define FT_VCF_GZ 3\n#define FT_BCF 4\n#define FT_BCF_GZ 5\n' > $$d/htslib/sam.h; \
	  printf 'typedef struct bcf_hdr_t bcf_hdr_t; typedef struct bcf1_t bcf1_t;\n' > $$d/htslib/vcf.h; \
	  printf 'typedef struct faidx_t faidx_t;\n' > $$d/htslib/faidx.h; \
	  for f in integration/call_genotypes_amd.c integration/call_genotypes_amd_overlap.c integration/call_genotypes_amd_bcf.c; do \
	    $(CC) -std=gnu11 -Wall -fsyntax-only -D__LINUX__ -DAMD_GLUE_CHECK -I$$d -I$(REF)/include -I$(REF)/gt/include -Iinclude $$f && echo "glue-check: $$f ok" || exit 1; \
	  done; rm -rf $$d; \
	else echo "glue-check: $(REF) not present, skipped"; fi

asm: $(CSRC)/kernels.hip
	$(HIPCC) $(HIPFLAGS) -S --cuda-device-only -Rpass-analysis=kernel-resource-usage $< -o $(LIBDIR)/kernels.s

clean:
	rm -rf $(LIBDIR)/san; rm -f tests/devmath/libdevmath_probe.so tests/dbsnpdev/dbsnp_flat_host tests/csidev/csi_walk_host $(LIBDIR)/*.o $(LIBDIR)/*.so $(LIBDIR)/*.s $(LIBDIR)/demo_block $(LIBDIR)/bam2bcf $(LIBDIR)/methregions_san $(LIBDIR)/bigwig_san $(LIBDIR)/bigwig_z_san $(LIBDIR)/bigwig_cov_san $(LIBDIR)/bigbed_san $(LIBDIR)/tabix_san $(LIBDIR)/variants_san $(LIBDIR)/cpg_reads_san $(LIBDIR)/asm_san $(LIBDIR)/mbias_san $(LIBDIR)/epi_san $(LIBDIR)/pat_san $(LIBDIR)/frag_san
	$(MAKE) -C oracle clean

.PHONY: all oracle demo asm clean glue-check san devmath-probe dbsnp-flat-host csi-walk-host tabix-san bigwig-cov-san variants-san cpg-reads-san asm-san mbias-san epi-san pat-san frag-san
