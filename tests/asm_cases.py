"""Inputs of the allele-specific methylation table's tests (tests/test_asm_host.py, tests/test_gpu_asm.py): the blocks of
tests/cpg_reads_cases.py (TEMPLATE arrays, their read bytes, reference codes) with dense VCF_CORE records and emit bytes beside them — the
hand-worked block, the 48 ALLELE blocks, the targeted blocks and seeded random ones.  The dense records are record BYTES with chosen gt, phred,
flt and emit, not called ones.  A block is a dict {name, tpl, seq, x, y, ref, core, emit, min_qual, params}."""
import numpy as np

import cpg_reads_cases as K
from bs_call_amd.abi import VCF_CORE

HET = (1, 2, 3, 5, 6, 8)
DEFAULT = {"min_phred": 20, "pass_only": 0, "max_dist": 500, "min_cov": 2}


def cores(x, n, snps):
    """VCF_CORE[n] for x .. x + n - 1, all-zero but for snps = {pos: gt or (gt, phred, flt, emit)}."""
    c = np.zeros(n, VCF_CORE)
    for pos, v in snps.items():
        gt, phred, flt, emit = v if isinstance(v, tuple) else (v, 40, 0, 1)
        r = c[pos - x]
        r["pos"], r["gt"], r["phred"], r["flt"], r["emit"] = pos, gt, phred, flt, emit
    return c


def block(name, rows, x, y, ref, snps, emit=None, min_qual=20, params=None):
    b = K.block(name, rows, x, y, ref, min_qual=min_qual)
    n = y - x + 1
    b["core"] = cores(x, n, snps)
    b["emit"] = emit
    b["params"] = dict(DEFAULT, **(params or {}))
    return b


# ---- the hand-worked block: 7 templates, the sites 205, 212, 220, 230 and the SNPs 210 (AT), 221 (CG, the G of 220) and 230 (CT, the C of 230)
#      of positions 201 .. 240, W = 8 ------------------------------------------------------------------------------------------------------------
def hand_block():
    rows = [
        (1, K.read(203, 20, "G", at={210: "A", 205: "C", 212: "T"}), None),  # allele 1 of 210: 205 M, 212 U; its G at 221 is allele 2 of CG
        (1, K.read(203, 20, "G", at={210: "T", 205: "T", 212: "T"}), None),  # a T on C2T is C or T: allele 2 of AT; U U; allele 2 at 221
        (2, K.read(203, 20, "T", at={210: "A", 206: "G", 213: "A"}), None),  # an A on G2A is G or A: allele 1 of AT; M U; T at 221: neither
        (1, K.read(208, 8, "G", at={210: ("A", 10), 212: "C"}), None),  # the SNP's byte below min_qual: no allele, nothing counted
        (1, K.read(203, 5, "G", at={205: "C"}), K.read(209, 6, "G", at={210: "T", 212: "C"})),  # read 1 gives the SNP byte, read 0 a CpG: allele 2, M M
        (1, K.read(225, 12, "G", at={230: "C"}), None),  # CT on a C2T template: no allele
        (2, K.read(225, 12, "T", at={230: "C"}), None),  # CT on a G2A template: allele 1; the only site of the window is the SNP's own
    ]
    return block("hand", rows, 201, 240, K.ref_with_sites(201, 40, [205, 212, 220, 230]), {210: 3, 221: 5, 230: 6}, params={"max_dist": 8, "min_cov": 1})


# snp_pos, cpg_pos, m1, u1, m2, u2, aq, info — tallied by hand from the rule (the host test's docstring has the tally).  Fisher's p of {2, 0, 1, 1}
# and of {0, 2, 1, 1} is 1: the two tables of those margins have probability 1/2 each
HAND_RECORDS = [
    (210, 205, 2, 0, 1, 1, 0, 3),
    (210, 212, 0, 2, 1, 1, 0, 3),
    (221, 220, 0, 0, 0, 0, 0, 5 | 1 << 8),
    (230, 230, 0, 0, 0, 0, 0, 6 | 1 << 8),
]
HAND_TOTALS = (3, 4, 7, 3, 8, 0, 0, 0)
HAND_TABLE = (b"chrT\t204\t206\t210\tAT\t2\t0\t1\t1\t0\t-5\n"
              b"chrT\t211\t213\t210\tAT\t0\t2\t1\t1\t0\t2\n")

# ---- ALLELE: 2 strands x 6 genotypes x 4 read bases, written by hand from the rule ----------------------------------------------------------
# (bs_strand, gt): the allele for a read A, C, G, T
ALLELE_TABLE = {
    (1, 1): (1, 2, 0, 2),  # AC, C2T: a T may be a C
    (1, 2): (1, 0, 2, 0),  # AG
    (1, 3): (1, 0, 0, 2),  # AT
    (1, 5): (0, 1, 2, 1),  # CG: a T may be a C
    (1, 6): (0, 0, 0, 0),  # CT: cannot be told from conversion
    (1, 8): (0, 0, 1, 2),  # GT
    (2, 1): (1, 2, 0, 0),  # AC, G2A
    (2, 2): (0, 0, 0, 0),  # AG: cannot be told from conversion
    (2, 3): (1, 0, 0, 2),  # AT
    (2, 5): (2, 1, 2, 0),  # CG: an A may be a G
    (2, 6): (0, 1, 0, 2),  # CT
    (2, 8): (1, 0, 1, 2),  # GT: an A may be a G
}


def allele_blocks():
    """One block per entry: a SNP at 1010, a site at 1015, one template that reads the site methylated.  -> [(block, expected allele)]"""
    out = []
    x = 1000
    for (bs, gt), want in ALLELE_TABLE.items():
        for base, al in zip("ACGT", want):
            at = {1010: base}
            at[1015 if bs == 1 else 1016] = "C" if bs == 1 else "G"
            rows = [(bs, K.read(1005, 20, "G" if bs == 1 else "T", at=at), None)]
            out.append((block("allele bs %d gt %d read %s" % (bs, gt, base), rows, x, x + 29, K.ref_with_sites(x, 30, [1015]), {1010: gt}, params={"min_cov": 1}), al))
    return out


# ---- the targeted blocks ---------------------------------------------------------------------------------------------------------------------
def _c2t(pos, length, at):
    return K.read(pos, length, "G", at={p: {"M": "C", "U": "T"}.get(s, s) for p, s in at.items()})


def _g2a(pos, length, at):
    """States are given by SITE position (the byte lies one further); a base at a SNP is given as ("snp", base)."""
    d = {}
    for p, s in at.items():
        if isinstance(s, tuple):
            d[p] = s[1]
        else:
            d[p + 1] = {"M": "G", "U": "A"}.get(s, s)
    return K.read(pos, length, "T", at=d)


def targeted_blocks():
    out = []
    # SNPs at x and at y, h - W < 0 (x == 1), W = 1 and W = 65535 on a 200-position block
    sites = [3, 40, 41 + 60, 150, 198]
    rows = [
        (1, _c2t(1, 200, {1: "A", 200: "T", 3: "M", 40: "U", 101: "M", 150: "M", 198: "U"}), None),
        (1, _c2t(1, 200, {1: "T", 200: "A", 3: "U", 40: "U", 101: "M", 150: "U", 198: "M"}), None),
        (2, _g2a(1, 200, {1: ("snp", "A"), 200: ("snp", "T"), 3: "M", 40: "M", 101: "U", 150: "M", 198: "M"}), None),
        (2, _g2a(150, 51, {200: ("snp", "A"), 150: "U", 198: "U"}), None),
    ]
    for W in (1, 2, 65535):
        out.append(block("snps at x and y, W %d" % W, rows, 1, 200, K.ref_with_sites(1, 200, sites), {1: 3, 200: 3, 2: 3}, params={"max_dist": W, "min_cov": 1}))
    # a site with s == h and one with s + 1 == h, and their neighbours, which are counted
    x = 1000
    sites = [x + 10, x + 20, x + 30]
    rows = [
        (1, _c2t(x, 50, {x + 20: "T", x + 31: "A", x + 10: "M", x + 30: "M"}), None),  # h == s at 1020 (CT: no allele on C2T); AG at 1031 = s + 1
        (2, _g2a(x, 50, {x + 20: ("snp", "C"), x + 31: ("snp", "G"), x + 10: "M", x + 30: "U"}), None),  # CT on G2A: allele 1; AG on G2A: none
        (1, _c2t(x, 50, {x + 20: "C", x + 31: "G", x + 10: "U", x + 30: "U"}), None),  # AG on C2T: G -> allele 2
    ]
    out.append(block("overlapped sites", rows, x, x + 59, K.ref_with_sites(x, 60, sites), {x + 20: 6, x + 31: 2}, params={"max_dist": 25, "min_cov": 1}))
    # mates where read 1 gives the SNP byte and read 0 the CpG, and the other way round; a byte below min_qual at the SNP
    sites = [x + 10, x + 80]
    rows = [
        (1, _c2t(x + 5, 20, {x + 10: "M"}), _c2t(x + 50, 40, {x + 60: "A", x + 80: "U"})),
        (1, _c2t(x + 50, 40, {x + 60: "T", x + 80: "M"}), _c2t(x + 5, 20, {x + 10: "U"})),
        (2, _g2a(x + 5, 20, {x + 10: "M"}), _g2a(x + 50, 40, {x + 60: ("snp", "A"), x + 80: "M"})),
        (1, K.read(x + 5, 90, "G", at={x + 10: "C", x + 60: ("A", 19), x + 80: "C"}), None),  # below min_qual at the SNP: nothing
        (1, K.read(x + 5, 90, "G", at={x + 10: "C", x + 60: ("A", 19), x + 80: "C"}), K.read(x + 55, 10, "G", at={x + 60: "T"})),  # read 1 where 0 fails
    ]
    out.append(block("mates and quality", rows, x, x + 99, K.ref_with_sites(x, 100, sites), {x + 60: 3}, params={"max_dist": 100, "min_cov": 1}))
    # each threshold alone, and emit bytes with a 0 over an emitted het record
    sites = [x + 10]
    rows = [(1, _c2t(x, 40, {x + 5: "A", x + 15: "A", x + 20: "A", x + 25: "A", x + 30: "A", x + 10: "M"}), None)]
    snps = {x + 5: (3, 19, 0, 1), x + 15: (3, 20, 4, 1), x + 20: (3, 40, 0, 0), x + 25: (4, 40, 0, 1), x + 30: (3, 40, 0, 1)}
    for name, par in (("defaults", {}), ("min_phred 19", {"min_phred": 19}), ("min_phred 0", {"min_phred": 0}), ("pass_only", {"pass_only": 1}),
                      ("min_phred 41", {"min_phred": 41})):
        out.append(block("thresholds: " + name, rows, x, x + 39, K.ref_with_sites(x, 40, sites), snps, params=dict(par, min_cov=1)))
    emit = np.ones(40, np.uint8)
    emit[30] = 0
    out.append(block("emit bytes", rows, x, x + 39, K.ref_with_sites(x, 40, sites), snps, emit=emit, params={"min_cov": 1}))
    # no SNP, no site, no template
    out.append(block("no snp", rows, x, x + 39, K.ref_with_sites(x, 40, sites), {}))
    out.append(block("no site", rows, x, x + 39, K.ref_with_sites(x, 40, []), snps))
    out.append(block("no template", [], x, x + 39, K.ref_with_sites(x, 40, sites), snps))
    return out


def tile_blocks():
    """Tile-position cases of the kernels (tile k = positions x + 64 k ..)."""
    out = []
    x = 1000
    # a SNP in lane 0 and one in lane 63 of a tile, their windows across the tile's borders
    sites = [x + 60, x + 66, x + 120, x + 125, x + 130]
    rows = [
        (1, _c2t(x + 50, 100, {x + 64: "A", x + 127: "T", x + 60: "M", x + 66: "U", x + 120: "M", x + 125: "U", x + 130: "M"}), None),
        (2, _g2a(x + 50, 100, {x + 64: ("snp", "T"), x + 127: ("snp", "A"), x + 60: "U", x + 66: "M", x + 120: "U", x + 125: "M", x + 130: "U"}), None),
        (1, _c2t(x + 64, 64, {x + 64: "T", x + 127: "A", x + 66: "M", x + 120: "U", x + 125: "M"}), None),  # the tile exactly
    ]
    out.append(block("snps in lanes 0 and 63", rows, x, x + 199, K.ref_with_sites(x, 200, sites), {x + 64: 3, x + 127: 3}, params={"max_dist": 6, "min_cov": 1}))
    # a C at lane 63 read by a G2A template (its byte is lane 0 of the next tile)
    sites = [x + 63, x + 127]
    rows = [
        (2, _g2a(x + 40, 100, {x + 70: ("snp", "A"), x + 63: "M", x + 127: "U"}), None),
        (2, _g2a(x + 64, 65, {x + 70: ("snp", "T"), x + 63: "U", x + 127: "M"}), None),  # begins on the G of the site at lane 63
        (1, _c2t(x + 40, 100, {x + 70: "T", x + 63: "M", x + 127: "M"}), None),
    ]
    out.append(block("a C at lane 63 on G2A", rows, x, x + 199, K.ref_with_sites(x, 200, sites), {x + 70: 3}, params={"max_dist": 80, "min_cov": 1}))
    # a window that covers 3 tiles with an empty one in the middle
    sites = [x + 10, x + 20, x + 140, x + 150]
    rows = [
        (1, _c2t(x, 192, {x + 80: "A", x + 10: "M", x + 20: "U", x + 140: "M", x + 150: "M"}), None),
        (1, _c2t(x, 192, {x + 80: "T", x + 10: "U", x + 20: "U", x + 140: "U", x + 150: "M"}), None),
        (2, _g2a(x + 70, 100, {x + 80: ("snp", "A"), x + 140: "M", x + 150: "U"}), None),
    ]
    out.append(block("three tiles, the middle one empty", rows, x, x + 191, K.ref_with_sites(x, 192, sites), {x + 80: 3}, params={"max_dist": 75, "min_cov": 1}))
    # two SNPs 3 bases apart that share window sites
    sites = [x + 30, x + 45, x + 70]
    rows = [
        (1, _c2t(x + 20, 60, {x + 50: "A", x + 53: "G", x + 30: "M", x + 45: "U", x + 70: "M"}), None),
        (1, _c2t(x + 20, 60, {x + 50: "T", x + 53: "T", x + 30: "U", x + 45: "U", x + 70: "M"}), None),
        (2, _g2a(x + 20, 60, {x + 50: ("snp", "A"), x + 53: ("snp", "A"), x + 30: "M", x + 45: "M", x + 70: "U"}), None),
    ]
    out.append(block("two snps 3 bases apart", rows, x, x + 99, K.ref_with_sites(x, 100, sites), {x + 50: 3, x + 53: 8}, params={"max_dist": 20, "min_cov": 1}))
    return out


def long_read_block():
    """A single read of 5 000 bases (a span of 79 tiles) with two SNPs in it, on both strands."""
    b = K.long_read_block()
    x = b["x"]
    free = [p for p in range(x + 1000, x + 4000) if b["ref"][p - x] == 1 and b["ref"][p - 1 - x] == 1]  # an A behind an A: no site's C or G
    h1, h2 = free[0], free[-1]
    for t, base in ((0, (0, 3)), (1, (3, 0))):  # the C2T read: A at h1, T at h2; the G2A read: T, A
        for h, v in zip((h1, h2), base):
            b["seq"][int(b["tpl"]["off"][t][0]) + h - int(b["tpl"]["pos"][t][0])] = v | 30 << 2
    b["core"] = cores(x, 5000, {h1: 3, h2: 3})
    b["emit"] = None
    b["params"] = dict(DEFAULT, max_dist=700, min_cov=1)
    b["name"] = "long read"
    return b


def repeated_block(n):
    """n three-base C2T templates on one pair: the SNP at x + 10 (allele 1), the site at x + 11 (M)."""
    x = 50
    rows = [(1, K.read(x + 10, 3, "G", at={x + 10: "A", x + 11: "C"}), None)]
    b = block("%d templates on one pair" % n, rows, x, x + 19, K.ref_with_sites(x, 20, [x + 11]), {x + 10: 3}, params={"min_cov": 1})
    b["tpl"] = np.repeat(b["tpl"], n)
    return b


def contention_block(n=5000):
    """n templates on one pair of records, in all four counters."""
    x = 50
    rows = [
        (1, K.read(x, 20, "G", at={x + 10: "A", x + 3: "C", x + 15: "T"}), None),
        (1, K.read(x, 20, "G", at={x + 10: "T", x + 3: "T", x + 15: "C"}), None),
    ]
    b = block("contention", rows, x, x + 19, K.ref_with_sites(x, 20, [x + 3, x + 15]), {x + 10: 3}, params={"min_cov": 1})
    b["tpl"] = np.repeat(b["tpl"], n // 2)
    return b


def random_block(seed, n_pos, nr, n_snps, x=None, params=None, with_emit=True):
    """cpg_reads_cases.random_block with n_snps random heterozygous records (and as many records that fail one condition) beside it."""
    b = K.random_block(seed, n_pos, nr, x=x)
    rng = np.random.default_rng(seed + 77)
    core = np.zeros(n_pos, VCF_CORE)
    pos = rng.choice(n_pos, min(n_pos, 2 * n_snps), replace=False)
    for k, i in enumerate(pos):
        r = core[i]
        r["pos"], r["gt"], r["phred"], r["flt"], r["emit"] = b["x"] + i, rng.choice(HET), rng.integers(20, 60), 0, 1
        if k >= n_snps:  # not a SNP, for one reason each
            why = k % 4
            if why == 0:
                r["gt"] = rng.choice([0, 4, 7, 9])
            elif why == 1:
                r["phred"] = rng.integers(0, 20)
            elif why == 2:
                r["emit"] = 0
            else:
                r["flt"] = rng.choice([1, 2, 4, 8, 128])  # (a SNP unless pass_only)
    emit = None
    if with_emit:
        emit = (core["emit"] != 0).astype(np.uint8)
        emit[rng.random(n_pos) < 0.02] ^= 1  # a 0 over an emitted record, a 1 over a record not emitted
    b["core"], b["emit"] = core, emit
    b["params"] = dict(DEFAULT, **(params or {"max_dist": 150, "min_cov": 1}))
    b["name"] = "random %d" % seed
    return b
