"""Inputs of the per-read CpG pattern table's tests (tests/test_pat_host.py, tests/test_gpu_pat.py): a hand-worked block whose records, totals
and table bytes are written out here, blocks that cut templates at 64 sites, the placement blocks of the read-level and the epiallele table,
long reads, contention and seeded random blocks.  A block is a dict {name, tpl, seq, x, y, ref, min_qual, params} as tests/cpg_reads_cases.py
makes them; params are the pattern table's ({"min_sites": n})."""
import numpy as np

import cpg_reads_cases as K
import epi_cases as E

PAR = {"min_sites": 1}


def block(name, rows, x, y, ref, min_qual=20, min_sites=1):
    return K.block(name, rows, x, y, ref, min_qual=min_qual, params={"min_sites": min_sites})


def with_params(b, min_sites=1):
    """A block of another table's cases with this table's params."""
    return dict(b, params={"min_sites": min_sites})


# ---- the hand-worked block: 14 templates over the 7 sites 303, 310, 318, 325, 333, 342, 350 (ordinals 0 .. 6) of positions 301 .. 370 ------------
HAND_SITES = (303, 310, 318, 325, 333, 342, 350)


def hand_block():
    """min_qual 20.                                   ordinal 0 1 2 3 4 5 6
      T1  C2T 301 .. 370:                                     C T C C T T C   k 7   idx 0  CTCCTTC
      T2  G2A 304 .. 313 (the G's of 303, 310):               C T             k 2   idx 0  CT
      T3  C2T 301 .. 320:                                     C T C           k 3   idx 0  CTC: CT is its prefix and sorts first
      T4  C2T 301 .. 312 + 331 .. 352:                        C C . . T C T   k 5   idx 0  CC..TCT: 318 and 325 lie in the gap
      T5  C2T 301 .. 320, quality 19 at 310:                  C . T           k 2   idx 0  C.T: '.', 'C' (T4) and 'T' (T1) in column 1 of idx 0
      T6  C2T 316 .. 335, quality 5 at 333:                       C T q       k 2   idx 2  CT: the low quality at the end is trimmed; CT again
      T7, T8, T9  G2A 326 .. 345 (the G's of 325, 333, 342):        T T C     k 3   idx 3  TTC, three times
      T10 C2T 345 .. 354:                                                 C   k 1   idx 6  C
      T11 C2T 319 .. 324: no site                                             k 0   nothing
      T12 bs_strand 0 over all: ignored
    min_sites 1: 8 records, 10 pieces from 10 templates; C 1 + 3 + 1 + 2 + 4 + 1 + 3 x 1 + 1 = 16, T 1 + 2 + 1 + 1 + 3 + 1 + 3 x 2 + 0 = 15,
    '.' 1 + 2 = 3; nothing cut; S 7.
    min_sites 3: T1, T3, T4 and T7 .. T9 alone: 4 records, 6 pieces, C 4 + 2 + 3 + 3 = 12, T 3 + 1 + 2 + 6 = 12, '.' 2."""
    c2t, g2a = K._c2t, K._g2a
    three = (2, g2a(326, 20, {325: "U", 333: "U", 342: "M"}), None)
    rows = [
        (1, c2t(301, 70, {303: "M", 310: "U", 318: "M", 325: "M", 333: "U", 342: "U", 350: "M"}), None),
        (2, g2a(304, 10, {303: "M", 310: "U"}), None),
        (1, c2t(301, 20, {303: "M", 310: "U", 318: "M"}), None),
        (1, c2t(301, 12, {303: "M", 310: "M"}), c2t(331, 22, {333: "U", 342: "M", 350: "U"})),
        (1, c2t(301, 20, {303: "M", 310: ("C", 19), 318: "U"}), None),
        (1, c2t(316, 20, {318: "M", 325: "U", 333: ("C", 5)}), None),
        three, three, three,
        (1, c2t(345, 10, {350: "M"}), None),
        (1, c2t(319, 6, {}), None),
        (0, c2t(301, 70, {p: "M" for p in HAND_SITES}), None),
    ]
    return block("hand", rows, 301, 370, K.ref_with_sites(301, 70, HAND_SITES))


HAND_INDEX_BASE = 100
HAND_RECORDS = [(0, "C.T", 1), (0, "CC..TCT", 1), (0, "CT", 1), (0, "CTC", 1), (0, "CTCCTTC", 1), (2, "CT", 1), (3, "TTC", 3), (6, "C", 1)]
HAND_TOTALS = (8, 10, 10, 16, 15, 3, 0, 7)
HAND_TABLE = (b"chrP\t101\tC.T\t1\n" b"chrP\t101\tCC..TCT\t1\n" b"chrP\t101\tCT\t1\n" b"chrP\t101\tCTC\t1\n" b"chrP\t101\tCTCCTTC\t1\n"
              b"chrP\t103\tCT\t1\n" b"chrP\t104\tTTC\t3\n" b"chrP\t107\tC\t1\n")
HAND_RECORDS_3 = [(0, "CC..TCT", 1), (0, "CTC", 1), (0, "CTCCTTC", 1), (3, "TTC", 3)]
HAND_TOTALS_3 = (4, 6, 6, 12, 12, 2, 0, 7)
HAND_TABLE_3 = b"chrP\t101\tCC..TCT\t1\n" b"chrP\t101\tCTC\t1\n" b"chrP\t101\tCTCCTTC\t1\n" b"chrP\t104\tTTC\t3\n"


# ---- cutting: a site every 2 positions, templates given as their string from a first ordinal -------------------------------------------------------
def _string_row(x, first, s, strand=1):
    """A single-read template whose string is s from ordinal `first` on, over sites x + 2 i ('.': another base)."""
    st = {x + 2 * (first + j): {"C": "M", "T": "U"}.get(c, "A" if strand == 1 else "C") for j, c in enumerate(s)}
    p0, n = x + 2 * first, 2 * len(s)
    if strand == 2:
        return (2, K._g2a(p0 + 1, n, st), None)
    return (1, K._c2t(p0, n, st), None)


def _string_block(name, n_sites, rows, x=1000):
    n = 2 * n_sites + 4
    return block(name, [_string_row(x, *r) for r in rows], x, x + n - 1, K.ref_with_sites(x, n, [x + 2 * i for i in range(n_sites)]))


def _mix(n, seed):
    rng = np.random.default_rng(seed)
    return "".join("CT"[int(v)] for v in rng.integers(0, 2, n))


def cut_blocks():
    """(block, its records where they are worked by hand or None)."""
    out = []
    # spans of 64, 65, 128 and 129 sites, every site with a state, on both strands and from ordinals that are no multiple of 64
    rows, exp = [], []
    for k, (n, first, strand) in enumerate(((64, 0, 1), (65, 3, 2), (128, 5, 1), (129, 1, 2), (64, 70, 2), (65, 64, 1))):
        s = _mix(n, 100 + k)
        rows.append((first, s, strand))
        exp += [(first + a, s[a:a + 64], 1) for a in range(0, n, 64)]
    out.append((_string_block("spans of 64, 65, 128, 129", 140, rows), sorted(exp)))
    # a cut that leaves a piece of dots only; a piece trimmed at both ends
    a = "C" + "." * 127 + "T"
    b = "CCC" + "." * 61 + ".." + "CTC" + "." * 59 + "T"
    out.append((_string_block("a piece of dots, a piece trimmed at both ends", 140, [(2, a, 1), (4, b, 2)]),
                [(2, "C", 1), (4, "CCC", 1), (70, "CTC", 1), (130, "T", 1), (132, "T", 1)]))
    # equal in the first 64 sites and different at site 65; different only at site 64, at site 1, at sites 32 and 33 (the hi / lo seam)
    p64, p63, p31, p32 = _mix(64, 7), _mix(63, 8), _mix(31, 9), _mix(32, 10)
    rows = [(0, p64 + "C", 1), (0, p64 + "T", 2),  # piece 0 twice, then C and T at ordinal 64
            (1, p63 + "C", 1), (1, p63 + "T", 1),
            (2, "C" + p63, 2), (2, "T" + p63, 1),
            (3, p31 + "C" + p32, 1), (3, p31 + "T" + p32, 2),
            (4, p32 + "C" + p31, 1), (4, p32 + "T" + p31, 1)]
    exp = [(0, p64, 2), (64, "C", 1), (64, "T", 1)] + [(f, s, 1) for f, s, _ in rows[2:]]
    out.append((_string_block("seams", 80, rows), sorted(exp)))
    return out


# ---- placement: the blocks of the read-level and the epiallele table (lanes 0, 62, 63; one to four tiles with an empty one between; a site at y;
# mates and a read outside the buffer) ------------------------------------------------------------------------------------------------------------
def placement_blocks():
    return [with_params(b) for b in K.targeted_blocks() + E.targeted_blocks()] + [with_params(E.hand_block(), 3), with_params(K.hand_block(), 2)]


def long_read_blocks():
    """The 5 000-base reads: over 80 sites (one piece and two) and over 2 500 (40 pieces a read)."""
    return [with_params(K.long_read_block()), with_params(E.long_read_block()), with_params(E.long_read_block(), 2490)]


def identical_block(n=5000):
    """n identical templates: one record with count n."""
    return with_params(E.contention_block(n))


def sixteen_block(n=5000):
    """n templates in 16 patterns on one index."""
    return with_params(E.contention_block(n, spread=True))


def distinct_block(n=5000):
    """n templates, all distinct: template i spells i + 1 in 13 bits over sites 1 .. 13 (C = 1), behind a site 0 it lacks where bit 0 is 0."""
    x, sites = 50, [52 + 4 * i for i in range(14)]
    base, seq0 = K.templates([(1, K._c2t(x, 60, {}), None)])
    tpl = np.repeat(base, n)
    seq = np.tile(seq0, max(n, 1)).reshape(max(n, 1), 60)[:n].copy()
    for i in range(n):
        v = i + 1
        for j in range(13):
            seq[i, sites[j + 1] - x] = K.BASE["C" if (v >> j) & 1 else "T"] | 30 << 2
        if v & 1:
            seq[i, sites[0] - x] = K.BASE["T"] | 30 << 2
        tpl[i]["off"][0] = 60 * i
    return dict(name="%d distinct" % n, tpl=tpl, seq=seq.reshape(-1), x=x, y=x + 59, ref=K.ref_with_sites(x, 60, sites), min_qual=20, params=dict(PAR))


PIECE_COUNTS = (0, 1, 63, 64, 65, 4113)  # around a wave, a workgroup of the heads pass and a block of the sort


def dense_block(seed, n_pos, nr, min_sites=1):
    return with_params(E.dense_block(seed, n_pos, nr), min_sites)


TILE_EDGE_BLOCKS = E.TILE_EDGE_BLOCKS


def big_block():
    return with_params(E.big_block())


def host_blocks():
    """Every block the host test and the GPU test compare on, the big ones apart."""
    return ([hand_block(), dict(hand_block(), params={"min_sites": 3})] + [b for b, _ in cut_blocks()] + placement_blocks() + long_read_blocks()
            + [dense_block(seed, n_pos, 40) for n_pos, seed in TILE_EDGE_BLOCKS])
