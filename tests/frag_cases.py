"""Inputs of the per-region fragment summary's tests (tests/test_frag_host.py, tests/test_gpu_frag.py): blocks as tests/cpg_reads_cases.py and
tests/epi_cases.py make them — {name, tpl, seq, x, y, ref, min_qual, params} — with a list of regions beside them: b["regions"], (start, end)
pairs, 0-based and half-open, sorted by (start, end) as bsc_frag_attach wants them.  params are the summary's ({"min_sites": n, ...})."""
import numpy as np

import cpg_reads_cases as K
import epi_cases as E

PAR = {"min_sites": 3, "u_max_pct": 25, "m_min_pct": 75}


def with_regions(b, regions, params=None, name=None):
    out = dict(b, regions=sorted((int(a), int(e)) for a, e in regions), params=dict(PAR if params is None else params))
    if name:
        out["name"] = name
    return out


# ---- the hand-worked block: 6 templates over the 10 sites of positions 301 .. 380, five regions ----------------------------------------------
HAND_SITES = (305, 310, 316, 322, 330, 338, 345, 352, 360, 366)
HAND_REGIONS = [(300, 380), (309, 330), (330, 352), (340, 340), (352, 380)]


def hand_block():
    """min_sites 3, U iff 100 m <= 25 k, M iff 100 m >= 75 k; min_qual 20.  A site at p is in {start, end} iff start < p <= end:
      A (300, 380] all ten sites.   B (309, 330] = 310 316 322 330: 330 is its END, the C inside and the G (331) outside.
      C (330, 352] = 338 345 352: 330 is its START, the C outside (its G, 331, inside: not C's), 352 its end.   D (340, 340] empty.
      E (352, 380] = 360 366.
      T1 C2T 301 .. 380          305 M 310 M 316 U 322 M 330 M 338 U 345 U 352 U 360 M 366 U
                                 A k 10 m 5: X, discordant.  B k 4 m 3 (M U M M): 300 >= 300: M, discordant.  C k 3 m 0: U.  E k 2: short.
      T2 G2A 306 .. 353          (the G's of 305 .. 352) 305 U 310 U 316 U 322 M 330 M 338 M 345 M 352 M
                                 A k 8 m 5: X, discordant.  B k 4 m 2 (330's byte is read at 331, outside B; the site is B's): X, discordant.
                                 C k 3 m 3 (not 330, whose G is inside C; 352, whose G at 353 is outside C, counts): M.  E nothing.
      T3 C2T 301 .. 318 + 336 .. 365   305 U 310 U 316 U . . 338 U 345 M 352 U 360 U   (322 and 330 lie in the gap)
                                 A k 7 m 1: 100 <= 175: U, discordant.  B k 2: short.  C k 3 m 1: 100 > 75, 100 < 225: X, discordant.  E k 1: short.
      T4 C2T 308 .. 350          310 M 316 M 322 q19 330 M 338 M 345 M
                                 A k 5 m 5: M.  B k 3 = min_sites, m 3: M.  C k 2 = min_sites - 1: short.
      T5 bs_strand 0             ignored
      T6 G2A 361 .. 375          (the G's of 360 and 366) M M:  A k 2: short.  E k 2: short.
    A: frags 4 = U 1 (T3) + X 2 (T1 T2) + M 1 (T4), K 10 + 8 + 7 + 5 = 30, Mm 5 + 5 + 1 + 5 = 16, disc 3, short 1 (T6).
    B: frags 3 = X 1 (T2) + M 2 (T1 T4), K 4 + 4 + 3 = 11, Mm 3 + 2 + 3 = 8, disc 2, short 1 (T3).
    C: frags 3 = U 1 (T1) + X 1 (T3) + M 1 (T2), K 9, Mm 0 + 3 + 1 = 4, disc 1, short 1 (T4).     D: nothing.     E: short 3 (T1 T3 T6).
    totals: 5 templates with a state; frags 10, U 2, X 4, M 4, K 50, Mm 28, disc 6."""
    c2t, g2a = K._c2t, K._g2a
    rows = [
        (1, c2t(301, 80, dict(zip(HAND_SITES, "MMUMMUUUMU"))), None),
        (2, g2a(306, 48, dict(zip(HAND_SITES[:8], "UUUMMMMM"))), None),
        (1, c2t(301, 18, {305: "U", 310: "U", 316: "U"}), c2t(336, 30, {338: "U", 345: "M", 352: "U", 360: "U"})),
        (1, c2t(308, 43, {310: "M", 316: "M", 322: ("C", 19), 330: "M", 338: "M", 345: "M"}), None),
        (0, c2t(301, 80, {p: "M" for p in HAND_SITES}), None),
        (2, g2a(361, 15, {360: "M", 366: "M"}), None),
    ]
    return with_regions(K.block("hand", rows, 301, 380, K.ref_with_sites(301, 80, HAND_SITES)), HAND_REGIONS)


# frags U X M K Mm disc short, in the order of HAND_REGIONS
HAND_ACC = [(4, 1, 2, 1, 30, 16, 3, 1), (3, 0, 1, 2, 11, 8, 2, 1), (3, 1, 1, 1, 9, 4, 1, 1), (0,) * 8, (0, 0, 0, 0, 0, 0, 0, 3)]
HAND_TOTALS = (5, 10, 2, 4, 4, 50, 28, 6)
HAND_NAMES = ["all", None, "island", "empty", "tail"]
HAND_TABLE = (b"chrF\t300\t380\tall\t4\t1\t2\t1\t30\t16\t3\t1\n" b"chrF\t309\t330\t.\t3\t0\t1\t2\t11\t8\t2\t1\n"
              b"chrF\t330\t352\tisland\t3\t1\t1\t1\t9\t4\t1\t1\n" b"chrF\t340\t340\tempty\t0\t0\t0\t0\t0\t0\t0\t0\n"
              b"chrF\t352\t380\ttail\t0\t0\t0\t0\t0\t0\t0\t3\n")

BORDER_KM = [(4, 1), (4, 3), (3, 1), (8, 2), (8, 6), (8, 3), (1, 0), (1, 1)]


def borders_block(params=None):
    """One region over eight sites, a C2T template per (k, m) of BORDER_KM: it covers the first k sites and reads the first m of them M."""
    x = 500
    s = [x + 3 + 7 * i for i in range(8)]
    rows = [(1, K._c2t(x, s[k - 1] - x + 1, {p: "M" if i < m else "U" for i, p in enumerate(s[:k])}), None) for k, m in BORDER_KM]
    return with_regions(K.block("class borders", rows, x, x + 59, K.ref_with_sites(x, 60, s)), [(x - 1, x + 59)], params)


# ---- regions around a block's sites, tiles and ends -------------------------------------------------------------------------------------------
def edge_regions(b):
    """start in {p - 2, p - 1, p} and end in {p - 1, p, p + 1} around up to six sites (the first, the last, those at lanes 0 and 63), every
    pair of tile borders, regions inside a tile, empty ones, regions in front of x, behind y and across y, duplicates and nested ones."""
    from bs_call_amd import frag

    x, y = b["x"], b["y"]
    sp = frag.site_positions(x, y, b["ref"])
    pick = [p for p in sp if (p - x) % 64 in (0, 63)][:4] + sp[:1] + sp[-1:]
    out = []
    for p in pick:
        for a in (p - 2, p - 1, p):
            for e in (p - 1, p, p + 1):
                if 0 <= a <= e:
                    out.append((a, e))
    borders = [x - 1 + 64 * k for k in range((y - x) // 64 + 2)]
    out += [(a, e) for i, a in enumerate(borders) for e in borders[i:]]  # one to four tiles and more, start == end among them
    out += [(x + 3, x + 40), (x + 70, x + 70), (max(x - 50, 0), max(x - 10, 0)), (0, max(x - 1, 0)), (y, y + 30), (y + 5, y + 9), (y - 1, y + 1), (y - 1, y)]
    out += [(max(x - 1, 0), y), (max(x - 1, 0), y), (x + 10, y - 10), (x + 20, y - 20), (x + 20, y - 20)]  # duplicates, nested
    out += [(x + 5 + 9 * i, x + 30 + 9 * i) for i in range(8)]  # staggered
    return [(a, e) for a, e in out if a <= e]  # (a block shorter than the offsets above)


def edge_blocks():
    x = 1000
    s = [x, x + 63, x + 64, x + 127, x + 192, x + 255, x + 299]  # lanes 0 and 63; tile 2 is empty; the last site is y
    tiles = K.block("sites at lanes 0 and 63, an empty tile", [
        E._full(x, 300, s, 1, "MUMMUMM"), E._full(x, 300, s, 2, "UMMUMMM"), E._full(x, 300, s, 1, "MMMMMMM"), E._full(x, 300, s, 2, "UUUUUUU"),
        (1, K._c2t(x + 63, 130, {s[1]: "M", s[2]: "M", s[3]: "U", s[4]: "M"}), None),
        (2, K._g2a(x + 64, 130, {s[1]: "U", s[2]: "M", s[3]: "M"}), None),
        (1, K._c2t(x, 70, {s[0]: "M", s[1]: "M", s[2]: "M"}), K._c2t(x + 180, 120, {s[4]: "U", s[5]: "U", s[6]: "U"})),
    ], x, x + 299, K.ref_with_sites(x, 300, s))
    blocks = [tiles] + E.targeted_blocks() + [dict(K.hand_block()), E.hand_block()]
    out = []
    for b in blocks:
        for ms in (1, 3):
            out.append(with_regions(b, edge_regions(b), dict(PAR, min_sites=ms), "%s, edges, min_sites %d" % (b["name"], ms)))
    return out


def candidates_block(n):
    """One template over 300 positions (and three shorter ones) under n staggered regions that all hold some of its sites."""
    x = 2000
    s = [x + 4 + 6 * i for i in range(49)]
    rng = np.random.default_rng(n)
    st = "".join(rng.choice(list("MU"), 49))
    b = K.block("%d candidates" % n, [
        E._full(x, 300, s, 1, st), E._full(x, 300, s, 2, st[::-1]),
        (1, K._c2t(x + 100, 60, {p: "M" for p in s if x + 100 <= p < x + 160}), None),
        (2, K._g2a(x + 200, 90, {p: "U" for p in s if x + 199 <= p < x + 289}), None),
    ], x, x + 299, K.ref_with_sites(x, 300, s))
    return with_regions(b, [(x - 1 + i, x + 150 + i) for i in range(n)])


def first_long_block():
    """A whole-block region ahead of 300 short ones, on a seeded block of 3 000 positions."""
    b = E.dense_block(3001, 3000, 400)
    x = b["x"]
    return with_regions(b, [(max(x - 1, 0), b["y"])] + [(x + 10 * i, x + 10 * i + 35) for i in range(300)], name="a whole-block region ahead of 300 short ones")


def long_read_blocks():
    b = E.long_read_block()
    x, y = b["x"], b["y"]
    return [with_regions(b, [(x - 1, y)], name="long read, one long region"),
            with_regions(b, [(x - 1 + 25 * i, x + 24 + 25 * i) for i in range(200)], name="long read, 200 short regions"),
            with_regions(b, [(x - 1, y)] + [(x - 1 + 25 * i, x + 24 + 25 * i) for i in range(200)], dict(PAR, min_sites=1), name="long read, both")]


def contention_blocks(n=5000):
    out = []
    for spread in (False, True):
        b = E.contention_block(n, spread)  # four sites: code 5 = M U M U (X), or the sixteen codes in turn (all three classes)
        out.append(with_regions(b, [(b["x"] - 1, b["y"])]))
    return out


def random_regions(seed, x, y, n, lo=1, hi=600):
    rng = np.random.default_rng(seed)
    a = rng.integers(max(x - 100, 0), y + 50, n)
    return [(int(s), int(s + ln)) for s, ln in zip(a, rng.integers(lo, hi + 1, n))]


COUNTS = (0, 1, 63, 64, 65, 4113)


def count_block(nr):
    b = E.dense_block(7000 + nr, 2000, nr)
    return with_regions(b, random_regions(nr, b["x"], b["y"], 60, 1, 400), name="%d templates" % nr)


def big_block():
    """20 003 positions, 3 000 templates, 1 000 random intervals of 1 .. 600 bases."""
    b = E.big_block()
    return with_regions(b, random_regions(E.BIG_SEED, b["x"], b["y"], 1000), name="20 003 positions, 1 000 intervals")


def small_blocks():
    """Every block but the big one and the count series: the host tests and the device tests run all of them."""
    return ([hand_block(), borders_block(), borders_block(dict(PAR, min_sites=1)), borders_block({"min_sites": 1, "u_max_pct": 0, "m_min_pct": 100})]
            + edge_blocks() + [candidates_block(n) for n in (1, 63, 64, 65, 129)] + [first_long_block()] + long_read_blocks() + contention_blocks())
