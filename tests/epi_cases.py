"""Inputs of the epiallele table's tests (tests/test_epi_host.py, tests/test_gpu_epi.py): synthetic TEMPLATE arrays, their read bytes and
reference codes — a hand-worked block, the anchor on the read-level table's hand block, targeted blocks, a long read, contention and seeded
random blocks with a CpG every 8 .. 20 bases.  A block is a dict {name, tpl, seq, x, y, ref, min_qual, params} as tests/cpg_reads_cases.py
makes them; params are the epiallele table's ({"min_cov": n})."""
import numpy as np

import cpg_reads_cases as K
from bs_call_amd.abi import TEMPLATE

PAR = {"min_cov": 1}


def block(name, rows, x, y, ref, min_qual=20):
    return K.block(name, rows, x, y, ref, min_qual=min_qual, params=dict(PAR))


def rec(pos, span, **c):
    """(pos, span, c[16]) with c<code>=count."""
    cs = [0] * 16
    for k, v in c.items():
        cs[int(k[1:])] = v
    return (pos, span, cs)


def as_tuples(recs):
    return [(int(r["pos"]), int(r["span"]), [int(v) for v in r["c"]]) for r in recs]


# ---- the hand-worked block: 9 templates over the 7 sites 203, 208, 214, 221, 230, 240, 251 of positions 201 .. 260 ----------------------------
HAND_SITES = (203, 208, 214, 221, 230, 240, 251)


def hand_block():
    """Windows w0 = (203, 208, 214, 221) span 18, w1 = (208 .. 230) span 22, w2 = (214 .. 240) span 26, w3 = (221 .. 251) span 30; min_qual 20.
      T1 C2T 201 .. 260:           M M U M U U M   k 7   w0 MMUM = 1+2+8 = 11, w1 MUMU = 1+4 = 5, w2 UMUU = 2, w3 MUUM = 1+8 = 9   bits 3+2+1+2 = 8
      T2 G2A 204 .. 242:           U U U U M M .   k 6   w0 UUUU = 0, w1 UUUM = 8, w2 UUMM = 4+8 = 12; w3 holds 251, whose G (252) it lacks   bits 0+1+2 = 3
      T3 C2T 201 .. 216 + 228 .. 260: M M M . M M M  k 6   221 lies in the gap, and every window holds 221: no pattern
      T4 C2T 206 .. 245:           . M M q M M .   k 4   quality 19 at 221, in the middle of w1 and w2: no pattern
      T5 G2A 209 .. 232:           . M U U M . .   k 4   exactly four states: w1 MUUM = 9   bits 2
      T6 C2T 212 .. 245:           . . M M M g .   k 3   a G at 240: three states, no pattern, not in totals[4]
      T7 C2T 219 .. 235 + 228 .. 256: . . . M U M M  k 4   both mates read 230: read 0 says U, read 1 M, read 0 decides; w3 MUMM = 1+4+8 = 13   bits 3
      T8 bs_strand 0 over all:     ignored
      T9 G2A 204 .. 225:           M M U M . . .   k 4   w0 MMUM = 11   bits 3
    w0: c0 1 (T2), c11 2 (T1 T9): n 3, k 2.   w1: c5 1 (T1), c8 1 (T2), c9 1 (T5): n 3, k 3.   w2: c2 1 (T1), c12 1 (T2): n 2, k 2.
    w3: c9 1 (T1), c13 1 (T7): n 2, k 2.
    totals: 4 windows, 10 observations, 5 templates with a pattern (T1 T2 T5 T7 T9), 8 + 3 + 2 + 3 + 3 = 19 M bits, 7 templates with k >= 4
    (all but T6 and T8)."""
    c2t, g2a = K._c2t, K._g2a
    rows = [
        (1, c2t(201, 60, {203: "M", 208: "M", 214: "U", 221: "M", 230: "U", 240: "U", 251: "M"}), None),
        (2, g2a(204, 39, {203: "U", 208: "U", 214: "U", 221: "U", 230: "M", 240: "M"}), None),
        (1, c2t(201, 16, {203: "M", 208: "M", 214: "M"}), c2t(228, 33, {230: "M", 240: "M", 251: "M"})),
        (1, c2t(206, 40, {208: "M", 214: "M", 221: ("C", 19), 230: "M", 240: "M"}), None),
        (2, g2a(209, 24, {208: "M", 214: "U", 221: "U", 230: "M"}), None),
        (1, c2t(212, 34, {214: "M", 221: "M", 230: "M", 240: "G"}), None),
        (1, c2t(219, 17, {221: "M", 230: "U"}), c2t(228, 29, {230: "M", 240: "M", 251: "M"})),
        (0, c2t(201, 60, {p: "M" for p in HAND_SITES}), None),
        (2, g2a(204, 22, {203: "M", 208: "M", 214: "U", 221: "M"}), None),
    ]
    return block("hand", rows, 201, 260, K.ref_with_sites(201, 60, HAND_SITES))


HAND_RECORDS = [rec(203, 18, c0=1, c11=2), rec(208, 22, c5=1, c8=1, c9=1), rec(214, 26, c2=1, c12=1), rec(221, 30, c9=1, c13=1)]
HAND_TOTALS = (4, 10, 5, 19, 7, 0, 0, 0)
HAND_TABLE = (b"chrE\t202\t222\t3\t2\t1\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t2\t0\t0\t0\t0\n"
              b"chrE\t207\t231\t3\t3\t0\t0\t0\t0\t0\t1\t0\t0\t1\t1\t0\t0\t0\t0\t0\t0\n"
              b"chrE\t213\t241\t2\t2\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t0\n"
              b"chrE\t220\t252\t2\t2\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t0\t1\t0\t0\n")

# the read-level table's hand block (K.hand_block: sites 103, 107, 110, 120, 125): T1 reads M U M M U, so w0 = (103 .. 120) MUMM = 1+4+8 = 13 and
# w1 = (107 .. 125) UMMU = 2+4 = 6; T2 and T3 have three states, T4 has 107 and 110 in its gap, T6 two states
ANCHOR_RECORDS = [rec(103, 17, c13=1), rec(107, 18, c6=1)]
ANCHOR_TOTALS = (2, 2, 1, 5, 1, 0, 0, 0)  # 3 + 2 M bits; T1 alone has four states or more
ANCHOR_TABLE = (b"chrT\t102\t121\t1\t1" + b"\t0" * 13 + b"\t1\t0\t0\n" + b"chrT\t106\t126\t1\t1" + b"\t0" * 6 + b"\t1" + b"\t0" * 9 + b"\n")


# ---- the targeted blocks: at most 300 positions and 8 templates each ---------------------------------------------------------------------------
def _full(x, n, sites, strand, states):
    """A read over the whole block (one base further for G2A, so that the G of every site but one at y is its) with `states` at the sites."""
    st = {p: s for p, s in zip(sites, states)}
    if strand == 2:
        return (2, K._g2a(x, n + 1, st), None)
    return (strand, K._c2t(x, n, st), None)


def targeted_blocks():
    out = []
    x = 1000
    # S = 0, 1, 3 (no window), 4 (one) and 5 (two); bs_strand 0 and 3 beside the two strands
    for S in (0, 1, 3, 4, 5):
        s = [x + 10 + 12 * i for i in range(S)]
        out.append(block("S = %d" % S, [
            _full(x, 120, s, 1, "MMUMU"), _full(x, 120, s, 2, "UMMUM"), _full(x, 120, s, 0, "MMMMM"), _full(x, 120, s, 3, "MMMMM"),
            (1, K._c2t(x + 15, 60, {p: "M" for p in s if x + 15 <= p < x + 75}), None),
        ], x, x + 119, K.ref_with_sites(x, 120, s)))
    # the four sites of a window in one tile, in two, three and four different tiles (tile 2 empty); a fifth site closes a second window
    for name, s in (("one tile", [3, 9, 20, 40, 50]), ("two tiles", [50, 60, 70, 80, 200]), ("three tiles", [60, 100, 120, 130, 290]),
                    ("four tiles, an empty one between", [10, 70, 200, 290, 298]), ("four tiles in a row", [63, 64 + 10, 128 + 5, 192, 256])):
        s = [x + v for v in s]
        out.append(block(name, [
            _full(x, 300, s, 1, "MUMMU"), _full(x, 300, s, 2, "UUMUM"), _full(x, 300, s, 1, "MMMMM"),
            (1, K._c2t(s[0], s[3] - s[0] + 1, {p: "U" for p in s[:4]}), None),  # from the first site's C to the fourth's
            (2, K._g2a(s[0] + 1, s[3] - s[0] + 1, {p: "M" for p in s[:4]}), None),  # from the first site's G to the fourth's
            (1, K._c2t(s[1], s[4] - s[1] + 1, {p: "M" for p in s[1:]}), None),  # the second window alone
            (2, K._g2a(x, 150, {p: "M" for p in s if p - x < 149}), K._g2a(x + 150, 150, {p: "U" for p in s if 149 <= p - x < 299})),  # mates back to back
        ], x, x + 299, K.ref_with_sites(x, 300, s)))
    # sites at lanes 0, 62 and 63: the G2A byte of lane 63 lies in the next tile
    s = [x, x + 62, x + 127, x + 190, x + 255]
    out.append(block("lanes 0, 62, 63", [
        _full(x, 300, s, 1, "MUMUM"), _full(x, 300, s, 2, "UMMUU"),
        (1, K._c2t(x + 62, 194, {p: "M" for p in s[1:]}), None),  # lane 62 to lane 63
        (2, K._g2a(x + 63, 194, {p: "U" for p in s[1:]}), None),  # the G of lane 62's site to the G of lane 63's, lane 0 of the tile behind
        (2, K._g2a(x + 1, 255, {p: "M" for p in s[:4]}), None),  # ends on the G of lane 62's site
    ], x, x + 299, K.ref_with_sites(x, 300, s)))
    # a site at p == y never has a G2A state
    s = [x + 5, x + 10, x + 30, x + 50, x + 99]
    out.append(block("a site at y", [_full(x, 100, s, 1, "MMUUM"), _full(x, 100, s, 2, "MMMMM"), (2, K._g2a(x + 20, 120, {p: "U" for p in s[2:]}), None)],
                     x, x + 99, K.ref_with_sites(x, 100, s)))
    # a stateless site at each of the four window positions: another base on one strand, a low quality on the other
    s = [x + 10, x + 20, x + 30, x + 40, x + 50]
    rows = []
    for j in range(4):
        rows.append(_full(x, 100, s, 1, ["MUMUM"[i] if i != j else "A" for i in range(5)]))
        rows.append(_full(x, 100, s, 2, ["UMMUU"[i] if i != j else ("G", 7) for i in range(5)]))
    out.append(block("a stateless site at each window position", rows, x, x + 99, K.ref_with_sites(x, 100, s)))
    # mates: read 0's byte decides in an overlap, read 1's where read 0's does not count; a template that starts and ends inside a window; a read
    # outside the read buffer (its mate alone gives the pattern)
    s = [x + 10, x + 20, x + 30, x + 40]
    b = block("mates", [
        (1, K._c2t(x + 5, 30, {s[0]: "M", s[1]: "U", s[2]: "M"}), K._c2t(x + 15, 30, {s[1]: "M", s[2]: "U", s[3]: "M"})),  # M U M M = 13
        (1, K._c2t(x + 5, 30, {s[0]: "M", s[1]: ("T", 3), s[2]: "M"}), K._c2t(x + 15, 30, {s[1]: "M", s[2]: "U", s[3]: "U"})),  # M M M U = 7
        (2, K._g2a(x + 25, 30, {s[2]: "M", s[3]: "M"}), K._g2a(x + 5, 30, {s[0]: "U", s[1]: "U", s[2]: "U"})),  # pos[1] < pos[0]: U U M M = 12
        (1, K._c2t(x + 15, 20, {s[1]: "M", s[2]: "M"}), None),  # starts and ends inside the window
        (1, K._c2t(x + 5, 40, {p: "U" for p in s}), K._c2t(x + 5, 40, {p: "M" for p in s})),  # read 0 is moved outside the buffer below: M M M M = 15
        (1, K._c2t(x + 5, 10, {s[0]: "M"}), K._c2t(x + 25, 20, {s[2]: "M", s[3]: "M"})),  # s[1] in the gap
    ], x, x + 59, K.ref_with_sites(x, 60, s))
    b["tpl"]["off"][4][0] = len(b["seq"]) - 39  # off + len = the buffer's length + 1
    out.append(b)
    return out


MATES_RECORDS = [rec(1010, 30, c13=1, c7=1, c12=1, c15=1)]


def long_read_block():
    """5 000 positions with a site every 2 bases (2 500 sites, 2 497 windows, 79 tiles): one C2T read over all of it, the same states as a G2A
    read one base on (every site's G), and a C2T read one base on (it lacks the first site); about one state in fifty is "none"."""
    x = 7
    rng = np.random.default_rng(2500)
    s = [x + 2 * i for i in range(2500)]
    st = {p: "MUA"[int(v)] for p, v in zip(s, rng.choice(3, 2500, p=[0.49, 0.49, 0.02]))}
    st_g = {p: {"A": "C"}.get(v, v) for p, v in st.items()}  # (a C at a G2A site's G: no state)
    rows = [(1, K._c2t(x, 5000, st), None), (2, K._g2a(x + 1, 5000, st_g), None), (1, K._c2t(x + 1, 5000, {p: v for p, v in st.items() if p > x}), None)]
    return block("long read", rows, x, x + 4999, K.ref_with_sites(x, 5000, s))


CONTENTION_SITES = (53, 59, 65, 71)


def contention_block(n=5000, spread=False):
    """n templates on the one window of a block of 30 positions: all with the code 5 (M U M U), or spread over the 16 codes in turn."""
    x = 50
    s = list(CONTENTION_SITES)
    codes = range(16) if spread else [5]
    tpl, seq = K.templates([(1, K._c2t(x, 30, {p: "M" if (c >> j) & 1 else "U" for j, p in enumerate(s)}), None) for c in codes])
    return dict(name="contention, %s" % ("16 codes" if spread else "one code"), tpl=np.resize(tpl, n), seq=seq, x=x, y=x + 29,
                ref=K.ref_with_sites(x, 30, s), min_qual=20, params=dict(PAR))


def dense_block(seed, n_pos, nr, x=None):
    """Seeded random templates over a reference with a CpG every 8 .. 20 bases: reads of 100 .. 150 bases whose bases are the converted
    strand's nine times in ten, pairs with inserts up to 250, absent mates, every bs_strand."""
    rng = np.random.default_rng(seed)
    x = int(rng.integers(1, 5000)) if x is None else x
    ref = rng.integers(1, 5, n_pos + 2).astype(np.uint8)
    p = int(rng.integers(0, 8))
    while p < n_pos + 1:
        ref[p], ref[p + 1] = 2, 3
        p += int(rng.integers(8, 21))
    tpl = np.zeros(nr, TEMPLATE)
    tpl["bs_strand"] = rng.choice([0, 1, 1, 1, 1, 2, 2, 2, 2, 3], nr)
    tpl["mapq"] = 60
    seq, off = [], 0
    for t in tpl:
        start = x + int(rng.integers(-60, n_pos))
        pair = (1, 3) if int(t["bs_strand"]) != 2 else (2, 0)  # C / T, or G / A
        for k in range(2):
            if rng.random() < (0.1 if k == 0 else 0.3):
                continue
            ln = int(rng.integers(100, 151))
            pos = max(1, start + (int(rng.integers(0, 250)) if k else 0))
            b = np.where(rng.random(ln) < 0.9, rng.choice(pair, ln), rng.integers(0, 4, ln)).astype(np.uint8)
            q = np.where(rng.random(ln) < 0.9, rng.integers(20, 42, ln), rng.integers(0, 64, ln)).astype(np.uint8)
            t["pos"][k], t["len"][k], t["off"][k] = pos, ln, off
            seq.append(b | q << 2)
            off += ln
    return dict(name="dense %d" % seed, tpl=tpl, seq=np.concatenate(seq) if seq else np.zeros(0, np.uint8), x=x, y=x + n_pos - 1, ref=ref, min_qual=20,
                params=dict(PAR))


# seeds for which the host form alone finds a pattern in every block (the tests assert it)
TILE_EDGE_BLOCKS = [(63, 6300), (64, 6400), (65, 6500), (127, 12700), (128, 12800), (129, 12900)]  # (positions, seed)
BIG_SEED = 20003


def big_block():
    return dense_block(BIG_SEED, 20_003, 3_000)
