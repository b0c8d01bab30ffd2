"""Inputs of the read-level CpG table's tests (tests/test_cpg_reads_host.py, tests/test_gpu_cpg_reads.py): synthetic TEMPLATE arrays, their
read bytes and reference codes — the hand-worked block, the targeted blocks and seeded random ones.  A block is a dict
{name, tpl, seq, x, y, ref, min_qual, params}."""
import numpy as np

from bs_call_amd.abi import TEMPLATE

BASE = {"A": 0, "C": 1, "G": 2, "T": 3}
CODE = {"N": 0, "A": 1, "C": 2, "G": 3, "T": 4}


def ref_of(text):
    return np.array([CODE[c] for c in text], np.uint8)


def ref_with_sites(x, n, sites, fill="A"):
    """n + 2 codes for x .. x + n + 1: `fill` everywhere, C G at every p, p + 1 of `sites`."""
    r = np.full(n + 2, CODE[fill], np.uint8)
    for p in sites:
        r[p - x] = 2
        if p + 1 - x < n + 2:
            r[p + 1 - x] = 3
    return r


def read(pos, length, fill="G", qual=30, at=None):
    """A read of `length` bytes at `pos`: base `fill` with quality `qual`, and at[p] = base or (base, quality) at position p."""
    b = np.full(length, BASE[fill] | qual << 2, np.uint8)
    for p, v in (at or {}).items():
        base, q = v if isinstance(v, tuple) else (v, qual)
        b[p - pos] = BASE[base] | q << 2
    return pos, b


def templates(rows):
    """rows: (bs_strand, read 0 or None, read 1 or None), a read as read() gives it -> (TEMPLATE[], seq)."""
    tpl = np.zeros(len(rows), TEMPLATE)
    seq = []
    off = 0
    for t, (bs, r0, r1) in zip(tpl, rows):
        t["bs_strand"] = bs
        t["mapq"] = 60
        for k, r in enumerate((r0, r1)):
            if r is None:
                continue
            t["pos"][k], t["len"][k], t["off"][k] = r[0], len(r[1]), off
            seq.append(r[1])
            off += len(r[1])
    return tpl, (np.concatenate(seq) if seq else np.zeros(0, np.uint8))


def block(name, rows, x, y, ref, min_qual=20, params=None):
    tpl, seq = templates(rows)
    assert len(ref) == y - x + 3, name
    return dict(name=name, tpl=tpl, seq=seq, x=x, y=y, ref=ref, min_qual=min_qual, params=params or {"min_sites": 2, "min_cov": 1})


# ---- the hand-worked block: 7 templates over the 5 sites 103, 107, 110, 120, 125 of positions 101 .. 130 -----------------------------------
HAND_REF = "AACGATCGACGTTAATAATCGAATCGATAA" + "AA"
HAND_SITES = (103, 107, 110, 120, 125)


def hand_block():
    rows = [
        (1, read(101, 30, "A", at={103: "C", 107: "T", 110: "C", 120: "C", 125: "T"}), None),  # M U M M U
        (1, read(103, 8, "A", at={103: "C", 107: "C", 110: "C"}), None),  # M M M
        (2, read(104, 8, "C", at={104: "G", 108: "A", 111: "G"}), None),  # the G's of 103, 107, 110: M U M
        (1, read(101, 5, "A", at={103: "T"}), read(118, 10, "A", at={120: "T", 125: "C"})),  # U . . U M: 107 and 110 lie in the gap
        (1, read(106, 3, "A", at={107: ("C", 19)}), None),  # below min_qual: no state at all
        (2, read(119, 8, "C", at={121: "A", 126: "G"}), None),  # the G's of 120, 125: U M; two states < min_sites
        (0, read(101, 30, "C"), None),  # not converted: ignored
    ]
    return block("hand", rows, 101, 130, ref_of(HAND_REF), params={"min_sites": 3, "min_cov": 1})


# pos, dist, m, u, e, d, mm, mu, um, uu — tallied by hand from the rule (the test's docstring has the tally)
HAND_RECORDS = [
    (103, 4, 3, 1, 4, 3, 1, 2, 0, 0),
    (107, 3, 1, 2, 3, 2, 1, 0, 2, 0),
    (110, 10, 3, 0, 3, 2, 1, 0, 0, 0),
    (120, 5, 1, 2, 2, 2, 0, 1, 2, 0),
    (125, 0, 2, 1, 2, 2, 0, 0, 0, 0),
]
HAND_TOTALS = (5, 10, 6, 10, 5, 4, 3, 0)
HAND_TABLE = (b"chrT\t102\t104\t3\t1\t4\t3\t4\t1\t2\t0\t0\n"
              b"chrT\t106\t108\t1\t2\t3\t2\t3\t1\t0\t2\t0\n"
              b"chrT\t109\t111\t3\t0\t3\t2\t10\t1\t0\t0\t0\n"
              b"chrT\t119\t121\t1\t2\t2\t2\t5\t0\t1\t2\t0\n"
              b"chrT\t124\t126\t2\t1\t2\t2\t0\t0\t0\t0\t0\n")


# ---- the targeted blocks: at most 300 positions and 8 templates each (the long read apart) ---------------------------------------------------
def _c2t(pos, length, states, **kw):
    """A C2T read with state M / U / anything else at the given sites."""
    return read(pos, length, "G", at={p: {"M": "C", "U": "T"}.get(s, s) for p, s in states.items()}, **kw)


def _g2a(pos, length, states, **kw):
    """A G2A read; the states are given by SITE position, the bytes lie one further."""
    return read(pos, length, "T", at={p + 1: {"M": "G", "U": "A"}.get(s, s) for p, s in states.items()}, **kw)


def targeted_blocks():
    out = []
    x = 1000
    # a site at lanes 0 and 62 of the first tile and at lane 63 of the second (its G is lane 0 of the third)
    s = [x, x + 62, x + 127]
    out.append(block("lanes 0, 62, 63", [
        (1, _c2t(x, 200, {s[0]: "M", s[1]: "U", s[2]: "M"}), None),
        (2, _g2a(x, 200, {s[0]: "U", s[1]: "M", s[2]: "U"}), None),
        (1, _c2t(x + 62, 66, {s[1]: "M", s[2]: "M"}), None),  # starts on lane 62, ends on lane 63
        (2, _g2a(x + 63, 66, {s[1]: "M", s[2]: "M"}), None),  # its first byte is the G of the site at lane 62
        (2, _g2a(x + 128, 10, {s[2]: "U"}), None),  # the G at lane 0 of the third tile alone
        (1, _c2t(x + 127, 1, {s[2]: "U"}), None),  # one byte, at lane 63
    ], x, x + 199, ref_with_sites(x, 200, s)))
    # NEXT in the same round, in the next round, two rounds on with an empty round between, and beyond the template's end
    s = [x + 5, x + 20, x + 70, x + 200, x + 280]
    for name, ln in (("next: span of four tiles", 250), ("next: span of five tiles", 299)):
        out.append(block(name, [  # (the shorter reads end in front of the last site: its state is "none" for them)
            (1, _c2t(x, ln, {p: "MUMUM"[i] for i, p in enumerate(s) if p < x + ln}), None),
            (2, _g2a(x, ln, {p: "UUMMU"[i] for i, p in enumerate(s) if p + 1 < x + ln}), None),
            (1, _c2t(x, ln, {s[0]: "M", s[1]: "A", s[2]: "U", s[3]: "M"}), None),  # no state at the NEXT of the first site
            (1, _c2t(x + 64, ln - 64, {p: "U" for p in s[2:] if p < x + ln}), None),
            (2, _g2a(x + 6, 16, {s[1]: "M"}), None),  # begins on the G of a site whose C it does not hold... and ends behind the next
        ], x, x + 299, ref_with_sites(x, 300, s), params={"min_sites": 3, "min_cov": 1}))
    # mates: a site in the gap, pos[1] < pos[0], a read absent, overlaps
    s = [x + 10, x + 30, x + 50, x + 70, x + 90]
    out.append(block("mates", [
        (1, _c2t(x + 5, 10, {s[0]: "M"}), _c2t(x + 45, 50, {s[2]: "U", s[3]: "M", s[4]: "M"})),  # s[1] in the gap
        (1, _c2t(x + 45, 50, {s[2]: "U", s[3]: "M", s[4]: "M"}), _c2t(x + 5, 10, {s[0]: "M"})),  # pos[1] < pos[0]
        (2, None, _g2a(x + 5, 90, {p: "M" for p in s})),  # read 0 absent
        (2, _g2a(x + 5, 90, {p: "U" for p in s}), None),  # read 1 absent
        (1, _c2t(x + 5, 60, {s[0]: "M", s[1]: "G", s[2]: "M"}), _c2t(x + 25, 70, {s[1]: "M", s[2]: "U", s[3]: "U", s[4]: "U"})),  # read 0 decides
        (1, _c2t(x + 5, 60, {s[0]: "M", s[1]: ("C", 5), s[2]: ("C", 63)}), _c2t(x + 25, 70, {s[1]: "U", s[2]: "U", s[3]: "U"})),  # read 1 where 0 fails
        (2, _g2a(x + 60, 40, {s[3]: "M", s[4]: "U"}), _g2a(x + 5, 60, {s[0]: "U", s[1]: "U", s[2]: "U"})),
        (1, None, None),  # both absent
    ], x, x + 119, ref_with_sites(x, 120, s), params={"min_sites": 3, "min_cov": 1}))
    # qualities 0, min_qual - 1, min_qual, 62 and 63 at a site; bs_strand 0 and 3
    s = [x + 3, x + 9, x + 15, x + 21, x + 27]
    for mq in (20, 1, 43):
        quals = (0, mq - 1, mq, 62, 63)
        out.append(block("qualities, min_qual %d" % mq, [
            (1, _c2t(x, 40, {p: ("C", q) for p, q in zip(s, quals)}), None),
            (2, _g2a(x, 40, {p: ("A", q) for p, q in zip(s, quals)}), None),
            (0, _c2t(x, 40, {p: "M" for p in s}), None),
            (3, _c2t(x, 40, {p: "M" for p in s}), None),
            (1, _c2t(x, 40, {p: "U" for p in s}, qual=mq), None),
        ], x, x + 39, ref_with_sites(x, 40, s), min_qual=mq))
    # x == 1 with a site at 1; a site at y (its G is y + 1: a C2T state only); a C with ref(p + 1) == 0; a read reaching past y
    ref = ref_with_sites(1, 70, [1, 33, 70])
    ref[40 - 1] = 2
    ref[41 - 1] = 0  # C N: no site
    out.append(block("edges", [
        (1, _c2t(1, 90, {1: "M", 33: "U", 40: "C", 70: "M"}), None),
        (2, _g2a(1, 90, {1: "M", 33: "M", 70: "M"}), None),  # the byte of the site at y lies at y + 1: none
        (1, _c2t(60, 40, {70: "U"}), None),
        (2, _g2a(2, 1, {1: "U"}), None),
        (1, _c2t(71, 10, {}), None),  # wholly behind y
    ], 1, 70, ref, params={"min_sites": 2, "min_cov": 1}))
    # k_t = min_sites - 1 and min_sites, all-M, all-U and mixed; min_sites 1 and 65
    s = list(range(x + 2, x + 2 + 4 * 70, 4))  # 70 sites
    for ms in (1, 4, 65):
        rows = []
        for k in sorted({max(ms - 1, 1), ms}):
            ln = 4 * k  # covers sites s[0 .. k - 1]
            rows.append((1, _c2t(x, ln, {p: "M" for p in s[:k]}), None))
            rows.append((1, _c2t(x, ln, {p: "U" for p in s[:k]}), None))
            rows.append((2, _g2a(x, ln, {p: "MU"[(i * 7 // 3) & 1] for i, p in enumerate(s[:k])}), None))
        out.append(block("min_sites %d" % ms, rows, x, x + 299, ref_with_sites(x, 300, s), params={"min_sites": ms, "min_cov": 1}))
    return out


def long_read_block():
    """A single read of 5 000 bases over 80 sites (a span of 79 tiles), and a mate pair around it."""
    x = 7
    rng = np.random.default_rng(80)
    s = sorted(int(v) for v in rng.choice(np.arange(x, x + 4990, 3), 80, replace=False))
    st = {p: "MU"[int(rng.integers(2))] for p in s}
    rows = [(1, _c2t(x, 5000, st), None), (2, _g2a(x, 5000, st), None), (1, _c2t(x, 100, {p: "M" for p in s if p < x + 100}), _c2t(x + 4800, 200, {p: "U" for p in s if p >= x + 4800}))]
    return block("long read", rows, x, x + 4999, ref_with_sites(x, 5000, s), params={"min_sites": 4, "min_cov": 1})


def contention_block(n=5000):
    x = 50
    s = [x + 3, x + 9]
    tpl, seq = templates([(1, _c2t(x, 20, {s[0]: "M", s[1]: "U"}), None)])
    return dict(name="contention", tpl=np.repeat(tpl, n), seq=seq, x=x, y=x + 19, ref=ref_with_sites(x, 20, s), min_qual=20, params={"min_sites": 2, "min_cov": 1})


def random_block(seed, n_pos, nr, x=None, params=None):
    """Seeded random templates over a random reference in which about one position in five starts a CG."""
    rng = np.random.default_rng(seed)
    x = int(rng.integers(1, 5000)) if x is None else x
    ref = rng.integers(0, 5, n_pos + 2).astype(np.uint8)
    for p in np.flatnonzero(rng.random(n_pos + 1) < 0.2):
        ref[p], ref[p + 1] = 2, 3
    tpl = np.zeros(nr, TEMPLATE)
    tpl["bs_strand"] = rng.choice([0, 1, 1, 1, 2, 2, 2, 3], nr)
    tpl["mapq"] = 60
    seq = []
    off = 0
    for t in tpl:
        start = x + int(rng.integers(0, n_pos))
        for k in range(2):
            if rng.random() < 0.15:
                continue
            ln = int(rng.integers(1, 400 if rng.random() < 0.1 else 120))
            pos = start + int(rng.integers(0, 150)) * (k if rng.random() < 0.8 else 1 - k)
            b = rng.integers(0, 4, ln).astype(np.uint8)
            q = np.where(rng.random(ln) < 0.8, rng.integers(20, 42, ln), rng.integers(0, 64, ln)).astype(np.uint8)
            t["pos"][k], t["len"][k], t["off"][k] = pos, ln, off
            seq.append(b | q << 2)
            off += ln
    return dict(name="random %d" % seed, tpl=tpl, seq=np.concatenate(seq) if seq else np.zeros(0, np.uint8), x=x, y=x + n_pos - 1, ref=ref, min_qual=20,
                params=params or {"min_sites": 3, "min_cov": 1})
