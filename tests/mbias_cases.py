"""Raw blocks for the M-bias table's tests (tests/test_mbias_host.py, tests/test_gpu_mbias.py): a builder of raw templates with mismatch lists,
the hand-made cases of the rule of include/bscall_amd.h (READ, END, CYCLE, G(j), COUNTS, CONTEXT, TABLE), every malformed-list form, and a
seeded random generator whose templates bsc_prepare_templates accepts (legal soft clips, mates that do not overlap).  A block is a dict:
name, raw, seq, misms, x, y, ref (the codes of x .. y + 2), min_qual."""
import numpy as np

from bs_call_amd.abi import MISMS, MISMS_DEL, MISMS_INS, MISMS_MISMS, MISMS_SOFT, RAW_TEMPLATE

MIN_QUAL = 20
A, C_, G_, T = 0, 1, 2, 3  # read bases
N, RA, RC, RG, RT = 0, 1, 2, 3, 4  # reference codes


def byte(base, qual=40):
    return base | (qual << 2)


class Builder:
    """Collects templates; read k is None or (pos, bytes, entries) with entries = [(type, position, size), ...]."""

    def __init__(self, name, x, ref, min_qual=MIN_QUAL):
        self.name, self.x, self.ref, self.min_qual = name, int(x), np.asarray(ref, dtype=np.uint8), min_qual
        self.raw, self.seq, self.misms = [], [], []

    def add(self, bs, orient, r0=None, r1=None, span=None):
        t = np.zeros((), dtype=RAW_TEMPLATE)
        t["bs_strand"], t["orientation"] = bs, orient
        for k, r in enumerate((r0, r1)):
            if r is None:
                continue
            pos, data, entries = r
            data = np.asarray(data, dtype=np.uint8)
            t["pos"][k], t["len"][k], t["off"][k] = pos, len(data), sum(len(s) for s in self.seq)
            t["misms_off"][k], t["n_misms"][k] = len(self.misms), len(entries)
            t["mapq"][k] = 60
            taken = sum(e[2] for e in entries if e[0] in (MISMS_DEL, MISMS_SOFT))
            gaps = sum(e[2] for e in entries if e[0] == MISMS_INS)
            t["reference_span"][k] = ((len(data) - taken + gaps) & 0xFFFFFFFF) if span is None else span[k]
            self.seq.append(data)
            self.misms.extend(entries)
        self.raw.append(t)
        return len(self.raw) - 1

    def build(self):
        raw = np.array(self.raw, dtype=RAW_TEMPLATE) if self.raw else np.zeros(0, dtype=RAW_TEMPLATE)
        seq = np.concatenate(self.seq).astype(np.uint8) if self.seq else np.zeros(0, dtype=np.uint8)
        misms = np.array(self.misms, dtype=MISMS) if self.misms else np.zeros(0, dtype=MISMS)
        return dict(name=self.name, raw=raw, seq=seq, misms=misms, x=self.x, y=self.x + len(self.ref) - 3, ref=self.ref, min_qual=self.min_qual)


def merge(name, blocks):
    """Several blocks over the same x, ref and min_qual as one (the templates, reads and lists concatenated)."""
    b0 = blocks[0]
    raws, so, mo = [], 0, 0
    for b in blocks:
        assert (b["x"], b["y"], b["min_qual"]) == (b0["x"], b0["y"], b0["min_qual"]) and b["ref"].tobytes() == b0["ref"].tobytes()
        r = b["raw"].copy()
        far = np.uint64(1) << np.uint64(63)  # (an offset far beyond its buffer stays one)
        r["off"] = np.where(r["off"] < far, r["off"] + np.uint64(so), r["off"])
        r["misms_off"] = np.where(r["misms_off"] < far, r["misms_off"] + np.uint64(mo), r["misms_off"])
        raws.append(r)
        so += len(b["seq"])
        mo += len(b["misms"])
    return dict(b0, name=name, raw=np.concatenate(raws), seq=np.concatenate([b["seq"] for b in blocks]),
                misms=np.concatenate([b["misms"] for b in blocks]))


# ---- the block worked by hand -------------------------------------------------------------------------------------------------------------------
def hand_worked():
    """x = 101, y = 112, positions 101 .. 114:  C G C A G C T T G C G  N  C  G
                                                 101 .          106 .      111 112 113 114
    Three templates; the expected cells are HAND_CELLS, the totals HAND_TOTALS (n_cycles 8)."""
    ref = [RC, RG, RC, RA, RG, RC, RT, RT, RG, RC, RG, N, RC, RG]
    b = Builder("hand", 101, ref)
    # t0: C2T, FORWARD, read[0] at 101, 6 bytes, no list: C G T A G C  ->  101 C (CpG, C: meth, cycle 0); 103 C with n1 = A, n2 = G (CHG, T:
    #     unmeth, cycle 2); 106 C with n1 = T, n2 = T (CHH, C: meth, cycle 5).  END 0.
    b.add(1, 0, (101, [byte(C_), byte(G_), byte(T), byte(A), byte(G_), byte(C_)], []))
    # t1: G2A, REVERSE, read[1] at 105 alone, 5 bytes G C T T A -> END = 1 ^ 1 = 0; cycles 4, 3, 2, 1, 0.  105 G: p1 = A, p2 = C -> CHG, base G:
    #     meth, cycle 4.  109 G: p1 = T, p2 = T -> CHH, base A: unmeth, cycle 0.
    b.add(2, 1, None, (105, [byte(G_), byte(C_), byte(T), byte(T), byte(A)], []))
    # t2: C2T, REVERSE, read[0] at 110 with a 2-byte left soft clip and a 1-base CIGAR D behind the first aligned byte: bytes T T | C . C G C
    #     (7 bytes; list SOFT 0 2, INS 3 1).  END = 0 ^ 1 = 1.  byte 2 -> 110 C, n1 = G: CpG, C: meth, cycle 2.  byte 3 -> 112 (N: no bin), byte
    #     4 -> 113 > y: no G.  Bytes with a G: 2.
    b.add(1, 1, (110, [byte(T), byte(T), byte(C_), byte(A), byte(C_), byte(G_), byte(C_)], [(MISMS_SOFT, 0, 2), (MISMS_INS, 3, 1)]))
    return b.build()


# (e, s, ctx, c, state) -> count
HAND_CELLS = {(0, 0, 0, 0, 0): 1, (0, 0, 1, 2, 1): 1, (0, 0, 2, 5, 0): 1, (0, 1, 1, 4, 0): 1, (0, 1, 2, 0, 1): 1, (1, 0, 0, 2, 0): 1}
HAND_TOTALS = (3, 6 + 5 + 2, 6, 0, 2, 0, 0, 0)


# ---- targeted cases -----------------------------------------------------------------------------------------------------------------------------
def _ctx_ref(n, seed=5):
    """A reference rich in every context, with Ns: n + 2 codes."""
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.array([RA, RC, RG, RT, RC, RG, N], dtype=np.uint8), n + 2, p=[0.17, 0.2, 0.2, 0.17, 0.1, 0.1, 0.06])
    return ref


def _read_of(ref, x, pos, n, bs, rng, quals=None):
    """n bytes that follow the reference from pos on (no list), C / G kept or converted at random."""
    out = np.zeros(n, dtype=np.uint8)
    for j in range(n):
        g = pos + j - x
        code = int(ref[g]) if 0 <= g < len(ref) else 0
        base = (code - 1) if code else int(rng.integers(0, 4))
        if bs == 1 and base == C_ and rng.random() < 0.5:
            base = T
        if bs == 2 and base == G_ and rng.random() < 0.5:
            base = A
        q = int(rng.integers(MIN_QUAL, 45)) if quals is None else quals[j % len(quals)]
        out[j] = byte(base, q)
    return out


def targeted():
    """The cases of the issue, one small block each, all over the same reference (x = 1000, 400 positions) so that they merge into one."""
    x, n = 1000, 400
    ref = _ctx_ref(n)
    # the edges: a C at y with its context behind the block, a G at x and x + 1 with its context in front of it, N in either context base
    ref[n - 1], ref[n], ref[n + 1] = RC, RA, RG  # y: CHG through y + 1, y + 2
    ref[0], ref[1] = RG, RG  # x, x + 1
    ref[50:56] = [RC, N, RG, RC, RA, N]
    ref[60:66] = [N, RA, RG, RC, N, RG]
    y = x + n - 1
    rng = np.random.default_rng(77)
    out = []

    def block(name):
        return Builder(name, x, ref)

    rd = lambda pos, ln, bs, quals=None: _read_of(ref, x, pos, ln, bs, rng, quals)
    b = block("one read of length 1")
    b.add(1, 0, (x + n - 1, [byte(C_)], []))
    b.add(2, 0, (x, [byte(G_)], []))
    out.append(b.build())
    b = block("all soft-clipped but one, and clips at both ends")
    b.add(1, 0, (1100, rd(1095, 12, 1), [(MISMS_SOFT, 0, 5), (MISMS_SOFT, 6, 6)]))
    b.add(2, 0, (1100, rd(1097, 30, 2), [(MISMS_SOFT, 0, 3), (MISMS_SOFT, 25, 5)]))
    b.add(1, 1, None, (1200, rd(1196, 30, 1), [(MISMS_SOFT, 0, 4), (MISMS_MISMS, 7, 1), (MISMS_SOFT, 28, 2)]))
    out.append(b.build())
    b = block("indels at the first and the last aligned byte, two indels in one read")
    b.add(1, 0, (1050, rd(1050, 40, 1), [(MISMS_DEL, 0, 3)]))  # CIGAR I at the first aligned byte
    b.add(1, 0, (1050, rd(1050, 40, 1), [(MISMS_INS, 0, 2)]))  # CIGAR D in front of it
    b.add(2, 0, (1050, rd(1050, 40, 2), [(MISMS_DEL, 39, 1)]))  # CIGAR I at the last aligned byte
    b.add(2, 0, (1050, rd(1050, 40, 2), [(MISMS_INS, 39, 4)]))  # CIGAR D in front of the last byte
    b.add(1, 1, (1050, rd(1050, 70, 1), [(MISMS_INS, 10, 2), (MISMS_MISMS, 12, 1), (MISMS_DEL, 30, 3), (MISMS_DEL, 33, 1), (MISMS_INS, 34, 1)]),
          (1300, rd(1300, 70, 1), [(MISMS_SOFT, 0, 2), (MISMS_DEL, 2, 1), (MISMS_INS, 66, 5), (MISMS_SOFT, 66, 4)]))
    b.add(2, 0, (1040, rd(1040, 50, 2), [(MISMS_INS, 50, 7), (MISMS_INS, 60, 1)]))  # gaps behind the read: no byte moves
    b.add(2, 0, (1040, rd(1040, 50, 2), [(MISMS_DEL, 20, 0), (MISMS_INS, 20, 0)]))  # empty entries
    out.append(b.build())
    b = block("read[1] alone, orientation 0 and 1, bs_strand 0 .. 3")
    for bs in (0, 1, 2, 3):
        for orient in (0, 1, 2):
            b.add(bs, orient, None, (1150, rd(1150, 33, bs if bs in (1, 2) else 1), []))
            b.add(bs, orient, (1150, rd(1150, 33, bs if bs in (1, 2) else 1), []), (1250, rd(1250, 21, bs if bs in (1, 2) else 1), []))
    out.append(b.build())
    b = block("the block's edges and N in the context")
    for bs in (1, 2):
        b.add(bs, 0, (x - 10, rd(x - 10, 30, bs), []), (y - 15, rd(y - 15, 30, bs), []))  # across x and across y + 2
        b.add(bs, 0, (1045, rd(1045, 30, bs), []))
        for _ in range(4):
            b.add(bs, 1, (x + n - 3, rd(x + n - 3, 3, bs), []), None)
            b.add(bs, 1, (x, rd(x, 2, bs), []), None)
    b.add(1, 0, (5, rd(5, 20, 1), []), (y + 3, rd(y + 3, 20, 1), []))  # wholly outside
    b.add(1, 0, (0xFFFFFFF0, rd(1000, 40, 1), [(MISMS_INS, 3, 0xFFFFFFFF), (MISMS_INS, 4, 0xFFFFFFFF)]))  # G beyond 32 bits
    out.append(b.build())
    b = block("qualities around the window")
    for bs in (1, 2):
        b.add(bs, 0, (1045, rd(1045, 80, bs, quals=[MIN_QUAL - 1, MIN_QUAL, 62, 63, 0, 40]), []))
    out.append(b.build())
    b = block("malformed lists and reads beyond their buffers")
    good = rd(1100, 20, 1)
    for entries in ([(MISMS_DEL, 5, 2), (MISMS_DEL, 6, 1)],  # position below the cursor
                    [(MISMS_DEL, 5, 2), (MISMS_INS, 6, 1)],
                    [(MISMS_INS, 6, 1), (MISMS_INS, 5, 1)],
                    [(MISMS_SOFT, 0, 3), (MISMS_MISMS, 0, 0), (MISMS_DEL, 2, 1)],
                    [(MISMS_DEL, 18, 3)],  # beyond len
                    [(MISMS_SOFT, 15, 6)],
                    [(MISMS_DEL, 0xFFFFFFFF, 2)],
                    [(MISMS_DEL, 2, 0xFFFFFFFF)],
                    [(MISMS_INS, 1, 1), (MISMS_SOFT, 5, 2), (MISMS_INS, 9, 1)],  # a SOFT in the middle
                    [(MISMS_MISMS, 1, 1), (MISMS_SOFT, 5, 2), (MISMS_MISMS, 9, 1)],
                    [(4, 1, 1)], [(0xFFFFFFFF, 0, 0)]):  # no such type
        b.add(1, 0, (1100, good, entries))
        b.add(2, 1, (1100, rd(1100, 20, 2), []), (1130, rd(1130, 20, 2), entries))  # the mate is walked all the same
    # legal neighbours of the above
    for entries in ([(MISMS_DEL, 5, 2), (MISMS_DEL, 7, 1)], [(MISMS_DEL, 17, 3)], [(MISMS_SOFT, 15, 5)], [(MISMS_INS, 5, 1), (MISMS_INS, 5, 1)],
                    [(MISMS_SOFT, 3, 2)], [(MISMS_MISMS, 19, 9), (MISMS_SOFT, 0, 20)], [(MISMS_INS, 0xFFFFFFFF, 0xFFFFFFFF)]):
        b.add(1, 0, (1100, good, entries))
    blk = b.build()
    # off + len one beyond seq_bytes (the last read), misms_off + n_misms one beyond the list, and both far beyond
    extra = np.zeros(4, dtype=RAW_TEMPLATE)
    extra["bs_strand"], extra["pos"], extra["len"] = 1, 1100, 10
    extra["off"][0, 0] = len(blk["seq"]) - 9
    extra["off"][1, 0] = len(blk["seq"]) - 10  # fits exactly
    extra["off"][2, 0], extra["n_misms"][2, 0], extra["misms_off"][2, 0] = 0, 2, len(blk["misms"]) - 1
    extra["off"][3, 0], extra["misms_off"][3, 1] = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF
    extra["len"][:, 1] = 0
    extra["len"][3, 1], extra["n_misms"][3, 1] = 10, 1
    blk["raw"] = np.concatenate([blk["raw"], extra])
    out.append(blk)
    return out


def long_reads(lengths=(1025, 5000)):
    """Reads longer than every n_cycles (the overflow total), as read[0] and as read[1], over a reference of their length."""
    n = max(lengths) + 50
    ref = _ctx_ref(n, seed=9)
    rng = np.random.default_rng(99)
    b = Builder("long reads", 1, ref)
    for ln in lengths:
        for bs in (1, 2):
            b.add(bs, 0, (1, _read_of(ref, 1, 1, ln, bs, rng), []), None)
            b.add(bs, 0, None, (20, _read_of(ref, 1, 20, ln, bs, rng), [(MISMS_DEL, 600, 2), (MISMS_INS, 700, 3)]))
    return b.build()


def lengths_block(lengths=(1, 63, 64, 65, 129)):
    ref = _ctx_ref(300, seed=11)
    rng = np.random.default_rng(111)
    b = Builder("read lengths around a round", 500, ref)
    for ln in lengths:
        for bs in (1, 2):
            b.add(bs, 0, (520, _read_of(ref, 500, 520, ln, bs, rng), []), (660, _read_of(ref, 500, 660, ln, bs, rng), []))
            if ln > 4:
                b.add(bs, 1, (520, _read_of(ref, 500, 520, ln, bs, rng), [(MISMS_SOFT, 0, 1), (MISMS_DEL, ln - 3, 1), (MISMS_INS, ln - 1, 2)]), None)
    return b.build()


def contention(n=5000):
    """n identical templates on one position: every lane of every wave adds to the same cells."""
    ref = _ctx_ref(200, seed=13)
    ref[20:84] = np.tile(np.array([RC, RG], dtype=np.uint8), 32)
    rng = np.random.default_rng(131)
    data = np.array([byte(C_ if j % 2 == 0 else G_) for j in range(64)], dtype=np.uint8)
    one = Builder("one", 300, ref)
    one.add(1, 0, (320, data, []), None)
    blk = one.build()
    blk["raw"] = np.repeat(blk["raw"], n)  # all of them read the same 64 bytes
    blk["name"] = "contention"
    del rng
    return blk


# ---- seeded random blocks -----------------------------------------------------------------------------------------------------------------------
def _random_read(rng, ref, x, pos, max_len, bs, clips=True, indels=True):
    """(bytes, entries, span): a read whose first aligned byte lies at pos, legal for bsc_prepare_templates."""
    n_al = int(rng.integers(1, max_len + 1))  # aligned read bytes (M and CIGAR I)
    left = int(rng.integers(1, 6)) if clips and rng.random() < 0.3 else 0
    right = int(rng.integers(1, 6)) if clips and rng.random() < 0.3 else 0
    entries = []
    if left:
        entries.append((MISMS_SOFT, 0, left))
    span, j = 0, 0  # j: aligned bytes placed
    while j < n_al:
        step = int(rng.integers(1, 40))
        step = min(step, n_al - j)
        if indels and rng.random() < 0.25 and j > 0:
            size = int(rng.integers(1, 4))
            if rng.random() < 0.5:
                entries.append((MISMS_INS, left + j, size))  # CIGAR D: a gap in the read
                span += size
            else:
                size = min(size, n_al - j)
                entries.append((MISMS_DEL, left + j, size))  # CIGAR I: bytes with no position
                j += size
                continue
        if rng.random() < 0.2:
            entries.append((MISMS_MISMS, left + j, 1))
        j += step
        span += step
    if right:
        entries.append((MISMS_SOFT, left + n_al, right))
    ln = left + n_al + right
    data = _read_of(ref, x, pos, ln, bs, rng)
    q = rng.random(ln)
    quals = np.where(q < 0.1, rng.integers(0, MIN_QUAL, ln), np.where(q < 0.13, 63, np.where(q < 0.16, 62, data >> 2)))
    data = ((data & 3) | (quals.astype(np.uint8) << 2)).astype(np.uint8)
    return data, entries, span


def random_block(seed, nr, n_pos=1500, x=2000, max_len=120, clips=True, indels=True, strands=(1, 1, 1, 2, 2, 2, 0, 3), orients=(0, 0, 0, 1, 1, 1, 1, 0)):
    """nr templates over a block of n_pos positions: one or two reads, the second always beyond the first one's span, so the mates never
    overlap; reads hang over both ends of the block.  With the default strands a quarter of the templates is skipped."""
    rng = np.random.default_rng(seed)
    ref = _ctx_ref(n_pos, seed=seed + 1)
    b = Builder("random %d x %d" % (seed, nr), x, ref)
    for _ in range(nr):
        bs, orient = int(rng.choice(strands)), int(rng.choice(orients))
        gen_bs = bs if bs in (1, 2) else 1
        p0 = int(rng.integers(max(1, x - max_len), x + n_pos + 5))
        d0, e0, s0 = _random_read(rng, ref, x, p0, max_len, gen_bs, clips, indels)
        kind = rng.random()
        if kind < 0.6:
            p1 = p0 + s0 + 1 + int(rng.integers(0, 60))
            d1, e1, s1 = _random_read(rng, ref, x, p1, max_len, gen_bs, clips, indels)
            b.add(bs, orient, (p0, d0, e0), (p1, d1, e1), span=(s0, s1))
        elif kind < 0.8:
            b.add(bs, orient, (p0, d0, e0), None, span=(s0, 0))
        else:
            b.add(bs, orient, None, (p0, d0, e0), span=(0, s0))
    return b.build()
