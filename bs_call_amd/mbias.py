"""The M-bias table in Python: the rule of include/bscall_amd.h (READ, END, CYCLE, G(j), COUNTS, CONTEXT, TABLE, TOTALS, LINE) written from
the rule — the third form beside the kernel (csrc/mbiasdev.hip) and the host form (csrc/mbias.c), for tests and for users who hold raw
templates in numpy.  A read's list is first turned into a per-byte map (genome position, or -1), then the mapped bytes are classified with
numpy masks and added to the table."""

import numpy as np

from .abi import MISMS, MISMS_DEL, MISMS_INS, MISMS_MISMS, MISMS_SOFT, RAW_TEMPLATE

MAX_CYCLES = 1024
N_BINS = 12
N_TOTALS = 8
TOTAL_NAMES = ("reads", "mapped", "counted", "overflow", "cpg_meth", "cpg_unmeth", "skipped", "zero")
HEADER = b"#read\tstrand\tcontext\tcycle\tmeth\tunmeth\n"
STRANDS = ("C2T", "G2A")
CONTEXTS = ("CpG", "CHG", "CHH")


def n_cycles_of(params):
    """n_cycles of None ({512}), an int, a dict or a _lib.MbiasParams; ValueError outside 1 .. 1024."""
    if params is None:
        n = 512
    elif isinstance(params, dict):
        unknown = set(params) - {"n_cycles"}
        if unknown:
            raise ValueError("unknown mbias parameter(s): %s" % ", ".join(sorted(unknown)))
        n = params.get("n_cycles", 512)
    elif hasattr(params, "n_cycles"):
        n = params.n_cycles
    else:
        n = params
    n = int(n)
    if not 1 <= n <= MAX_CYCLES:
        raise ValueError("n_cycles must be within 1 .. %d" % MAX_CYCLES)
    return n


def empty(params=None):
    """(counts[2][2][3][n_cycles][2] of zeros, totals[8] of zeros)"""
    return np.zeros((2, 2, 3, n_cycles_of(params), 2), dtype=np.uint64), np.zeros(N_TOTALS, dtype=np.uint64)


def genome_map(pos, length, entries):
    """G(j) of every byte of one read before the block's cut: an int64 array, -1 = taken out; None for a malformed list."""
    taken = np.zeros(length, dtype=bool)
    shift = np.zeros(length + 1, dtype=np.int64)
    cursor = 0
    n = len(entries)
    for z in range(n):
        kind, at, size = int(entries["type"][z]), int(entries["position"][z]), int(entries["size"][z])
        if kind == MISMS_MISMS:
            continue
        if kind not in (MISMS_INS, MISMS_DEL, MISMS_SOFT):
            return None
        if at < cursor:
            return None
        if kind == MISMS_INS:
            cursor = at
            if at < length:
                shift[at] += size
            continue
        if kind == MISMS_SOFT and z not in (0, n - 1):
            return None
        if at + size > length:
            return None
        taken[at : at + size] = True
        cursor = at + size
    kept_before = np.cumsum(~taken) - (~taken)
    g = int(pos) + kept_before.astype(np.int64) + np.cumsum(shift[:length])
    g[taken] = -1
    return g


def add_block(counts, totals, raw, seq, misms, x, y, ref, min_qual=20):
    """One block's reads added into counts / totals (empty()'s arrays, any n_cycles): raw RAW_TEMPLATE[nr], seq their read bytes, misms
    MISMS[n], the block x .. y and ref, the codes of x .. y + 2."""
    raw = np.asarray(raw, dtype=RAW_TEMPLATE)
    seq = np.asarray(seq, dtype=np.uint8)
    misms = np.asarray(misms, dtype=MISMS)
    x, y = int(x), int(y)
    ref = np.asarray(ref, dtype=np.uint8)
    if y < x or ref.size < y - x + 3:
        raise ValueError("ref must hold the codes of x .. y + 2")
    nc = counts.shape[3]
    # r(p) for p = x - 2 .. y + 4: N outside x .. y + 2
    r = np.zeros(y - x + 7, dtype=np.uint8)
    r[2 : y - x + 5] = ref[: y - x + 3]
    for t in raw:
        bs, orient = int(t["bs_strand"]), int(t["orientation"])
        for k in range(2):
            ln = int(t["len"][k])
            if ln == 0 or bs == 0:
                continue
            off, mo, nm = int(t["off"][k]), int(t["misms_off"][k]), int(t["n_misms"][k])
            g = None
            if off + ln <= seq.size and mo + nm <= misms.size and bs in (1, 2) and orient <= 1:
                g = genome_map(t["pos"][k], ln, misms[mo : mo + nm])
            if g is None:
                totals[6] += np.uint64(1)
                continue
            totals[0] += np.uint64(1)
            b = seq[off : off + ln]
            j = np.flatnonzero((g >= x) & (g <= y))
            totals[1] += np.uint64(j.size)
            q = b[j] >> 2
            j = j[(q >= int(min_qual)) & (q < 63)]
            at = g[j] - x + 2  # index into r
            base = b[j] & 3
            if bs == 1:
                here, a1, a2, meth, unmeth = 2, r[at + 1], r[at + 2], 1, 3
            else:
                here, a1, a2, meth, unmeth = 3, r[at - 1], r[at - 2], 2, 0
            partner = 5 - here  # the other base of the CpG
            ctx = np.full(j.size, -1, dtype=np.int64)
            ctx[a1 == partner] = 0
            other1 = (a1 != 0) & (a1 != partner)
            ctx[other1 & (a2 == partner)] = 1
            ctx[other1 & (a2 != 0) & (a2 != partner)] = 2
            state = np.full(j.size, -1, dtype=np.int64)
            state[base == meth] = 0
            state[base == unmeth] = 1
            keep = (r[at] == here) & (ctx >= 0) & (state >= 0)
            j, ctx, state = j[keep], ctx[keep], state[keep]
            c = j if k == 0 else ln - 1 - j
            over = c >= nc
            totals[3] += np.uint64(over.sum())
            c, ctx, state = c[~over], ctx[~over], state[~over]
            np.add.at(counts[k ^ orient, bs - 1], (ctx, c, state), 1)
            totals[2] += np.uint64(c.size)
            totals[4] += np.uint64(((ctx == 0) & (state == 0)).sum())
            totals[5] += np.uint64(((ctx == 0) & (state == 1)).sum())
    return counts, totals


def table(raw, seq, misms, x, y, ref, min_qual=20, params=None):
    """The table of one block: add_block into empty(params)."""
    counts, totals = empty(params)
    return add_block(counts, totals, raw, seq, misms, x, y, ref, min_qual)


def format_table(counts):
    """LINE: the table's text (bytes) of counts[2][2][3][n_cycles][2]."""
    counts = np.asarray(counts, dtype=np.uint64)
    if counts.ndim != 5 or counts.shape[:3] != (2, 2, 3) or counts.shape[4] != 2:
        raise ValueError("counts must be [2][2][3][n_cycles][2]")
    out = [HEADER]
    for e in range(2):
        used = np.flatnonzero(counts[e].any(axis=(0, 1, 3)))
        if used.size == 0:
            continue
        last = int(used[-1])
        for s in range(2):
            for ctx in range(3):
                for c in range(last + 1):
                    out.append(b"%d\t%s\t%s\t%d\t%d\t%d\n" % (e + 1, STRANDS[s].encode(), CONTEXTS[ctx].encode(), c + 1, int(counts[e, s, ctx, c, 0]),
                                                              int(counts[e, s, ctx, c, 1])))
    return b"".join(out)


def read_table(text, params=None):
    """The reader of format_table's text (bytes, str or a path): counts[2][2][3][n_cycles][2]; cycles the text does not list are 0."""
    if isinstance(text, str):
        if "\n" not in text:
            with open(text, "rb") as f:
                text = f.read()
        else:
            text = text.encode()
    counts, _ = empty(params)
    lines = text.split(b"\n")
    if lines[0] + b"\n" != HEADER:
        raise ValueError("not an M-bias table: %r" % lines[0][:60])
    if lines[-1] != b"":
        raise ValueError("the table's last line is cut")
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        if len(f) != 6:
            raise ValueError("bad line: %r" % ln[:60])
        e, s, ctx, c = int(f[0]) - 1, STRANDS.index(f[1].decode()), CONTEXTS.index(f[2].decode()), int(f[3]) - 1
        if e not in (0, 1) or not 0 <= c < counts.shape[3]:
            raise ValueError("bad line: %r" % ln[:60])
        counts[e, s, ctx, c] = (int(f[4]), int(f[5]))
    return counts
