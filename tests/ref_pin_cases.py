"""Inputs shared by tests/test_ref_pin.py (CPU), tests/test_gpu_ref_pin.py (GPU) and tools/make_ref_vectors.py: what is handed
to the reference's binary (oracle/_ref/libbscall_ref.so through oracle/ref_loader.py) and to the oracle / the kernels alike.
Nothing here opens the GPU or loads the reference's library.  Every generator is seeded: the same call gives the same input."""
import numpy as np

from bs_call_amd.abi import GT_METH, PILEUP, TEMPLATE

SEED = 88172645463325252
# the parameter corners of tests/test_gpu_parity.py (test_other_parameters, test_adversarial_pileups_with_extreme_parameters)
PARAM_CORNERS = [(0.01, 0.05, 2.0), (0.02, 0.01, 1.0), (0.0, 0.0, 5.0), (0.2, 0.3, 0.5), (0.5, 0.4999, 2.0), (0.9, 0.05, 2.0),
                 (0.3, 0.69999, 2.0), (0.999, 0.0, 2.0)]


# ---- level 1: (counts[8], qual[8], rf) ------------------------------------------------------------------------------------------
def adversarial_pileups(rng, n, jitter=True, scales=(1, 3, 10, 40, 400), scale_p=None):
    """tests/test_gpu_parity.py::test_adversarial_random_pileups' input (with test_gpu_chain.py::_adversarial's uncovered
    positions): uniformly random class counts / qualities, every class combination, deep sites, exact likelihood ties."""
    pile = np.zeros(n, dtype=PILEUP)
    depth_scale = rng.choice(scales, size=n, p=scale_p)
    mask = rng.random((n, 2, 8)) < rng.choice([0.1, 0.3, 0.6, 1.0], size=(n, 1, 1))
    cnt = (rng.integers(0, 8, size=(n, 2, 8)) * depth_scale[:, None, None] * mask).astype(np.uint32)
    cnt[rng.random(n) < 0.05] = 0
    pile["counts"] = cnt
    tot = cnt.sum(axis=1)
    pile["n"] = tot.sum(axis=1)
    meanq = rng.integers(20, 44, size=(n, 8))
    jit = rng.integers(0, 2, size=(n, 8)) * (tot > 0) if jitter else 0
    pile["quality"] = (tot * meanq + jit * rng.integers(0, 1 + tot // 2)).astype(np.float32)
    pile["quality"] = np.minimum(pile["quality"], 43.0 * tot)
    pile["mapq2"] = (pile["n"] * rng.choice([0, 1, 400, 1521, 3600], size=n)).astype(np.float32)
    ref = rng.integers(0, 5, size=n).astype(np.uint8)
    return pile, ref


def boundary_pileups(rng, n):
    """tests/test_gpu_parity.py::test_summary_rounding_boundaries' input: mean qualities a few ulps around k + 0.5."""
    pile = np.zeros(n, dtype=PILEUP)
    cnt = rng.integers(1, 60, size=(n, 8)).astype(np.uint32) * (rng.random((n, 8)) < 0.7)
    pile["counts"][:, 0, :] = cnt
    pile["n"] = cnt.sum(axis=1)
    k = rng.integers(0, 43, size=(n, 8)).astype(np.float64)
    frac = rng.choice([0.5, 0.0, 0.25, 0.499999, 0.500001], size=(n, 8))
    target = ((k + frac) * cnt).astype(np.float32)
    steps = rng.integers(-3, 4, size=(n, 8))
    for s in (1, 2, 3):
        target = np.where(steps >= s, np.nextafter(target, np.float32(np.inf)), target)
        target = np.where(steps <= -s, np.nextafter(target, np.float32(-np.inf)), target)
    pile["quality"] = np.clip(target, 0, None) * (cnt > 0)
    pile["quality"] = np.minimum(pile["quality"], (43.4 * cnt).astype(np.float32))
    pile["mapq2"] = (pile["n"] * rng.choice([1, 399.5, 3600, 3599.9], size=n)).astype(np.float32)
    return pile, rng.integers(0, 5, size=n).astype(np.uint8)


def sites_from_summaries(oracle, tables, pile, ref):
    """The (counts, qual) the summary of src/call_genotypes.c:44-59 derives from pile-ups (through the oracle's restatement of
    it), as calc_gt_prob inputs: GT_METH records with only counts and qual set, covered positions only."""
    gtm, skip = oracle.call_sites(pile, ref, tables, oracle.LIBM, -8)
    keep = skip == 0
    g = np.zeros(int(keep.sum()), dtype=GT_METH)
    g["counts"], g["qual"] = gtm["counts"][keep], gtm["qual"][keep]
    return g, np.ascontiguousarray(ref[keep])


def random_sites(rng, n):
    """Random calc_gt_prob inputs: depths 1 .. 3000 per site spread over a random subset of the classes, qualities 0 .. 43."""
    g = np.zeros(n, dtype=GT_METH)
    depth = np.exp(rng.uniform(0, np.log(3000), size=n))
    present = rng.random((n, 8)) < rng.choice([0.15, 0.4, 0.8, 1.0], size=(n, 1))
    present[np.arange(n), rng.integers(0, 8, n)] = True
    w = rng.random((n, 8)) * present
    g["counts"] = np.maximum(np.rint(w / w.sum(axis=1, keepdims=True) * depth[:, None]), present).astype(np.uint64) * present
    g["qual"] = rng.integers(0, 44, size=(n, 8)) * present
    return g, rng.integers(0, 5, size=n).astype(np.uint8)


def edge_sites(rng):
    """The cases a random draw does not reach: only bisulfite-informative classes present (4 .. 7: the tied likelihoods of
    DESIGN section 2), one class of each complementary pair empty, quality 0 and quality 43 throughout, single classes at depth
    65 535, every pair of classes — each at every reference code 0 .. 4."""
    rows = []
    for a in range(8):
        for b in range(8):
            for ca, cb in ((1, 1), (7, 7), (30, 1), (65535, 65535), (65535, 1), (300, 299)):
                for qa, qb in ((0, 0), (43, 43), (20, 43), (0, 43), (1, 30)):
                    c, q = [0] * 8, [0] * 8
                    c[a], q[a] = ca, qa
                    if b != a:
                        c[b], q[b] = cb, qb
                    rows.append((c, q))
    for _ in range(20_000):  # bisulfite-informative classes only; then whole complementary halves empty
        c = [0] * 4 + [int(v) for v in rng.integers(0, 200, 4) * (rng.random(4) < 0.7)]
        rows.append((c, [0] * 4 + [int(v) for v in rng.integers(0, 44, 4)]))
    for _ in range(20_000):
        c = rng.integers(0, 65536 if rng.random() < 0.1 else 60, 8)
        c[[(0, 1, 4, 5), (2, 3, 6, 7), (4, 5, 6, 7), (0, 4), (1, 5, 7), (2, 4, 6), (3, 7)][int(rng.integers(0, 7))],] = 0
        rows.append(([int(v) for v in c], [int(v) for v in rng.integers(0, 44, 8)]))
    rows = [r for r in rows if sum(r[0]) > 0]
    g = np.zeros(len(rows) * 5, dtype=GT_METH)
    g["counts"] = np.repeat(np.array([r[0] for r in rows], dtype=np.uint64), 5, axis=0)
    g["qual"] = np.repeat(np.array([r[1] for r in rows], dtype=np.int32), 5, axis=0) * (g["counts"] > 0)
    return g, np.tile(np.arange(5, dtype=np.uint8), len(rows))


def fisher_tables(rng, n, top=46340):
    """2 x 2 tables with entries up to `top` (46 340 = floor(sqrt(2^31)): beyond it the reference's int products overflow):
    small, lopsided, balanced, zero margins, and entries across the lfact_store / lgamma switch at 256."""
    c = np.zeros((n, 4), dtype=np.int32)
    kind = rng.choice(5, size=n, p=[0.3, 0.35, 0.31, 0.02, 0.02])  # the walk over a table is as long as its entries are large
    hi = np.array([8, 300, 5000, top + 1, top + 1])[kind]
    c[:] = rng.integers(0, hi[:, None], size=(n, 4))
    c[kind == 4] = (c[kind == 4] // 2 + top // 2)  # all four large
    z = rng.random((n, 4)) < 0.1
    c[z] = 0
    edge = np.array([[0, 0, 0, 0], [top, top, top, top], [top, 0, 0, top], [0, top, top, 0], [255, 256, 257, 254], [1, 0, 0, 0],
                     [top, 1, 1, top], [1, top, top, 1], [128, 127, 1, 0]], dtype=np.int32)
    return np.concatenate([edge, c])


# ---- level 2: blocks of prepared templates ----------------------------------------------------------------------------------------
def generator_block(B, seed, x0, n, cov, pad=2):
    """tests/test_gpu_accumulate.py::_block: the read generator's block."""
    tpl, seq = B.synth_reads_host(seed, x0, n, cov)
    x = max(1, x0 - pad)
    y = int((tpl["pos"] + tpl["len"]).max()) - 1 if len(tpl) else x0 + n
    return tpl, seq, x, y


def adversarial_template_list(seed):
    """tests/test_gpu_accumulate.py::test_adversarial_template_lists' lists: arbitrary order, mates far apart or swapped, reads
    of 1 .. 400 bases, reads over the block end or beyond it, absent / fully trimmed / quality-0 reads, identical templates."""
    rng = np.random.default_rng(4242 + seed)
    n_pos = int(rng.choice([1, 63, 64, 65, 1000, 20_000]))
    x = int(rng.integers(1, 1_000_000))
    y = x + n_pos - 1
    nt = int(rng.choice([0, 1, 7, 300, 5000]))
    if seed == 4:
        n_pos, nt = 20_000, 5000
        y = x + n_pos - 1
    tpl = np.zeros(nt, dtype=TEMPLATE)
    chunks, off = [], 0
    for i in range(nt):
        fwd = x + int(rng.integers(0, n_pos + 50))
        gap = int(rng.choice([0, 1, 50, 300, 3000])) * int(rng.choice([1, -1]))
        rev = max(x, fwd + gap)
        tpl["orientation"][i] = rng.integers(0, 2)
        tpl["bs_strand"][i] = rng.integers(0, 3)
        for k, pos in ((0, fwd), (1, rev)):
            kind = rng.integers(0, 10)
            if kind == 0:
                continue
            rl = int(rng.choice([1, 2, 30, 100, 400]))
            q = rng.integers(1, 44, size=rl).astype(np.uint8)
            b = rng.integers(0, 4, size=rl).astype(np.uint8)
            if kind == 1:
                q[:] = 63
            elif kind == 2:
                q[: rl // 3] = 63
                q[rl - rl // 4:] = 0
            elif kind == 3 and k == 0:
                q[:] = 0  # a quality-0 read 0: never walked, the orientation does not flip
            tpl["pos"][i, k] = pos
            tpl["len"][i, k] = rl
            tpl["off"][i, k] = off
            tpl["mapq"][i, k] = rng.integers(0, 61)
            chunks.append(b | (q << 2))
            off += rl
        if tpl["len"][i, 0] == 0 and tpl["len"][i, 1] == 0:
            tpl["pos"][i, 0], tpl["len"][i, 0], tpl["off"][i, 0] = x, 1, off
            chunks.append(np.array([1 | (30 << 2)], dtype=np.uint8))
            off += 1
    if nt >= 300:
        tpl[10:60] = tpl[5]
    seq = np.concatenate(chunks) if chunks else np.zeros(1, dtype=np.uint8)
    return tpl, seq, x, y


def mapq255_block(x=500):
    """MAPQ 255 at depth 258: mapq2 = 258 * 65 025 = 16 776 450, the last depth at which every partial sum of the f32
    accumulation stays below 2^24 and so exact (259 * 65 025 > 2^24); next to it a position one template shallower."""
    n0, n1 = 258, 257
    tpl = np.zeros(n0 + n1, dtype=TEMPLATE)
    tpl["pos"][:n0, 0], tpl["pos"][n0:, 0] = x + 2, x + 3
    tpl["len"][:, 0] = 1
    tpl["off"][:, 0] = np.arange(n0 + n1)
    tpl["mapq"][:, 0] = 255
    tpl["orientation"] = np.arange(n0 + n1) % 2
    tpl["bs_strand"] = np.arange(n0 + n1) % 3
    seq = ((np.arange(n0 + n1) % 4) | ((20 + np.arange(n0 + n1) % 24) << 2)).astype(np.uint8)
    return tpl, seq, x, x + 6


def het_dense_source(n=1500, seed=20261020):
    """The adversarial pile-ups the expansion below starts from: depths weighted so that most positions can be expanded
    exactly (the rest — sums beyond what f32 adds exactly in any order — are there on purpose: they are dropped)."""
    rng = np.random.default_rng(seed)
    pile, ref = adversarial_pileups(rng, n, scales=(1, 3, 10, 40, 400), scale_p=(0.37, 0.3, 0.2, 0.1, 0.03))
    ref[ref == 0] = 1 + rng.integers(0, 4, int((ref == 0).sum()))
    return pile, ref


# class -> (bs_strand, base) with base_tab_st[bs_strand][base] - 1 == class (src/call_genotypes.c:17-19)
_CLASS_ST = np.array([0, 0, 0, 0, 2, 1, 2, 1], dtype=np.uint8)
_CLASS_BASE = np.array([0, 1, 2, 3, 0, 1, 2, 3], dtype=np.uint8)


def expand_pileups(pile, x, min_qual=20):
    """One one-base template per counted base of every pile-up: orientation = the strand row, bs_strand and base chosen so
    that base_tab_st gives the class, integer qualities (min_qual .. 43) adding up to the class's quality sum, one MAPQ m per
    position with n * m * m = mapq2.  Positions that cannot be written this way exactly are dropped (returned emptied):
    a non-integer or out-of-range quality sum, no such m, or sums of 2^24 and more, which f32 adds order-dependently.
    -> (TEMPLATE[], seq, the pile-ups the expansion must reproduce, dropped mask)."""
    cnt = pile["counts"].astype(np.int64)  # n x 2 x 8
    tot = cnt.sum(axis=1)
    n_site = pile["n"].astype(np.int64)
    S = pile["quality"].astype(np.float64)
    ok_q = ((S == np.floor(S)) & (S >= min_qual * tot) & (S <= 43 * tot)).all(axis=1)
    m = np.sqrt(pile["mapq2"].astype(np.float64) / np.maximum(n_site, 1))
    ok_m = (m == np.floor(m)) & (m <= 255)
    exact = (n_site * np.maximum(m, 1) ** 2 < 2**24) & (S.max(axis=1) < 2**24)
    good = ok_q & ok_m & exact & (n_site == tot.sum(axis=1))
    dropped = (n_site > 0) & ~good
    want = pile.copy()
    want[~good] = np.zeros(1, dtype=PILEUP)
    cnt = cnt * good[:, None, None]
    tot = tot * good[:, None]
    # templates ordered by (position, class, strand row): the rank of a template within its (position, class) group decides
    # which of them carry the remainder of the quality sum
    per = np.transpose(cnt, (0, 2, 1)).reshape(-1)  # index = (i * 8 + c) * 2 + ori
    idx = np.repeat(np.arange(per.size), per)
    i, c, ori = idx // 16, (idx // 2) % 8, idx % 2
    group = i * 8 + c
    start = np.concatenate([[0], np.cumsum(tot.reshape(-1))])[group]
    rank = np.arange(idx.size) - start
    Si, ti = S.astype(np.int64).reshape(-1)[group], np.maximum(tot.reshape(-1)[group], 1)
    q = Si // ti + (rank < Si % ti)
    tpl = np.zeros(idx.size, dtype=TEMPLATE)
    tpl["pos"][:, 0] = x + i
    tpl["len"][:, 0] = 1
    tpl["off"][:, 0] = np.arange(idx.size)
    tpl["mapq"][:, 0] = m.astype(np.int64)[i]
    tpl["orientation"] = ori
    tpl["bs_strand"] = _CLASS_ST[c]
    seq = (_CLASS_BASE[c] | (q << 2)).astype(np.uint8)
    return tpl, seq, want, dropped


# ---- level 3: raw templates -------------------------------------------------------------------------------------------------------
def prep_block(T, py_prep, rng, n_templates, x0=1000, spread=4000, qlo=5):
    """A block of random alignments (tests/test_prep.py's generator) the reference accepts: every template is filtered on
    its own through oracle/py_prep.py (soft clips off the read's end, indels the overlap trimming leaves beyond the read — where
    the reference exits or is undefined); a leading single-read template starts the block, since process_template_vector takes
    the block start from its first template and asserts that none starts before it.
    -> (template dicts, x, y, n_drawn, n_filtered)."""
    ts, n_filtered = [], 0
    for _ in range(n_templates):
        r0, m0, s0 = T._random_read(rng, qlo)
        r1, m1, s1 = T._random_read(rng, qlo)
        kind = rng.random()
        p0 = x0 + 200 + int(rng.integers(0, spread))  # a reverse read may start a read length to the left
        if kind < 0.15:
            t = T.tpl((p0, 0), (s0, 0), (r0, None), (m0, ()))
        elif kind < 0.3:
            t = T.tpl((0, p0), (0, s1), (None, r1), ((), m1))
        else:
            t = T.tpl((p0, max(1, p0 + int(rng.integers(-s1 - 5, s0 + 30)))), (s0, s1), (r0, r1), (m0, m1))
        t["orientation"] = int(rng.integers(0, 2))
        t["bs_strand"] = int(rng.integers(0, 3))
        t["mapq"] = [int(rng.integers(0, 61)), int(rng.integers(0, 61))]
        try:
            py_prep.prepare([t])
        except py_prep.PrepError:
            n_filtered += 1
            continue
        ts.append(t)
    lead = T.tpl((x0, 0), (12, 0), (T.read(12, 1, 33), None))
    ts = [lead] + ts
    out, _ = py_prep.prepare(ts)
    y = max(o["pos"][k] + len(o["reads"][k]) for o in out for k in range(2) if o["reads"][k]) + 1
    assert min(p for o in out for p in o["pos"] if p) >= x0 - 2  # negative "overlaps" move a start left by a few bases at most
    return ts, x0 - 2, y, n_templates, n_filtered
