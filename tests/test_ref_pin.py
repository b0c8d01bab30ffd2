"""The oracle (oracle/bsc_oracle.c, orc_model.inc, py_model.py, py_prep.py) and the host pre-processing (csrc/prep.c) against
the REFERENCE'S OWN BINARY: oracle/_ref/libbscall_ref.so, compiled by `make -C oracle ref` from the reference's unchanged
sources behind oracle/ref_driver.c.  Every other test of this suite compares the kernels with the oracle — this project's
reading of the reference; a misreading shared by both would pass them all.  Here the reading itself is checked, byte for byte:
  level 1  calc_gt_prob / fisher / lfact_store        vs orc_calc_gt_prob_array / orc_fisher_array / orc_tables_init (LIBM)
  level 2  call_genotypes_ML (HOT LOOP A + B)           vs orc_accumulate + orc_call_sites (LIBM)
  level 3  process_template_vector + meth_profile       vs csrc/prep.c (prepare_templates), py_prep.prepare, the host read profile
CPU only.  Where the reference's tree is absent and no library was shipped, these tests skip and say which recipe makes it;
tests/golden/ref_vectors.json (recorded from the binary by tools/make_ref_vectors.py) is checked everywhere."""
import importlib.util
import json
import os

import numpy as np
import pytest

import bs_call_amd as B
from bs_call_amd.abi import GT_HET, GT_METH, PILEUP, TEMPLATE
from bs_call_amd.caller import ReadProfile, prepare_templates
from oracle import py_prep, ref_loader as R

import ref_pin_cases as K
import test_prep as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "ref_vectors.json")
REF_TREE = os.environ.get("REF", "/root/reference")


@pytest.fixture(scope="module")
def ref():
    """The reference's binary.  Presence: where the reference's tree exists the recipe MUST produce a loadable library."""
    if os.path.isdir(os.path.join(REF_TREE, "include")):
        assert R.build(REF_TREE), "`%s` did not produce oracle/_ref/libbscall_ref.so although %s/include exists" % (R.RECIPE, REF_TREE)
    if not R.available():
        pytest.skip("no oracle/_ref/libbscall_ref.so and no reference tree to build it from (recipe: `%s REF=<reference root>`)" % R.RECIPE)
    R.lib()
    return R


def _same_records(got, exp, what):
    if got.tobytes() != exp.tobytes():
        for f in got.dtype.names:
            a, b = got[f], exp[f]
            if a.tobytes() != b.tobytes():
                bad = np.flatnonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))
                raise AssertionError("%s: field %s differs at %d records, first %s: reference %s, ours %s"
                                     % (what, f, len(bad), bad[:5].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))
        raise AssertionError(what + ": padding bytes differ")


def _orc_calc(oracle, tb, g, rf):
    out = g.copy()
    oracle.lib().orc_calc_gt_prob_array(out.ctypes.data, rf.ctypes.data, len(out), tb.ptr, oracle.LIBM)
    return out


# ---- presence ---------------------------------------------------------------------------------------------------------------------
def test_the_reference_binary_is_built_from_the_recipe_and_has_the_abi_layouts(ref):
    L = ref.lib()
    assert (L.refdrv_sizeof_pileup(), L.refdrv_sizeof_gt_meth(), L.refdrv_sizeof_gt_vcf()) == (PILEUP.itemsize, GT_METH.itemsize, 208)


# ---- level 1 ----------------------------------------------------------------------------------------------------------------------
def test_tables(ref, oracle, tables):
    lf, het = ref.tables()
    assert lf.tobytes() == tables.lfact_store.tobytes()
    assert het.tolist() == GT_HET.astype(int).tolist()


@pytest.mark.parametrize("corner", range(len(K.PARAM_CORNERS)))
def test_calc_gt_prob_random_sites(ref, oracle, corner):
    """1 040 000 random sites in all: 130 000 per parameter corner, all 200 bytes of every record."""
    assert 130_000 * len(K.PARAM_CORNERS) >= 10**6
    under, over, rb = K.PARAM_CORNERS[corner]
    tb = oracle.Tables(under, over, rb, 20)
    g, rf = K.random_sites(np.random.default_rng(9000 + corner), 130_000)
    _same_records(ref.calc_gt_prob_array(g, rf, under, over, rb), _orc_calc(oracle, tb, g, rf), "calc_gt_prob %s" % (K.PARAM_CORNERS[corner],))


def test_calc_gt_prob_adversarial_boundary_and_edge_sites(ref, oracle, tables):
    """The adversarial and boundary pile-ups of tests/test_gpu_parity.py and test_gpu_chain.py (counts and qualities from
    their summaries), bisulfite-only sites, empty partner classes, quality 0 and 43, depth 65 535 per class, rf 0 .. 4."""
    sets = []
    sets.append(K.sites_from_summaries(oracle, tables, *K.adversarial_pileups(np.random.default_rng(7), 200_000)))
    sets.append(K.sites_from_summaries(oracle, tables, *K.adversarial_pileups(np.random.default_rng(20261004), 150_000, jitter=False)))
    sets.append(K.sites_from_summaries(oracle, tables, *K.boundary_pileups(np.random.default_rng(17), 120_000)))
    sets.append(K.edge_sites(np.random.default_rng(3)))
    for i, (g, rf) in enumerate(sets):
        assert len(g) > 50_000
        for under, over, rb in (K.PARAM_CORNERS[0], K.PARAM_CORNERS[4 + i]):
            tb = oracle.Tables(under, over, rb, 20)
            _same_records(ref.calc_gt_prob_array(g, rf, under, over, rb), _orc_calc(oracle, tb, g, rf), "set %d at %s" % (i, (under, over, rb)))
    g, rf = sets[3]
    assert (g["counts"].max(axis=1) == 65535).any() and (g["counts"][:, :4].sum(axis=1) == 0).any()
    assert {0, 43} <= set(np.unique(g["qual"]).tolist()) and set(np.unique(rf).tolist()) == {0, 1, 2, 3, 4}


def test_calc_gt_prob_python_restatement_on_a_subset(ref):
    """oracle/py_model.py — the independently written restatement — against the binary: genotype exact, posteriors to 1e-9
    (Python's math.log / math.exp are the C library's, its summation order is the restatement's own)."""
    from oracle import py_model

    g, rf = K.random_sites(np.random.default_rng(31), 1500)
    e, erf = K.edge_sites(np.random.default_rng(3))
    pick = np.random.default_rng(32).choice(len(e), 500, replace=False)
    g, rf = np.concatenate([g, e[pick]]), np.concatenate([rf, erf[pick]])
    want = ref.calc_gt_prob_array(g, rf)
    for i in range(len(g)):
        max_gt, probs = py_model.calc_gt_prob([int(v) for v in g["counts"][i]], [int(v) for v in g["qual"][i]], int(rf[i]))
        sp = sorted(want["gt_prob"][i])
        assert max_gt == int(want["max_gt"][i]) or sp[-1] - sp[-2] < 1e-12, i
        np.testing.assert_allclose(probs, want["gt_prob"][i], rtol=0, atol=1e-9)


def test_fisher_and_lfact(ref, oracle, tables):
    """fisher bit for bit on 200 000 tables with entries up to 46 340: margins on both sides of lfact2's switch from
    lfact_store to lgamma at 256 (the store itself: test_tables)."""
    c = K.fisher_tables(np.random.default_rng(11), 200_000)
    assert int(c.max()) == 46340
    got, exp = ref.fisher_array(c), oracle.fisher_array(c, tables, oracle.LIBM)
    bad = np.flatnonzero(got.view(np.int64) != exp.view(np.int64))
    assert len(bad) == 0, "fisher differs on %d tables, first %s: reference %s, ours %s" % (len(bad), c[bad[:3]].tolist(), got[bad[:3]], exp[bad[:3]])


# ---- level 2 ----------------------------------------------------------------------------------------------------------------------
def _oracle_block(oracle, tb, tpl, seq, x, y, refc, min_qual):
    rc, pile = oracle.accumulate(tpl, seq, x, y, min_qual)
    assert rc == 0, "the reference would assert on this block: it must not be handed over"
    gtm, skip = oracle.call_sites(pile, refc[: y - x + 1], tb, oracle.LIBM, 1)
    return pile, gtm, skip


def _pin_block(ref, oracle, tpl, seq, x, y, refc, params=(0.01, 0.05, 2.0), min_qual=20, threads=(1, 3), what="block"):
    tb = oracle.Tables(*params, min_qual)
    epile, egtm, eskip = _oracle_block(oracle, tb, tpl, seq, x, y, refc, min_qual)
    outs = []
    for nt in threads:
        with ref.Session(*params, min_qual=min_qual, n_calc_threads=nt) as s:
            pile, gtm, skip = s.block(tpl, seq, x, y, refc)
        _same_records(pile, epile, "%s: pile-up (%d calc threads)" % (what, nt))
        assert (skip == eskip).all(), what
        _same_records(gtm, egtm, "%s: gt_meth (%d calc threads)" % (what, nt))
        outs.append(gtm.tobytes())
    assert all(o == outs[0] for o in outs)
    return egtm, eskip


@pytest.mark.parametrize("cov,n", [(2, 20_000), (30, 20_000), (300, 3_000)])
def test_call_genotypes_ml_generator_blocks(ref, oracle, cov, n):
    tpl, seq, x, y = K.generator_block(B, K.SEED + cov, 5000, n, cov)
    refc = B.synth_ref_host(K.SEED + cov, x, y - x + 3)
    gtm, skip = _pin_block(ref, oracle, tpl, seq, x, y, refc, what="generator %dx" % cov)
    assert int((skip == 0).sum()) > n // 2 and (cov < 300 or (gtm["counts"].sum(axis=1) >= 256).any())


@pytest.mark.parametrize("n_pos", [1, 63, 64, 65])
def test_call_genotypes_ml_block_sizes(ref, oracle, n_pos):
    """Blocks of 1, 63, 64 and 65 positions cut out of a generated block: reads hang over the block end (the walk stops at y)."""
    tpl, seq, x, _ = K.generator_block(B, K.SEED, 300, 400, 30, pad=0)
    keep = np.minimum(np.where(tpl["pos"][:, 0] > 0, tpl["pos"][:, 0], 2**31), np.where(tpl["pos"][:, 1] > 0, tpl["pos"][:, 1], 2**31)) >= x
    tpl = tpl[keep & ((tpl["pos"][:, 0] < x + n_pos) | (tpl["pos"][:, 1] < x + n_pos))]
    y = x + n_pos - 1
    refc = B.synth_ref_host(K.SEED, x, n_pos + 2)
    for threads in ((1, 3), (2,)):
        _pin_block(ref, oracle, tpl, seq, x, y, refc, threads=threads, what="%d positions" % n_pos)


@pytest.mark.parametrize("seed", range(5))
def test_call_genotypes_ml_adversarial_template_lists(ref, oracle, seed):
    """Fully trimmed read 0 and quality-0 read 0 (the orientation flip that the two `continue`s skip), reads over the block end,
    absent reads, identical templates, arbitrary order."""
    tpl, seq, x, y = K.adversarial_template_list(seed)
    refc = np.random.default_rng(seed).integers(0, 5, y - x + 3).astype(np.uint8)
    _pin_block(ref, oracle, tpl, seq, x, y, refc, what="adversarial list %d" % seed)
    if len(tpl) >= 300:  # unwalked read 0s (every quality 0 or 63) with a mate behind them are among them
        q0 = np.array([t["len"][0] > 0 and bool(((seq[int(t["off"][0]) : int(t["off"][0] + t["len"][0])] >> 2) % 63 == 0).all()) for t in tpl])
        assert (q0 & (tpl["len"][:, 1] > 0)).sum() > 20


@pytest.mark.parametrize("min_qual", [1, 20, 43])
def test_call_genotypes_ml_min_qual_and_parameters(ref, oracle, min_qual):
    tpl, seq, x, y = K.adversarial_template_list(4)
    refc = np.random.default_rng(min_qual).integers(0, 5, y - x + 3).astype(np.uint8)
    _pin_block(ref, oracle, tpl, seq, x, y, refc, params=K.PARAM_CORNERS[1 + min_qual % 3], min_qual=min_qual, what="min_qual %d" % min_qual)


def test_call_genotypes_ml_mapq_255_at_the_exact_limit(ref, oracle):
    tpl, seq, x, y = K.mapq255_block()
    gtm, skip = _pin_block(ref, oracle, tpl, seq, x, y, np.full(y - x + 3, 2, dtype=np.uint8), what="MAPQ 255")
    assert gtm["mq"][2] == 255 and gtm["counts"][2].sum() == 258 and 258 * 65025 < 2**24 <= 259 * 65025


def test_block_dense_in_heterozygous_calls(ref, oracle, tables):
    """The strand table (with its counts[0][6] term in the GT row) and fisher_strand: an adversarial pile-up expanded into
    one-base templates, through HOT LOOP A, the summary, the model and the Fisher test of the reference."""
    src, refc = K.het_dense_source()
    x = 1000
    tpl, seq, want, dropped = K.expand_pileups(src, x)
    y = x + len(src) - 1
    rc, pile = oracle.accumulate(tpl, seq, x, y, 20)
    assert rc == 0
    _same_records(pile, want, "the expansion does not reproduce its source pile-up")
    assert 0 < dropped.sum() <= 0.10 * len(src), "dropped %d of %d" % (dropped.sum(), len(src))
    refc = np.concatenate([refc, [1, 2]]).astype(np.uint8)
    gtm, skip = _pin_block(ref, oracle, tpl, seq, x, y, refc, what="heterozygous-dense block")
    cov = skip == 0
    het = GT_HET[gtm["max_gt"]] & cov
    assert het.sum() >= 0.30 * cov.sum(), "heterozygous: %d of %d covered" % (het.sum(), cov.sum())
    assert set(np.unique(gtm["max_gt"][het]).tolist()) == {1, 2, 3, 5, 6, 8}
    gt_sites = het & (gtm["max_gt"] == 8)
    assert (pile["counts"][gt_sites, 0, 6] != pile["counts"][gt_sites, 1, 6]).any()  # where the GT row's quirk changes the table
    assert (gtm["fisher_strand"][het] != 0).any()


# ---- level 3 ----------------------------------------------------------------------------------------------------------------------
def _flatten(out, oseq):
    return [{"pos": [int(v) for v in o["pos"]], "reads": [oseq[int(o["off"][k]) : int(o["off"][k]) + int(o["len"][k])].tolist() for k in range(2)],
             "mapq": [int(v) for v in o["mapq"]], "orientation": int(o["orientation"]), "bs_strand": int(o["bs_strand"])} for o in out]


def _pin_prep(ref, oracle, ts, x, y, refc, left_trim=(0, 0), right_trim=(0, 0), min_qual=20, what="prep"):
    """refc: the codes of x .. y + 2.  Reference (process_template_vector, meth_profile, call_genotypes_ML) against csrc/prep.c,
    py_prep and the oracle's accumulate / call over prep.c's output."""
    raw, seq, ms = T.to_arrays(ts)
    kw = dict(left_trim=left_trim, right_trim=right_trim, min_qual=min_qual)
    with ref.Session(min_qual=min_qual, n_calc_threads=2, left_trim=left_trim, right_trim=right_trim, with_stats=True) as s:
        r = s.prep_block(raw, seq, ms, y, refc, x)
    assert r["x"] == x
    pf = ReadProfile(cap=4096)
    h_tpl, h_seq, h_st = prepare_templates(raw, seq, ms, profile=pf, x=x, ref=refc, **kw)
    got, host = _flatten(r["tpl"], r["seq"]), _flatten(h_tpl, h_seq)
    for i, (a, b) in enumerate(zip(got, host)):
        assert a == b, "%s: prepared template %d: reference %s, csrc/prep.c %s (raw %s)" % (what, i, a, b, ts[i])
    pp = py_prep.Profile(4096)
    p_out, p_st = py_prep.prepare(ts, profile=pp, x=x, ref=[int(v) for v in refc], **kw)
    assert got == p_out, what + ": py_prep differs from the reference"
    names = ("base_none", "base_trim", "base_clip", "base_overlap", "base_lowqual", "reads", "read_bases")
    rst = {f: int(v) for f, v in zip(names, r["stats"])}
    assert rst == {f: int(h_st[f]) for f in names} == p_st, what
    assert len(r["prof"]) == pf.used == pp.used, what
    assert r["prof"].tolist() == pf.counts[: pf.used].tolist() == pp.mem[: pp.used], what + ": read profile"
    tb = oracle.Tables(0.01, 0.05, 2.0, min_qual)
    epile, egtm, eskip = _oracle_block(oracle, tb, h_tpl, h_seq, x, y, refc, min_qual)
    _same_records(r["pile"], epile, what + ": pile-up")
    assert (r["skip"] == eskip).all()
    _same_records(r["gtm"], egtm, what + ": gt_meth")
    return r, len(ts)


def _hand_worked():
    """The hand-worked cases of tests/test_prep.py (positions 100 .. 340), each as (templates, trims)."""
    rd, INS, DEL, SOFT = T.read, T.INS, T.DEL, T.SOFT
    r20 = rd(20)
    r0, r1 = rd(20, 0, 20), rd(24, 1, 40)
    cases = [
        ([T.tpl((100, 0), (10, 0), (rd(10), None))], dict(left_trim=(2, 0), right_trim=(3, 0))),
        ([T.tpl((100, 300), (10, 10), (rd(10), rd(10, 1)), orientation=1)], dict(left_trim=(1, 0))),
        ([T.tpl((100, 0), (16, 0), (r20, None), (((SOFT, 0, 3), (INS, 13, 2), (SOFT, 17, 3)), ()))], {}),
        ([T.tpl((100, 110), (20, 20), (rd(20, 0, 25), rd(20, 2, 35)))], {}),
        ([T.tpl((100, 110), (20, 20), (rd(20, 0, 30), rd(20, 2, 30)))], {}),  # equal spans, equal means: read 0 is trimmed
        ([T.tpl((100, 110), (20, 20), (rd(20, 0, 35), rd(20, 2, 25)))], {}),  # equal spans, read 1 the worse one
        ([T.tpl((100, 120), (30, 20), (rd(30), rd(20, 1)))], {}),
        ([T.tpl((115, 100), (20, 25), (rd(20), rd(25, 3)))], {}),
        ([T.tpl((115, 100), (30, 20), (rd(30), rd(20, 3)))], {}),
        ([T.tpl((100, 200), (20, 20), (rd(20), rd(20, 1))), T.tpl((100, 0), (20, 0), (rd(20), None)), T.tpl((0, 150), (0, 20), (None, rd(20, 2)))], {}),
        ([T.tpl((100, 120), (20, 20), (rd(20), rd(20, 1)))], {}),
        ([T.tpl((100, 112), (22, 24), (r0, r1), (((INS, 10, 2),), ()))], {}),
        ([T.tpl((100, 106), (22, 24), (r0, r1), (((INS, 10, 2),), ()))], {}),
        ([T.tpl((100, 110), (17, 24), (rd(20, 2, 20), r1), (((DEL, 5, 3),), ()))], {}),
        ([T.tpl((100, 120), (30, 20), (rd(30), rd(18, 1)), ((), ((INS, 6, 2),)))], {}),
        ([T.tpl((100, 130), (40, 30), (rd(40), rd(28, 1)), ((), ((INS, 15, 2),)))], {}),
        ([T.tpl((100, 120), (28, 24), (rd(28), rd(14, 2)), ((), ((INS, 4, 10),)))], {}),
        ([T.tpl((100, 0), (13, 0), (rd(12), None), (((INS, 3, 2), (DEL, 7, 1)), ()))], {}),
    ]
    return cases


def test_process_template_vector_hand_worked_cases(ref, oracle):
    """Every hand-worked case of tests/test_prep.py through the reference's own trim_read, trim_soft_clips, handle_overlap and
    indel normalisation: the right-trim quirk, the equal-span tie-break, both walks over the indel list."""
    refc = np.random.default_rng(5).integers(0, 5, 400).astype(np.uint8)
    n = 0
    for ts, kw in _hand_worked():
        # a single read leads each block: process_template_vector takes the block start from its first template, and the
        # cases with the reverse read first would start before it
        lead = T.tpl((100, 0), (12, 0), (T.read(12, 1, 33), None))
        _pin_prep(ref, oracle, [lead] + ts, 98, 345, refc[: 345 - 98 + 3], what="hand-worked case %d" % n, **kw)
        n += 1
    assert n == 18
    # the read-profile cases of tests/test_prep.py: block start 10 (first template at 11 would give 9: lead the block at 12)
    ref12 = np.array([1, 2, 1, 2, 3, 4, 3, 3, 2, 4, 1, 1, 1, 1, 1, 1], dtype=np.uint8)
    b = T.b
    rd = [b(v) for v in (3, 0, 1, 2, 3, 2, 0, 1, 3)]
    _pin_prep(ref, oracle, [T.tpl((12, 0), (9, 0), (rd, None), bs_strand=1), T.tpl((0, 12), (0, 9), (None, rd), bs_strand=1)], 10, 22, ref12[:15], what="profile")
    # a read that begins at the block start itself (position 1: x = 1), walked one reference base late
    _pin_prep(ref, oracle, [T.tpl((1, 0), (4, 0), ([b(1), b(0), b(1), b(3)], None), bs_strand=1),
                            T.tpl((3, 0), (5, 0), ([b(0), b(0), b(1), b(3), b(3), b(1)], None), (([T.SOFT, 0, 2], [T.INS, 4, 1]), ()), bs_strand=1)],
              1, 9, np.array([2, 1, 2, 4, 3, 1, 2, 1, 4, 4, 1], dtype=np.uint8), what="block-start quirk")


@pytest.mark.parametrize("trial", range(8))
def test_process_template_vector_random_alignments(ref, oracle, trial):
    """4000 random alignments in 8 blocks, fixed trims and min_qual varied; at most 5 % filtered through py_prep."""
    rng = np.random.default_rng(515151 + trial)
    lt = tuple(int(v) for v in rng.integers(0, 4, 2)) if trial % 2 else (0, 0)
    rt = tuple(int(v) for v in rng.integers(0, 4, 2)) if trial % 3 == 1 else (0, 0)
    mq = [20, 1, 43, 10, 30, 20, 5, 37][trial]
    ts, x, y, drawn, filtered = K.prep_block(T, py_prep, rng, 500)
    assert filtered <= 0.05 * drawn, "filtered %d of %d" % (filtered, drawn)
    refc = rng.integers(0, 5, y - x + 3).astype(np.uint8)
    r, _ = _pin_prep(ref, oracle, ts, x, y, refc, left_trim=lt, right_trim=rt, min_qual=mq, what="random alignments %d" % trial)
    assert int(r["stats"][3]) > 0 and int(r["prof"].sum()) > 0 and int(r["pile"]["n"].sum()) > 0


# ---- golden data: the pin where the binary is absent ------------------------------------------------------------------------------------
def _golden():
    """the JSON with every {"bin": [offset, bytes, dtype, shape]} replaced by that array of ref_vectors.bin"""
    with open(GOLDEN) as f:
        G = json.load(f)
    with open(os.path.splitext(GOLDEN)[0] + ".bin", "rb") as f:
        blob = f.read()

    def resolve(v):
        if isinstance(v, dict) and list(v) == ["bin"]:
            off, nbytes, dtype, shape = v["bin"]
            return np.frombuffer(blob[off : off + nbytes], dtype=dtype).reshape(shape).copy()
        return {k: resolve(w) for k, w in v.items()} if isinstance(v, dict) else v

    return resolve(G)


def _as(a, dtype):
    """an array of the golden file (records travel as their bytes) as `dtype`"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).view(dtype).copy()


def test_golden_vectors_against_the_oracle(oracle, libm_exact):
    """tests/golden/ref_vectors.json — what the reference's binary computed — against the oracle's LIBM flavour (bytes; on a
    host whose libm is not glibc's FMA variant the doubles to 1e-11) and its BSM flavour (bytes with libm_exact, since the two
    flavours are then the same function; 1e-11 otherwise)."""
    G = _golden()
    p = G["params"]
    tb = oracle.Tables(p["under_conv"], p["over_conv"], p["ref_bias"], p["min_qual"])
    s = G["sites"]
    n = len(s["rf"])
    g = np.zeros(n, dtype=GT_METH)
    g["counts"], g["qual"] = np.array(s["counts"], dtype=np.uint64), np.array(s["qual"], dtype=np.int32)
    rf = np.array(s["rf"], dtype=np.uint8)
    want = _as(s["gt_prob"], "<f8").reshape(n, 10)
    assert n >= 2000
    for flav in (oracle.LIBM, oracle.BSM):
        out = g.copy()
        oracle.lib().orc_calc_gt_prob_array(out.ctypes.data, rf.ctypes.data, n, tb.ptr, flav)
        if libm_exact:
            assert out["gt_prob"].tobytes() == want.tobytes() and out["max_gt"].tolist() == s["max_gt"].tolist()
        else:
            np.testing.assert_allclose(out["gt_prob"], want, rtol=0, atol=1e-11)
    f = G["fisher"]
    c = np.array(f["c"], dtype=np.int32)
    wantp = f["p"]
    assert len(c) >= 200
    for flav in (oracle.LIBM, oracle.BSM):
        got = oracle.fisher_array(c, tb, flav)
        if libm_exact:
            assert got.tobytes() == wantp.tobytes()
        else:
            np.testing.assert_allclose(got, wantp, rtol=1e-11, atol=1e-300, equal_nan=True)
    b = G["block"]
    tpl, seq = _as(b["tpl"], np.uint8).view(TEMPLATE), _as(b["seq"], np.uint8)
    refc = np.array(b["ref"], dtype=np.uint8)
    x, y = b["x"], b["y"]
    wpile, wgtm, wskip = _as(b["pile"], np.uint8).view(PILEUP), _as(b["gtm"], np.uint8).view(GT_METH), np.array(b["skip"], dtype=np.uint8)
    rc, pile = oracle.accumulate(tpl, seq, x, y, p["min_qual"])
    assert rc == 0 and pile.tobytes() == wpile.tobytes()
    for flav in (oracle.LIBM, oracle.BSM):
        gtm, skip = oracle.call_sites(pile, refc[: y - x + 1], tb, flav, 1)
        assert (skip == wskip).all()
        if libm_exact:
            _same_records(wgtm, gtm, "golden block, flavour %d" % flav)
        else:
            for fld in ("counts", "qual", "mq", "aq"):
                assert (gtm[fld] == wgtm[fld]).all()
            np.testing.assert_allclose(gtm["gt_prob"], wgtm["gt_prob"], rtol=0, atol=1e-11)
    assert GT_HET[wgtm["max_gt"]][wskip == 0].sum() >= 5 and (wgtm["fisher_strand"] != 0).any()


def golden_prep(G):
    """the level-3 part of the golden file -> (raw, seq, misms, x, y, ref codes, trims, expected dict)"""
    from bs_call_amd.abi import MISMS, RAW_TEMPLATE

    p = G["prep"]
    want = dict(tpl=_as(p["out_tpl"], np.uint8).view(TEMPLATE), seq=_as(p["out_seq"], np.uint8), stats=p["stats"],
                prof=np.array(p["prof"], dtype=np.uint64).reshape(-1, 4))
    return (_as(p["raw"], np.uint8).view(RAW_TEMPLATE), _as(p["seq"], np.uint8), _as(p["misms"], np.uint8).view(MISMS), p["x"], p["y"],
            np.array(p["ref"], dtype=np.uint8), dict(left_trim=tuple(p["left_trim"]), right_trim=tuple(p["right_trim"]), min_qual=G["params"]["min_qual"]), want)


def test_golden_prepared_templates_against_the_host_form():
    """What process_template_vector and meth_profile left of the golden block's raw templates, against csrc/prep.c."""
    raw, seq, ms, x, y, refc, kw, want = golden_prep(_golden())
    pf = ReadProfile(cap=4096)
    h_tpl, h_seq, h_st = prepare_templates(raw, seq, ms, profile=pf, x=x, ref=refc, **kw)
    assert len(raw) >= 100 and _flatten(h_tpl, h_seq) == _flatten(want["tpl"], want["seq"])
    assert [int(h_st[f]) for f in h_st.dtype.names] == want["stats"] and want["stats"][2] > 0 and want["stats"][3] > 0
    assert pf.used == len(want["prof"]) and pf.counts[: pf.used].tolist() == want["prof"].tolist() and int(want["prof"].sum()) > 0


def test_golden_vectors_regenerate_to_the_same_file(ref, tmp_path):
    spec = importlib.util.spec_from_file_location("make_ref_vectors", os.path.join(ROOT, "tools", "make_ref_vectors.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    out = tmp_path / "ref_vectors.json"
    M.write(str(out))
    for new, old in ((out, GOLDEN), (tmp_path / "ref_vectors.bin", os.path.splitext(GOLDEN)[0] + ".bin")):
        with open(old, "rb") as f:
            assert new.read_bytes() == f.read(), "tools/make_ref_vectors.py no longer reproduces %s" % os.path.relpath(old, ROOT)
