"""The kernels against the REFERENCE'S OWN BINARY (oracle/_ref/libbscall_ref.so: the reference's unchanged sources behind
oracle/ref_driver.c, built by `make -C oracle ref` on a machine that has the reference's tree).  The rest of the GPU suite
compares the kernels with the oracle, this project's restatement of the reference; here the expected bytes were computed by the
reference's calc_gt_prob, call_genotypes_ML, process_template_vector, meth_profile and — for the device BAM reader's record parser
(bsc_bam_parse_kernel, bsc_bam_misms_kernel, bsc_bam_decode_kernel) — get_next_align_details themselves.

The reference's code never runs in this process (it holds the GPU, and the reference's asserts abort): every reference result
comes from oracle.ref_loader.run_in_child — a fresh Python process that opens no GPU — once per module.  Where the binary is
absent the tests do not skip: they fall back to tests/golden/ref_vectors.json / .bin, recorded from the same binary (smaller inputs:
2048 sites, one heterozygous-dense block, one block of 119 raw templates), and to tests/golden/ref_align_details.json / .bin (the
reduced set of BAM records of tests/bam_record_cases.py), and print that they did.

Flavour policy as in tests/test_gpu_parity.py: with libm_exact every byte; otherwise integers exact, doubles to 1e-11."""
import os

import numpy as np
import pytest
import torch

import bs_call_amd as B
from bs_call_amd.abi import GT_METH, PILEUP, VCF_CORE
from bs_call_amd.caller import ReadProfile
from oracle import ref_loader as R

import bam_record_cases as BC
import ref_pin_cases as K
import test_gpu_bamdev as GB
import test_gpu_parity as TP
import test_gpu_reads_chain as RC
import test_prep as T
import test_ref_pin as CP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = np.array([0.01, 0.05, 2.0, 20, 3], dtype=np.float64)  # the defaults; 3 calc threads
# BSC_REF_PIN_GOLDEN=1: take the fallback although the binary is there (how the fallback itself is checked on a machine that has it)
HAVE_REF = R.available() and not os.environ.get("BSC_REF_PIN_GOLDEN")


def _say_fallback(what):
    print("\n[ref pin] oracle/_ref/libbscall_ref.so is absent (recipe: `%s`): %s from tests/golden/ref_vectors.json" % (R.RECIPE, what))


@pytest.fixture(scope="module")
def full():
    c = B.SiteCaller()
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_cu():
    """a context whose kernels run on a one-CU grid: the grid-stride rounds see these inputs too"""
    old = os.environ.get("BSC_NUM_CUS")
    os.environ["BSC_NUM_CUS"] = "1"
    try:
        c = B.SiteCaller()
    finally:
        if old is None:
            os.environ.pop("BSC_NUM_CUS", None)
        else:
            os.environ["BSC_NUM_CUS"] = old
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _same_gtm(got, want, libm_exact, what):
    if libm_exact:
        CP._same_records(want, got, what)
    else:
        TP._assert_close(got, want)


# ---- the site arithmetic: bsc_call_sites and the pile-up-in chain against calc_gt_prob ---------------------------------------------
def _pile_of_sites(g):
    """pile-ups whose summary is exactly (counts, qual): everything on the forward row, quality sums = counts * qual"""
    pile = np.zeros(len(g), dtype=PILEUP)
    pile["counts"][:, 0, :] = g["counts"]
    pile["n"] = g["counts"].sum(axis=1)
    pile["quality"] = (g["counts"] * g["qual"]).astype(np.float32)
    pile["mapq2"] = (3600.0 * pile["n"]).astype(np.float32)
    return pile


@pytest.fixture(scope="module")
def sites(oracle, tables):
    """(pile-ups, reference codes n + 2, covered mask, the reference's gt_prob / max_gt of the covered positions)"""
    if HAVE_REF:
        pile, _ = K.adversarial_pileups(np.random.default_rng(20261021), 20_000 + 37)
        ref2 = np.random.default_rng(5).integers(0, 5, len(pile) + 2).astype(np.uint8)
        g, rf = K.sites_from_summaries(oracle, tables, pile, ref2[: len(pile)])
        want = R.run_in_child("calc_gt_prob", dict(gt=g, rf=rf, params=PARAMS[:3]))["gt"]
        assert (want["counts"] == g["counts"]).all()
    else:
        _say_fallback("the sites")
        G = CP._golden()["sites"]
        n = len(G["rf"])
        g = np.zeros(n, dtype=GT_METH)
        g["counts"], g["qual"] = np.array(G["counts"], dtype=np.uint64), np.array(G["qual"], dtype=np.int32)
        keep = (g["counts"] * g["qual"]).max(axis=1) < 2**24  # quality sums a float holds exactly
        pile = _pile_of_sites(g[keep])
        ref2 = np.concatenate([np.array(G["rf"], dtype=np.uint8)[keep], [1, 2]]).astype(np.uint8)
        want = g[keep].copy()
        want["gt_prob"] = CP._as(G["gt_prob"], "<f8").reshape(n, 10)[keep]
        want["max_gt"] = np.array(G["max_gt"], dtype=np.uint8)[keep]
    return pile, ref2, pile["n"] > 0, want


@pytest.mark.parametrize("grid", ["full", "one_cu"])
def test_call_sites_against_calc_gt_prob(request, sites, libm_exact, grid):
    c = request.getfixturevalue(grid)
    pile, ref2, cov, want = sites
    got, skip = c.call_sites(pile, ref2[: len(pile)])
    assert ((skip == 0) == cov).all() and cov.sum() >= 1500
    g = got[cov]
    assert (g["counts"] == want["counts"]).all() and (g["qual"] == want["qual"]).all()
    if libm_exact:
        bad = np.flatnonzero((g["gt_prob"].view(np.int64) != want["gt_prob"].view(np.int64)).any(axis=1) | (g["max_gt"] != want["max_gt"]))
        assert len(bad) == 0, "gt_prob / max_gt differ from the reference's at %d sites, first %s" % (len(bad), bad[:5].tolist())
    else:
        np.testing.assert_allclose(g["gt_prob"], want["gt_prob"], rtol=0, atol=1e-11)
        sp = np.sort(want["gt_prob"], axis=1)
        assert ((g["max_gt"] == want["max_gt"]) | (sp[:, -1] - sp[:, -2] < 1e-12)).all()


def test_chain_against_calc_gt_prob(full, oracle, tables, sites, libm_exact):
    """bsc_chain_device, pile-ups in: the genotype and the GLs of its records (all_positions: every covered position is
    written) are those the print stage derives from the REFERENCE's gt_prob / max_gt."""
    pile, ref2, cov, want = sites
    n = len(pile)
    gtm, skip = oracle.call_sites(pile, ref2[:n], tables, oracle.LIBM if libm_exact else oracle.BSM, -8)
    gtm["gt_prob"][cov], gtm["max_gt"][cov] = want["gt_prob"], want["max_gt"]
    exp = oracle.vcf_block(gtm, skip, ref2, 777, all_positions=True)
    d_cts, d_ref = _dev(pile), _dev(ref2)
    d_core = torch.full((n * 64,), 0xA5, dtype=torch.uint8, device=DEV)
    full.chain_device(d_cts.data_ptr(), d_ref.data_ptr(), 777, n, 0, n, d_core.data_ptr(), True, 1, 0xFFFFFFFF, None, False, None)
    torch.cuda.synchronize()
    core = d_core.cpu().numpy().view(VCF_CORE)
    for f in ("pos", "emit", "gt", "gt_enc", "n_gl", "phred", "dp"):
        assert (core[f] == exp[f]).all(), f
    if libm_exact:
        assert core["gl"].tobytes() == exp["gl"].tobytes()
    else:
        np.testing.assert_allclose(core["gl"], exp["gl"], rtol=1e-6, atol=1e-6)  # f32 fields of doubles that agree to 1e-11
    assert (exp["emit"] == 1).sum() >= 1500


# ---- blocks of reads: bsc_accumulate, bsc_call_block, bsc_reads_chain_device (both forms) against call_genotypes_ML ----------------
def _golden_block():
    G = CP._golden()["block"]
    return (CP._as(G["tpl"], np.uint8).view(B.TEMPLATE), CP._as(G["seq"], np.uint8), G["x"], G["y"], np.array(G["ref"], dtype=np.uint8),
            CP._as(G["pile"], np.uint8).view(PILEUP), CP._as(G["gtm"], np.uint8).view(GT_METH), np.array(G["skip"], dtype=np.uint8))


def _make_block(name):
    if name == "gen30":
        tpl, seq, x, y = K.generator_block(B, K.SEED + 30, 5000, 20_000, 30)
        return tpl, seq, x, y, B.synth_ref_host(K.SEED + 30, x, y - x + 3)
    if name == "gen300":
        tpl, seq, x, y = K.generator_block(B, K.SEED + 300, 5000, 3_000, 300)
        return tpl, seq, x, y, B.synth_ref_host(K.SEED + 300, x, y - x + 3)
    if name == "het_dense":
        src, refc = K.het_dense_source()
        tpl, seq, _, _ = K.expand_pileups(src, 1000)
        return tpl, seq, 1000, 1000 + len(src) - 1, np.concatenate([refc, [1, 2]]).astype(np.uint8)
    tpl, seq, x, y = K.adversarial_template_list(3)
    return tpl, seq, x, y, np.random.default_rng(3).integers(0, 5, y - x + 3).astype(np.uint8)


_BLOCKS = {}


def _block(name):
    """(tpl, seq, x, y, ref codes of x .. y + 2, the reference's pile-up, gt_meth, skip) — computed once, never written to"""
    if name not in _BLOCKS:
        if HAVE_REF:
            tpl, seq, x, y, ref2 = _make_block(name)
            r = R.run_in_child("block", dict(tpl=tpl, seq=seq, ref=ref2, xy=np.array([x, y]), params=PARAMS))
            _BLOCKS[name] = (tpl, seq, x, y, ref2, r["pile"], r["gtm"], r["skip"])
        else:
            _say_fallback("block %r replaced by the golden block" % name)
            _BLOCKS[name] = _golden_block()
    return _BLOCKS[name]


@pytest.mark.parametrize("name,grid", [("gen30", "full"), ("gen30", "one_cu"), ("gen300", "full"), ("het_dense", "full"), ("adversarial", "full")])
def test_accumulate_and_call_block_against_call_genotypes_ml(request, libm_exact, name, grid):
    c = request.getfixturevalue(grid)
    tpl, seq, x, y, ref2, wpile, wgtm, wskip = _block(name)
    CP._same_records(wpile, c.accumulate(tpl, seq, x, y), "%s: pile-up" % name)
    got, skip = c.call_block(tpl, seq, x, y, ref2[: y - x + 1])
    assert (skip == wskip).all()
    _same_gtm(got, wgtm, libm_exact, "%s: gt_meth" % name)
    if name == "het_dense" and HAVE_REF:
        het = B.GT_HET[wgtm["max_gt"]] & (wskip == 0)
        assert het.sum() >= 0.3 * (wskip == 0).sum() and (wgtm["fisher_strand"][het] != 0).any()


@pytest.mark.parametrize("fused", [False, True], ids=["summaries", "one_kernel"])
@pytest.mark.parametrize("name", ["gen30", "gen300", "het_dense", "adversarial"])
def test_reads_chain_against_call_genotypes_ml(oracle, tables, libm_exact, name, fused):
    """bsc_reads_chain_device in both forms: its records are the print stage's over the REFERENCE's gt_meth array (genotype, GLs,
    FS from fisher_strand, the filters), its half records the reference's counts / qualities / mq / aq / max_gt."""
    if not libm_exact:
        pytest.skip("host libm differs from the replica: the record bytes go through exp/log (policy of tests/test_gpu_reads_chain.py)")
    tpl, seq, x, y, ref2, wpile, wgtm, wskip = _block(name)
    n = y - x + 1
    exp = oracle.vcf_block(wgtm, wskip, ref2, x)
    with B.SiteCaller() as c:
        c.set_reads_fused(fused)
        core, aux, _, cnt = RC._reads_chain(c, tpl, seq, x, y, ref2, with_stats=False)
    RC._same_core(core, exp, "%s, fused=%s" % (name, fused))
    has = exp["pos"] != 0
    for f in ("counts", "qual", "mq", "aq", "max_gt"):
        assert (aux[f][has] == wgtm[f][has]).all(), f
    assert cnt["sites"] == n and cnt["covered"] == int((wskip == 0).sum())


# ---- raw templates: bsc_prepare_templates_device and bsc_block_records_raw against process_template_vector ------------------------
@pytest.fixture(scope="module")
def prep():
    """(raw, seq, misms, x, y, ref codes, trims / min_qual, what the reference made of them)"""
    if not HAVE_REF:
        _say_fallback("the raw templates")
        return CP.golden_prep(CP._golden())
    from oracle import py_prep

    rng = np.random.default_rng(616161)
    ts, x, y, drawn, filtered = K.prep_block(T, py_prep, rng, 400, qlo=10)
    assert filtered <= 0.05 * drawn
    raw, seq, ms = T.to_arrays(ts)
    refc = rng.integers(0, 5, y - x + 3).astype(np.uint8)
    kw = dict(left_trim=(2, 0), right_trim=(0, 3), min_qual=20)
    r = R.run_in_child("prep_block", dict(raw=raw, seq=seq, misms=ms, ref=refc, xy=np.array([x, y, x]),
                                          params=np.array([0.01, 0.05, 2.0, 20, 2, 2, 0, 0, 3], dtype=np.float64)))
    r["stats"] = [int(v) for v in r["stats"]]
    return raw, seq, ms, x, y, refc, kw, r


def test_device_preprocessing_against_process_template_vector(full, prep):
    raw, seq, ms, x, y, refc, kw, want = prep
    pf = ReadProfile(cap=4096)
    d_tpl, d_seq, d_st = full.prepare_templates_device(raw, seq, ms, profile=pf, x=x, ref=refc, **kw)
    assert len(raw) >= 100 and CP._flatten(d_tpl, d_seq) == CP._flatten(want["tpl"], want["seq"])
    assert [int(d_st[f]) for f in d_st.dtype.names] == want["stats"]
    assert pf.used == len(want["prof"]) and pf.counts[: pf.used].tolist() == want["prof"].tolist() and int(want["prof"].sum()) > 0


def test_block_records_raw_against_process_template_vector(full, oracle, prep, libm_exact):
    """bsc_block_records_raw: its packed records are the print stage's over the gt_meth array the REFERENCE computed from the
    same raw templates (process_template_vector -> call_genotypes_ML); without the binary, over the oracle's calls of the
    golden prepared templates (what the reference prepared; the calls themselves are pinned by the golden block)."""
    if not libm_exact:
        pytest.skip("host libm differs from the replica: the record bytes go through exp/log (policy of tests/test_gpu_reads_chain.py)")
    import oracle_chain as OC

    raw, seq, ms, x, y, refc, kw, want = prep
    got, st = full.block_records_raw(raw, seq, ms, x, y, refc, **kw)
    assert [int(st[f]) for f in st.dtype.names] == want["stats"]
    if "gtm" in want:
        core = oracle.vcf_block(want["gtm"], want["skip"], refc, x)
        sel = core["emit"] == 1
        OC.same_records(got, core[sel], want["gtm"][sel])
    else:
        OC.same_records(got, *OC.records(want["tpl"], want["seq"], x, y, refc))
    assert len(got) > 50


# ---- BAM records: the device reader's parse, list and decode kernels against get_next_align_details -------------------------------------
BAM_VARIANTS = [({}, "kernels"), ({"BSC_BAMDEV_REPLAY": "1"}, "replay"), ({"BSC_BAMDEV_SLAB_KB": "64", "BSC_BAMDEV_PASS_KB": "1"}, "small passes")]


@pytest.fixture(scope="module")
def bam_sets():
    """group -> RefSet (tests/bam_record_cases.py): the records with what the reference's parser made of them, from a child process or
    from the recorded fixture"""
    if not (HAVE_REF and R.has_align_details()):  # absent, or left by an earlier recipe that had no refdrv_align_details
        print("\n[ref pin] oracle/_ref/libbscall_ref.so is not used, or has no refdrv_align_details (recipe: `%s`): the reduced set of BAM records and the reference's results "
              "for it from tests/golden/ref_align_details.json" % R.RECIPE)
        return BC.golden_sets()

    def in_child(records, offsets, ku, idup):
        r = R.run_in_child("align_details", dict(records=records, offsets=offsets,
                                                 params=np.array([BC.MAPQ_THRESH, BC.MAX_TEMPLATE_LEN, int(ku), int(idup)], dtype=np.uint64)))
        return r["align"], r["misms"], r["reads"]

    return BC.live_sets(in_child)


_BAM_FILES = {}


def _bam_file(bam_sets, tmp_path_factory, group, setting=BC.SETTINGS[0]):
    """(path, reader keywords, the reference's templates, its tally, csrc/bamio.c's blocks, records left out) of a group written as a file —
    once per module.  A file group holds its records without those whose CIGAR disagrees with l_seq (they are held against the
    reference on the CPU alone); the fixed group the records a reader accepts (bam_record_cases.gpu_flag_file)."""
    key = BC.setting_key(setting)
    if (group, key) not in _BAM_FILES:
        rs = bam_sets[group]
        a = rs.res[key][0]
        keep, out = BC.gpu_flag_file(rs, key) if group == "fixed" else (BC.file_records(rs, key), [])
        path = str(tmp_path_factory.mktemp("refpin_bam") / ("%s_%s.bam" % (group, key)))
        BC.write_bam_raw(path, [rs.raws[i] for i in keep])
        kw = dict(keep_unmatched=setting[0], ignore_duplicates=setting[1])
        host = GB.TB.c_blocks(path, **kw)  # no try: the host reader accepts the file, or the test fails here
        used = [i for i in keep if int(a["ret"][i]) == 0]
        _BAM_FILES[(group, key)] = (path, kw, [BC.template_of(rs, key, i) for i in used], BC.tally(rs, key, keep), host, (keep, out))
    return _BAM_FILES[(group, key)]


def _same_as_the_reference(what, got, want_tpl, want_tally, host):
    blocks, cts, bases = got
    ts = BC.flatten_blocks(blocks)
    assert len(ts) == len(want_tpl), "%s: %d templates, the reference uses %d records" % (what, len(ts), len(want_tpl))
    for k, (t, w) in enumerate(zip(ts, want_tpl)):
        assert t == w, "%s: template %d: reference %s, device %s" % (what, k, w, t)
    assert (cts, bases) == want_tally, what
    assert got == host, what + ": csrc/bamio.c's blocks"


@pytest.mark.parametrize("variant", range(len(BAM_VARIANTS)), ids=[v[1].replace(" ", "_") for v in BAM_VARIANTS])
@pytest.mark.parametrize("group", BC.FILE_GROUPS)
def test_device_reader_against_get_next_align_details(full, bam_sets, tmp_path_factory, group, variant):
    """The aux, CIGAR, sequence and mix groups as single-end files, one used record one template: positions, orientation, MAPQ, span,
    strand, the mismatch list and the decoded bytes of every template are the reference's per-record results, and the blocks
    csrc/bamio.c's — with the parallel kernels, with the one-lane replay, and with 64-KB slabs and 1-KB passes (the mix's 8-KB records
    lie across slabs)."""
    path, kw, want_tpl, want_tally, host, _ = _bam_file(bam_sets, tmp_path_factory, group)
    env, what = BAM_VARIANTS[variant]
    got, info = GB.dev_blocks(full, path, env, **kw)
    _same_as_the_reference("%s, %s" % (group, what), got, want_tpl, want_tally, host)
    assert info["malformed"] == 0 and len(want_tpl) == sum(len(b[2]) for b in host[0]) >= 40


def test_device_reader_against_get_next_align_details_on_a_one_cu_context(one_cu, bam_sets, tmp_path_factory):
    """The same through a context created under BSC_NUM_CUS=1.  (The reader's own grids follow the record count, not the CU count: this
    run pins that the reader does not depend on the context's grid, not a grid-stride round.)"""
    for group in BC.FILE_GROUPS:
        path, kw, want_tpl, want_tally, host, _ = _bam_file(bam_sets, tmp_path_factory, group)
        got, _ = GB.dev_blocks(one_cu, path, {}, **kw)
        _same_as_the_reference("%s, one CU" % group, got, want_tpl, want_tally, host)


@pytest.mark.parametrize("setting", [BC.SETTINGS[0], BC.SETTINGS[3]], ids=BC.setting_key)
@pytest.mark.parametrize("variant", [0, 2], ids=["kernels", "small_passes"])
def test_device_reader_flag_sweep_against_get_next_align_details(full, bam_sets, tmp_path_factory, setting, variant):
    """Every flag value with the mate right and left of the record, and the fixed fields' edge cases: the file holds the records the
    reference filters and those it uses with PAIRED cleared; lone mates, which read_input asserts on and csrc/bamio.c refuses, are left
    out — at most 2 % of the sweep.  The device's filter counters and base sums are the reference's tally, its templates the reference's
    used records."""
    path, kw, want_tpl, want_tally, host, (keep, out) = _bam_file(bam_sets, tmp_path_factory, "fixed", setting)
    n_out, n_sweep = BC.sweep_share(bam_sets["fixed"], out)
    print("\n[ref pin] flag sweep %s: %d records in the file, left out %d of the sweep's %d (%.2f %%), %d of all %d"
          % (BC.setting_key(setting), len(keep), n_out, n_sweep, 100.0 * n_out / n_sweep, len(out), len(bam_sets["fixed"])))
    assert n_out <= 0.02 * n_sweep
    env, what = BAM_VARIANTS[variant]
    got, info = GB.dev_blocks(full, path, env, **kw)
    _same_as_the_reference("flag sweep %s, %s" % (BC.setting_key(setting), what), got, want_tpl, want_tally, host)
    assert sum(want_tally[0]) > 100 and len(want_tpl) > 20 and info["malformed"] == 0
