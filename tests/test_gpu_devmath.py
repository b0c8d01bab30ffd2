"""The device numeric primitives of csrc/callmath.h, csrc/bsmath.h and csrc/sitestats_dev.h, one function at a time, on the
GPU (tests/devmath/devmath_probe.hip: the product headers unchanged, the product's compiler flags, the tables in LDS).

Whole-record tests (test_gpu_parity.py, test_gpu_chain.py, test_site_stats.py) reach these functions only with the values
a pile-up produces.  Here the inputs are chosen lane by lane: waves that are uniform, waves with one odd lane among 63
(the near-1 polynomial, the `far` form of exp, the full-function fallback, the all-ones divisor of get_Z), random mixes,
the domain edges and counts far beyond any pile-up.  A failure names the function, the case, its wave and lane.

"Bits" below: bytes equal to the oracle's BSM flavour (the bsmath.h twin on the host) always, and to its LIBM flavour
(the host's libm, the reference's own arithmetic) when libm_exact — the rule of test_gpu_parity._check.  NaN results
are compared as NaN (glibc and the device need not agree on a NaN's sign or payload).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "devmath", "libdevmath_probe.so")

pytestmark = pytest.mark.gpu

# function numbers of devmath_probe.hip
LOG_DEV, LOG_MAIN, LOG_NEAR1, BSM_LOG, EXP_DEV, EXP_MID, BSM_EXP, EXP_TERM, NORM_TAIL, DIV_LN10, GET_Z, PURE_LOG, LFACT, SS_LFACT, \
    FISHER, STRAND, SS_POSTERIOR = range(17)

LN10 = 2.30258509299404568402  # the reference's LOG10 macro
U = 2.0 ** -53
TINY = 2.0 ** -1074


def _f(bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _hex(v):
    return float(v).hex()


class Probe:
    def __init__(self, oracle, tables):
        if not os.path.exists(PROBE):
            raise AssertionError("%s is missing: `make devmath-probe` (part of `make all`) builds it" % PROBE)
        self.L = C.CDLL(PROBE)
        self.L.devmath_probe_run.restype = C.c_int
        self.L.devmath_probe_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L.devmath_probe_shape.restype = C.c_int
        self.L.devmath_probe_shape.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        libm = C.CDLL("libm.so.6")  # src/init_param.c:56: logp[] from libm's log, as bscall_api.c builds it
        libm.log.restype = C.c_double
        libm.log.argtypes = [C.c_double]
        self.logp = np.array([libm.log(0.01 * float(i + 1)) for i in range(100)], dtype=np.float64)
        self.lfact = np.ascontiguousarray(tables.lfact_store, dtype=np.float64)
        self.kq = np.ascontiguousarray(tables.q_prob[:, 1], dtype=np.float64)

    def run(self, fn, x):
        k, m = C.c_int(), C.c_int()
        assert self.L.devmath_probe_shape(fn, C.byref(k), C.byref(m)) == 1
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, k.value)
        n = len(x)
        assert fn == SS_POSTERIOR or n % 64 == 0, "cases fill whole waves"
        out = np.empty((n, m.value), dtype=np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = self.L.devmath_probe_run(fn, p(x), p(out), n, p(self.lfact), p(self.logp), p(self.kq))
        assert rc == 0, "devmath_probe_run(%d): hipError_t %d" % (fn, rc)
        return out if m.value > 1 else out[:, 0]


@pytest.fixture(scope="module")
def probe(oracle, tables):
    return Probe(oracle, tables)


def _same_bits(got, want):
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (g.view(np.int64) == w.view(np.int64)) | (np.isnan(g) & np.isnan(w))


def _assert_bits(name, x, got, want):
    ok = _same_bits(got, want)
    if ok.ndim > 1:
        ok = ok.all(axis=1)
    if ok.all():
        return
    bad = np.flatnonzero(~ok)
    xs = np.asarray(x).reshape(len(ok), -1)
    lines = []
    for i in bad[:6]:
        g, w = np.atleast_1d(got[i]), np.atleast_1d(want[i])
        lines.append("case %d (wave %d lane %d) in %s: got %s want %s" % (i, i // 64, i % 64, [_hex(v) for v in xs[i][:6]],
                                                                        [_hex(v) for v in g[:4]], [_hex(v) for v in w[:4]]))
    raise AssertionError("%s: %d of %d cases differ\n  %s" % (name, len(bad), len(ok), "\n  ".join(lines)))


def _check(name, oracle, libm_exact, x, got, ref):
    """ref(flavour) -> the oracle's values; bits against BSM always, against LIBM when libm_exact."""
    _assert_bits(name + " vs bsm", x, got, ref(oracle.BSM))
    if libm_exact:
        _assert_bits(name + " vs libm", x, got, ref(oracle.LIBM))


def _waves(rng, classes, n_uniform=4, n_odd=6, n_mixed=16):
    """Inputs laid out wave by wave from classes {name: values}: every value of every class at least once in waves of its
    own class; for every ordered pair (A, B) of classes, waves of 63 lanes of A and one lane of B (at lane 0, lane 63 and
    random lanes); waves whose lanes pick their class at random."""
    names = sorted(classes)
    pools = {c: np.asarray(classes[c], dtype=np.float64) for c in names}
    out = []
    for c in names:  # every value, in uniform waves (the tail of the pool padded with random picks from it)
        v = pools[c]
        pad = (-len(v)) % 64
        out.append(np.concatenate([v, rng.choice(v, pad)]))
        out.append(rng.choice(v, 64 * n_uniform))
    for a in names:
        for b in names:
            if a == b:
                continue
            for j in range(n_odd):
                w = rng.choice(pools[a], 64)
                w[[0, 63][j] if j < 2 else rng.integers(64)] = rng.choice(pools[b])
                out.append(w)
    for _ in range(n_mixed * len(names)):
        pick = rng.integers(len(names), size=64)
        out.append(np.array([rng.choice(pools[names[p]]) for p in pick]))
    x = np.concatenate(out)
    assert len(x) % 64 == 0
    return x


def _ulp_walk(x0, k):
    """x0 and its k neighbours on either side (same sign)."""
    b = np.float64(x0).view(np.int64)
    return (b + np.arange(-k, k + 1, dtype=np.int64)).view(np.float64)


def _random_bits(rng, n, exp_lo, exp_hi, sign=None):
    """doubles with a uniformly drawn biased exponent in [exp_lo, exp_hi] and a random significand."""
    e = rng.integers(exp_lo, exp_hi + 1, size=n).astype(np.uint64)
    m = rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    s = rng.integers(0, 2, size=n).astype(np.uint64) if sign is None else np.full(n, sign, dtype=np.uint64)
    return ((s << np.uint64(63)) | (e << np.uint64(52)) | m).view(np.float64)


# ---- log ----------------------------------------------------------------------------------------------------------------
NEAR_LO, NEAR_HI = _f([0x3FEE000000000000])[0], _f([0x3FF1090000000000])[0]  # 1 - 2^-4, 1 + 0x1.09p-4: bsm_log_t's near-1 test


def _log_classes(rng):
    table = _random_bits(rng, 60_000, 1, 2046, sign=0)
    table = table[(table < NEAR_LO) | (table >= NEAR_HI)]
    table = np.concatenate([table, [2.0 ** -1022, np.finfo(np.float64).max, 0.5, 2.0, 257.0, 1e300, 1e-300],
                            _ulp_walk(NEAR_LO, 3)[:3], _ulp_walk(NEAR_HI, 3)[3:]])
    near = np.concatenate([rng.uniform(NEAR_LO, NEAR_HI, 30_000), _ulp_walk(NEAR_LO, 3)[3:], _ulp_walk(NEAR_HI, 3)[:3],
                           _ulp_walk(1.0, 3)])
    special = np.concatenate([[0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1e-300, -2.0 ** -1074, 5e-324],
                              _random_bits(rng, 300, 0, 0, sign=0), -_random_bits(rng, 50, 1, 2046, sign=0)])
    return {"table": table, "near": near, "special": special}


def test_log_forms(probe, oracle, libm_exact):
    rng = np.random.default_rng(101)
    cl = _log_classes(rng)
    x = _waves(rng, cl)
    ref = lambda xx: (lambda fl: oracle.log_array(xx, fl))  # noqa: E731
    for fn, name in ((LOG_DEV, "log_dev"), (BSM_LOG, "bsm_log_t")):
        _check(name, oracle, libm_exact, x, probe.run(fn, x), ref(x))
    # the two halves of log_dev on their own domains, in waves of their own
    xt = _waves(rng, {"table": cl["table"]}, n_odd=0)
    _check("log_main", oracle, libm_exact, xt, probe.run(LOG_MAIN, xt), ref(xt))
    xn = _waves(rng, {"near": cl["near"]}, n_odd=0)
    got = probe.run(LOG_NEAR1, xn)
    _check("log_near1", oracle, libm_exact, xn, got, ref(xn))
    assert not np.signbit(got[xn == 1.0]).any(), "log_near1(1) must be +0"


def test_log_dev_boundaries_one_lane_at_a_time(probe, oracle, libm_exact):
    """Each edge value of the near-1 test (0x3fee0000 / 0x3ff10900 +- 1-3 ulp, 1 +- 3 ulp) and each special at every lane of a
    wave whose other 63 lanes take the table path, and of one whose other lanes take the near-1 polynomial."""
    rng = np.random.default_rng(102)
    edges = np.concatenate([_ulp_walk(NEAR_LO, 3), _ulp_walk(NEAR_HI, 3), _ulp_walk(1.0, 3), [0.0, -0.0, 5e-324, np.inf, np.nan, -1.0]])
    waves = []
    for bg in (rng.uniform(2.0, 3.0, 64), rng.uniform(0.95, 1.05, 64)):
        for v in edges:
            for lane in range(64):
                w = bg.copy()
                w[lane] = v
                waves.append(w)
    x = np.concatenate(waves)
    _check("log_dev", oracle, libm_exact, x, probe.run(LOG_DEV, x), lambda fl: oracle.log_array(x, fl))


# ---- exp ----------------------------------------------------------------------------------------------------------------
EXP_OVF = 709.782712893383973096  # largest x with a finite exp(x)
EXP_NORM = -708.3964185322641  # about where exp(x) leaves the normal range
EXP_UNF = -745.1332191019411  # about where exp(x) rounds to 0


def _exp_classes(rng):
    tiny = np.concatenate([[0.0, -0.0, 2.0 ** -55, -(2.0 ** -55)], _random_bits(rng, 2000, 0, 0x3C8)])
    mid = np.concatenate([_random_bits(rng, 30_000, 0x3C9, 0x407), rng.uniform(-512, 512, 20_000), [0.0],
                          _ulp_walk(2.0 ** -54, 2)[2:], -_ulp_walk(2.0 ** -54, 2)[2:], _ulp_walk(512.0, 3)[:3], -_ulp_walk(512.0, 3)[:3]])
    big = np.concatenate([rng.uniform(512, 1024, 5000), rng.uniform(-1024, -512, 5000), [512.0, -512.0],
                          _ulp_walk(EXP_OVF, 3), _ulp_walk(EXP_NORM, 3), _ulp_walk(EXP_UNF, 3), -_ulp_walk(1024.0, 2)[:2],
                          _ulp_walk(1024.0, 2)[:2], rng.uniform(-746, -700, 3000), rng.uniform(700, 710, 1000)])
    special = np.array([np.inf, -np.inf, np.nan, 1024.0, -1024.0, 1e308, -1e308, 1e4, -1e4, 2000.0])
    return {"tiny": tiny, "mid": mid, "big": big, "special": special}


def test_exp_forms(probe, oracle, libm_exact):
    rng = np.random.default_rng(201)
    cl = _exp_classes(rng)
    x = _waves(rng, cl)
    for fn, name in ((EXP_DEV, "exp_dev"), (BSM_EXP, "bsm_exp_t")):
        _check(name, oracle, libm_exact, x, probe.run(fn, x), lambda fl: oracle.exp_array(x, fl))
    xm = _waves(rng, {"mid": cl["mid"]}, n_odd=0)
    _check("exp_mid", oracle, libm_exact, xm, probe.run(EXP_MID, xm), lambda fl: oracle.exp_array(xm, fl))


# ---- exp_term_dev and the normalising tail ------------------------------------------------------------------------------
def _term_classes(rng):
    near = np.concatenate([rng.uniform(-512, 0, 20_000), rng.uniform(-40, 0, 5000), [0.0, -0.0, -(2.0 ** -60), -(2.0 ** -54)],
                           -_ulp_walk(512.0, 3)[:3]])
    far = np.concatenate([rng.uniform(-700, -512, 30_000), rng.uniform(-709, -500, 10_000).clip(-700, -512), [-512.0, -700.0],
                          -_ulp_walk(512.0, 3)[3:], -_ulp_walk(700.0, 3)[:4]])
    clamped = np.concatenate([rng.uniform(-800, -700, 20_000), rng.uniform(-709, -700, 10_000), -_ulp_walk(700.0, 3)[4:],
                              [EXP_NORM, EXP_UNF, -745.2, -800.0]])
    return {"near": near, "far": far, "clamped": clamped}


def test_exp_term_dev(probe, oracle, libm_exact):
    """exp(max(x, -700)) for x <= 0 (the clamp is part of the function's contract: callmath.h's proof that it cannot change
    the normalising sum is tested by test_normalising_tail)."""
    rng = np.random.default_rng(301)
    x = _waves(rng, _term_classes(rng))
    assert (x <= 0).all()
    _check("exp_term_dev", oracle, libm_exact, x, probe.run(EXP_TERM, x), lambda fl: oracle.exp_array(np.maximum(x, -700.0), fl))


def test_exp_term_dev_outside_its_domain(probe, oracle):
    """What exp_term_dev returns where no call site can reach it — its one caller, call_body.inc, passes ll[g] - max with max
    the largest of ten finite ll[g] (so x <= 0, finite; test_devmath_build.py pins the call sites):
      NaN, -inf  -> exp(-700): v_max_f64 returns the number when one operand is NaN, and -700 beats -inf;
      0 < x < 512 -> exp(x), the main path;
    512 <= x is not asserted (the main path without glibc's overflow handling)."""
    rng = np.random.default_rng(302)
    pos = np.concatenate([[2.0 ** -60, 1.0, 511.0], rng.uniform(0, 512, 63 * 40)])
    spec = np.array([np.nan, -np.inf])
    x = np.concatenate([pos[: 64 * (len(pos) // 64)], np.resize(spec, 64), rng.permutation(np.concatenate([pos[:62], spec]))])
    got = probe.run(EXP_TERM, x)
    want = oracle.exp_array(np.where(np.isnan(x) | (x == -np.inf), -700.0, x), oracle.BSM)
    _assert_bits("exp_term_dev outside x <= 0", x, got, want)


def _tail_inputs(rng, n):
    """n vectors of ten ll[g] - max: one exact 0 at a random index, the others mostly from [-760, -480] (terms in the far
    form, clamped at -700, subnormal or zero in libm), some from [-40, 0] and [-480, -40]."""
    v = rng.uniform(-760, -480, (n, 10))
    r = rng.random((n, 10))
    v[r < 0.15] = rng.uniform(-40, 0, (n, 10))[r < 0.15]
    v[(r >= 0.15) & (r < 0.25)] = rng.uniform(-480, -40, (n, 10))[(r >= 0.15) & (r < 0.25)]
    v[r > 0.97] = np.array([-700.0, -512.0, -745.2, -1e-300, -709.0, -708.5])[rng.integers(0, 6, (n, 10))][r > 0.97]
    v[np.arange(n), rng.integers(0, 10, n)] = 0.0
    return v


def test_normalising_tail(probe, oracle, libm_exact):
    """gt_prob[g] = (x_g - log(sum_g exp(x_g))) / LOG10 as call_body.inc composes it (exp_term_dev, index-order sum, log_dev,
    div_ln10_dev) against the reference's arithmetic in numpy float64 (src/genotype_model.c:240-245): every term through
    libm's exp unclamped, the sum in index order, libm's log, IEEE division.  Bit equality here is callmath.h's proof that
    the -700 clamp cannot change the sum."""
    rng = np.random.default_rng(401)
    x = _tail_inputs(rng, 64 * 2000)

    def ref(fl):
        e = oracle.exp_array(x, fl).reshape(x.shape)
        s = np.zeros(len(x))
        for g in range(10):
            s = s + e[:, g]
        ls = oracle.log_array(s, fl)
        return (x - ls[:, None]) / LN10

    got = probe.run(NORM_TAIL, x)
    _check("normalising tail", oracle, libm_exact, x, got, ref)


# ---- x / ln 10 ----------------------------------------------------------------------------------------------------------
def test_div_ln10_dev(probe):
    rng = np.random.default_rng(501)
    every_exp = np.concatenate([_random_bits(rng, 2046 * 16, 1, 2046)] + [_random_bits(rng, 8, e, e) for e in range(1, 2047)])
    tiny = np.concatenate([_random_bits(rng, 4000, 1, 22), _random_bits(rng, 2000, 0, 0), [2.0 ** -1000, -(2.0 ** -1000)],
                           _ulp_walk(2.0 ** -1000, 2)[:2], -_ulp_walk(2.0 ** -1000, 2)[:2], [5e-324, -5e-324]])
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float64).max, -np.finfo(np.float64).max])
    x = _waves(rng, {"normal": every_exp, "tiny": tiny, "special": special})
    _assert_bits("div_ln10_dev", x, probe.run(DIV_LN10, x), x / LN10)


# ---- get_Z and the tabulated logs ---------------------------------------------------------------------------------------
def _model_params(rng, n):
    """(l, t) over the range bsc_create accepts, drawn as test_pure_logs.py draws them."""
    under = rng.choice([0.0, 1e-9, 0.01, 0.3, 0.999999], size=n) * rng.random(n) ** rng.integers(0, 3, size=n)
    over = rng.random(n) * (1.0 - under - 2.0 ** -20)
    over[rng.random(n) < 0.1] = 0.0
    return 1.0 - under, over


def _counts(rng, n):
    c = np.floor(2.0 ** (33 * rng.random(n)))
    c[rng.random(n) < 0.2] = 0.0
    small = rng.random(n) < 0.1
    c[small] = rng.integers(1, 40, n)[small]
    return c


def _allones(d):
    b = np.asarray(d, dtype=np.float64).view(np.uint64)
    return (b & np.uint64((1 << 52) - 1)) == np.uint64((1 << 52) - 1)


def test_get_Z(probe, oracle, libm_exact):
    rng = np.random.default_rng(601)
    n = 64 * 3000
    l, t = _model_params(rng, n)
    x1, x2 = _counts(rng, n), _counts(rng, n)
    both0 = (x1 + x2) == 0
    x1[both0] = 1.0
    k1, k2 = 0.5 * rng.random(n), 0.5 * rng.random(n)
    k1[rng.random(n) < 0.05] = 0.5
    ordinary = np.stack([x1, x2, k1, k2, l, t], axis=1)
    # all-ones divisors built on purpose: l - t = 1 - 2^-53 and x1 + x2 a power of two
    m = 64 * 800
    p2 = 2.0 ** rng.integers(0, 34, m)
    a1 = np.floor(p2 * rng.random(m))
    a1[rng.random(m) < 0.1] = 0.0
    ones = np.stack([a1, p2 - a1, 0.5 * rng.random(m), 0.5 * rng.random(m), np.ones(m), np.full(m, 2.0 ** -53)], axis=1)
    assert _allones((ones[:, 0] + ones[:, 1]) * (ones[:, 4] - ones[:, 5])).all()
    x = np.concatenate([ordinary[: 64 * 1000], ones[: 64 * 200]])  # uniform waves of each kind
    mixed = ordinary[64 * 1000 :].copy()  # then waves of ordinary lanes with 1, 2 or many all-ones lanes among them
    for w in range(len(mixed) // 64):
        k = [1, 1, 2, 8, 32][w % 5]
        lanes = rng.choice(64, k, replace=False)
        mixed[64 * w + lanes] = ones[rng.integers(64 * 200, m, k)]
    x = np.concatenate([x, mixed, ones[64 * 200 :]])
    got = probe.run(GET_Z, x)
    _check("get_Z", oracle, libm_exact, x, got, lambda fl: oracle.get_Z_array(x, fl))


PT_Q = 44


def test_pure_log_entry(probe, oracle, libm_exact, tables):
    """callmath.h's tabulated logs (all 5 x 44 entries, over many (l, t)) equal log() of the argument the per-site path
    forms: get_Z of a pair with one class empty, then call_body.inc's / the reference's expression for that class."""
    rng = np.random.default_rng(701)
    n_par = 16 * 40
    l, t = _model_params(rng, n_par)
    idx = np.tile(np.arange(5 * PT_Q), n_par)
    L, T = np.repeat(l, 5 * PT_Q), np.repeat(t, 5 * PT_Q)
    x = np.stack([idx.astype(np.float64), L, T], axis=1)
    got = probe.run(PURE_LOG, x)
    kq = tables.q_prob[:, 1]
    ide, q = idx // PT_Q, idx % PT_Q
    k = kq[q]
    cnt = np.floor(2.0 ** (33 * rng.random(len(idx)))) + 1.0
    kz = 0.5 * rng.random(len(idx))
    zero = np.zeros(len(idx))
    # the pair's first class empty (x1 = 0): Zc; its second (x2 = 0): Zd.  All three quotients are clamped alike.
    zc = oracle.get_Z_array(np.stack([zero, cnt, kz, k, L, T], axis=1), oracle.BSM)
    zd = oracle.get_Z_array(np.stack([cnt, zero, k, kz, L, T], axis=1), oracle.BSM)
    assert (zc[:, 0] == zc[:, 1]).all() and (zc[:, 0] == zc[:, 2]).all() and (zd[:, 0] == zd[:, 1]).all() and (zd[:, 0] == zd[:, 2]).all()
    arg = np.select(
        [ide == 0, ide == 1, ide == 2, ide == 3, ide == 4],
        [1.0 - zc[:, 0] + k,  # class 7: CC (1.0 - Z[0] + k)      class 4: GG (1.0 - Z[3] + k)
         1.0 - 0.5 * zc[:, 1] + k,  # class 7: CT                 class 4: AG
         0.5 * (1.0 - zc[:, 2]) + k,  # class 7: AC, CG            class 4: CG, GT
         zd[:, 0] + k,  # class 5: CC (Z[0] + k)                  class 6: GG (Z[3] + k)
         0.5 * zd[:, 2] + k])  # class 5: CT, AC, CG               class 6: AG, CG, GT
    _check("pure_log_entry", oracle, libm_exact, x, got, lambda fl: oracle.log_array(arg, fl))
    # and log_dev of the same arguments: what the per-site path computes
    ya = probe.run(LOG_DEV, arg)
    _assert_bits("pure_log_entry vs log_dev", x, got, ya)


# ---- lfact2, Fisher, the strand table -----------------------------------------------------------------------------------
def test_lfact(probe, oracle, libm_exact, tables):
    rng = np.random.default_rng(801)
    every = np.arange(0, 2 ** 20 + 1, dtype=np.int64)
    big = rng.integers(2 ** 20, 2 ** 31 - 1, 1_000_000)  # up to 2^31 - 2: n + 1 stays an int
    big[:6] = [2 ** 31 - 2, 2 ** 31 - 3, 2 ** 30, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1]
    n = np.concatenate([every, big])
    n = np.concatenate([n, n[: (-len(n)) % 64]])
    for fn, name in ((LFACT, "lfact_dev"), (SS_LFACT, "ss_lfact")):
        got = probe.run(fn, n.astype(np.float64))
        _check(name, oracle, libm_exact, n, got, lambda fl: oracle.lfact_array(n, tables, fl))


NMAX = 46_340  # the largest n whose products row * col and (c - i) * (c' - i) fit the reference's int; beyond it both the
# reference's fisher() and fisher_dev overflow int (undefined behaviour in C), which is out of scope here


def _fisher_tables(rng):
    out = []
    out.append(rng.integers(0, 12, (64 * 300, 4)))  # small: every branch, zero rows and columns
    out.append(rng.integers(0, 200, (64 * 300, 4)))
    z = rng.integers(0, 60, (64 * 100, 4))  # zero rows / columns on purpose
    which = rng.integers(0, 4, len(z))
    z[which == 0, 0:2] = 0
    z[which == 1, 2:4] = 0
    z[which == 2, 0::2] = 0
    z[which == 3, 1::2] = 0
    out.append(z)
    # delta == 0 (c0 n == row0 col0): proportional tables
    a, b, s = rng.integers(0, 40, 64 * 50), rng.integers(0, 40, 64 * 50), rng.integers(1, 30, 64 * 50)
    out.append(np.stack([a * s, b * s, a, b], axis=1))
    # 2 delta on either side of an integer, or on it: searched among random tables
    c = rng.integers(0, 400, (400_000, 4))
    r0, r1, k0 = c[:, 0] + c[:, 1], c[:, 2] + c[:, 3], c[:, 0] + c[:, 2]
    nn = r0 + r1
    rem = np.where(nn > 0, (2 * (c[:, 0] * nn - r0 * k0)) % np.maximum(nn, 1), -1)
    sel = c[(nn > 0) & ((rem == 0) | (rem == 1) | (rem == nn - 1))]
    out.append(sel[: 64 * (min(len(sel), 64 * 200) // 64)])
    # large: n up to NMAX, balanced and skewed
    big = []
    for _ in range(64 * 40):
        nt = int(rng.integers(1000, NMAX + 1))
        p = rng.dirichlet(rng.uniform(0.2, 3.0, 4))
        v = np.floor(p * nt).astype(np.int64)
        big.append(v)
    big = np.array(big)
    big[:4] = [[NMAX // 4, NMAX // 4, NMAX // 4, NMAX // 4], [NMAX // 2, 0, 0, NMAX // 2], [0, NMAX // 2, NMAX // 2, 0], [NMAX, 0, 0, 0]]
    out.append(big)
    tabs = np.concatenate(out).astype(np.int64)
    assert (tabs.sum(axis=1) <= NMAX).all() and (tabs >= 0).all()
    return tabs


def test_fisher_dev(probe, oracle, libm_exact, tables):
    rng = np.random.default_rng(901)
    c = _fisher_tables(rng)
    c = c[rng.permutation(len(c))]  # mixed waves: loop trips and branches differ lane by lane
    c = np.concatenate([c, c[: (-len(c)) % 64]])
    got = probe.run(FISHER, c.astype(np.float64))
    _check("fisher_dev", oracle, libm_exact, c, got, lambda fl: oracle.fisher_array(c, tables, fl))
    # the edges the sample was built to contain
    r0, k0, n = c[:, 0] + c[:, 1], c[:, 0] + c[:, 2], c.sum(axis=1)
    delta = c[:, 0] - (r0 * k0) / np.maximum(n, 1)
    assert (n == 0).any() and ((delta == 0) & (n > 0)).any() and (n == NMAX).any()
    two = 2 * delta
    assert ((two != np.round(two)) & (np.abs(two - np.round(two)) < 0.01)).any()


def _strand_ref(mxi, f, r):
    """src/call_genotypes.c:64-100 (including :98, where the GT row's reverse count takes the FORWARD class-6 count)."""
    if mxi == 1:
        return f[0] + f[4], f[1] + f[5] + f[7], r[0] + r[4], r[1] + r[5] + r[7]
    if mxi == 2:
        return f[0], f[2] + f[6], r[0], r[2] + r[6]
    if mxi == 3:
        return f[0] + f[4], f[3] + f[7], r[0] + r[4], r[3] + r[7]
    if mxi == 5:
        return f[1] + f[5] + f[7], f[2] + f[4] + f[6], r[1] + r[5] + r[7], r[2] + r[4] + r[6]
    if mxi == 6:
        return f[1] + f[5], f[3], r[1] + r[5], r[3]
    if mxi == 8:
        return f[2] + f[4] + f[6], f[3] + f[7], r[2] + r[4] + f[6], r[3] + r[7]
    return 0, 0, 0, 0  # homozygous calls: no table (the caller never asks)


def test_strand_table(probe):
    rng = np.random.default_rng(1001)
    n = 64 * 200
    mxi = rng.integers(0, 9, n)
    mxi[: 9 * 64] = np.repeat(np.arange(9), 64)  # a uniform wave of each genotype, then mixed ones
    fr = rng.integers(0, 1 << 28, (n, 16))
    fr[rng.random((n, 16)) < 0.3] = 0
    x = np.concatenate([mxi[:, None], fr], axis=1).astype(np.float64)
    got = probe.run(STRAND, x)
    want = np.array([_strand_ref(int(m), [int(v) for v in row[:8]], [int(v) for v in row[8:]]) for m, row in zip(mxi, fr)], dtype=np.float64)
    _assert_bits("strand_table", x, got, want)


# ---- the methylation posterior ------------------------------------------------------------------------------------------
# ss_posterior sums its 128 lanes' values (101 bins, the rest 0) with v0 + v1 and six shuffle levels: every term passes
# through 7 additions of non-negative numbers, so the device sum is within gamma_7 = 7u / (1 - 7u) of the exact sum, and a
# bin z = RN(v / sum) within gamma_7 + u (+ u^2 terms) of v / sum, relatively.  The reference adds the 101 terms in index
# order (meth[0] or meth[100] first, then 1..99: src/print_vcf.c:492-505): within gamma_100 + u.  Bins that underflow
# carry an absolute slack of two subnormal steps.
BOUND_FSUM = 11 * U  # device vs RN(v / fsum(v)): gamma_7 + u + 2u for the comparison value's own two roundings, + slack
BOUND_REF = 110 * U  # device vs the reference's sequential order: gamma_7 + u + gamma_100 + u, + slack


def _posterior_ref(oracle, tables, logp, a, b, fl):
    """terms and bins of src/print_vcf.c:492-505 for pairs (a[i], b[i]), vectorised over the pairs: every operation is the
    reference's, in its order (numpy float64, no contraction)."""
    konst = oracle.lfact_array(a + b + 1, tables, fl) - oracle.lfact_array(a, tables, fl) - oracle.lfact_array(b, tables, fl)
    da, db = a.astype(np.float64), b.astype(np.float64)
    args = np.empty((len(a), 101))
    args[:, 0] = konst
    args[:, 100] = konst
    for i in range(1, 100):
        args[:, i] = konst + logp[i - 1] * da + logp[99 - i] * db
    v = oracle.exp_array(args, fl).reshape(len(a), 101)
    v[a != 0, 0] = 0.0
    v[b != 0, 100] = 0.0
    s = np.where(a == 0, v[:, 0], v[:, 100])  # `sum = meth[0] = ...` / `sum = (meth[100] = ...)`: one of the two, or 0
    s = np.where((a != 0) & (b != 0), 0.0, s)
    for i in range(1, 100):
        s = s + v[:, i]
    return v, v / s[:, None]


def test_ss_posterior(probe, oracle, tables):
    rng = np.random.default_rng(1101)
    a0, b0 = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    a, b = a0.ravel(), b0.ravel()
    keep = (a + b) > 0  # the caller evaluates a posterior only when a + b != 0
    a, b = a[keep], b[keep]
    m = 2000
    tot = rng.integers(64, 5001, m)
    fa = rng.integers(0, tot + 1)
    fa[: m // 10] = 0  # a = 0
    fa[m // 10 : m // 5] = tot[m // 10 : m // 5]  # b = 0
    fa[m // 5 : m // 5 + 3] = [5000, 0, 2500]
    tot[m // 5 : m // 5 + 3] = 5000
    a = np.concatenate([a, fa]).astype(np.int64)
    b = np.concatenate([b, tot - fa]).astype(np.int64)
    assert (a + b <= 5000).all() and ((a + b) >= 256).any()
    got = probe.run(SS_POSTERIOR, np.stack([a, b], axis=1).astype(np.float64))
    logp = probe.logp
    v, zref = _posterior_ref(oracle, tables, logp, a, b, oracle.BSM)  # the device's terms are these bits (test_exp_forms)
    # exact zeros where the reference has them, nothing else zero that the reference has as a normal number
    zero = v == 0
    assert (got[zero] == 0).all(), "a bin the reference sets to 0 is not 0"
    # device sum vs the correctly rounded sum of its own terms
    fs = np.array([math.fsum(row) for row in v])
    zf = v / fs[:, None]
    err = np.abs(got - zf)
    lim = BOUND_FSUM * zf + 2 * TINY
    bad = np.argwhere(err > lim)
    assert len(bad) == 0, "bins off the fsum bound: %s" % [(int(a[i]), int(b[i]), int(j), _hex(got[i, j]), _hex(zf[i, j])) for i, j in bad[:5]]
    err = np.abs(got - zref)
    lim = BOUND_REF * zref + 2 * TINY
    bad = np.argwhere(err > lim)
    assert len(bad) == 0, "bins off the sequential-order bound: %s" % [(int(a[i]), int(b[i]), int(j)) for i, j in bad[:5]]
    # the sample reaches bins that underflow and the lgamma branch
    assert ((v > 0) & (v < 2.0 ** -1022)).any() and (v[:, 1:100] == 0).any()


# ---- sweeps: the polynomials on tens of millions of arguments -----------------------------------------------------------
# A polynomial step computed unfused instead of fused (or the reverse) changes log near 1 or exp in about one argument in
# two million, too rarely for the edge sets above; these sweeps are what catch it.
SWEEP = 1 << 23


@pytest.mark.parametrize("fn,name,lo,hi,chunks", [
    (LOG_DEV, "log_dev near 1", float(NEAR_LO), float(NEAR_HI), 4),
    (LOG_DEV, "log_dev table path", 1.0625, 40.0, 2),
    (EXP_DEV, "exp_dev", -512.0, 512.0, 4),
    (EXP_TERM, "exp_term_dev", -700.0, 0.0, 4),
])
def test_sweep(probe, oracle, libm_exact, fn, name, lo, hi, chunks):
    rng = np.random.default_rng(1201 + fn)
    ref = oracle.log_array if fn == LOG_DEV else oracle.exp_array
    for _ in range(chunks):
        x = rng.uniform(lo, hi, SWEEP)
        _check(name, oracle, libm_exact, x, probe.run(fn, x), lambda fl: ref(x, fl))


def test_device_at_the_correctly_rounded_points(probe, tables):
    """The device forms at the edge points of tests/golden/devmath_hp.json (mpmath): within the bound test_devmath_hp.py
    measures for the host flavour (1 ulp)."""
    import json

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "devmath_hp.json")))
    for key, fns in (("log", (LOG_DEV, BSM_LOG)), ("exp", (EXP_DEV, BSM_EXP)), ("lgamma_n1", (LFACT, SS_LFACT))):
        x = np.array([float(a) if key == "lgamma_n1" else float.fromhex(a) for a, _ in g[key]])
        want = np.array([float.fromhex(b) for _, b in g[key]])
        pad = (-len(x)) % 64
        xp = np.concatenate([x, x[:pad]])
        for fn in fns:
            got = probe.run(fn, xp)[: len(x)]
            u = np.abs(got.view(np.int64) - want.view(np.int64))
            assert u.max() <= 1, (key, fn, x[np.argmax(u)], _hex(got[np.argmax(u)]), _hex(want[np.argmax(u)]))
