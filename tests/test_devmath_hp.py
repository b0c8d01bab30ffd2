"""The host side of the device-math chain against correctly rounded values (tests/golden/devmath_hp.json, written by
tools/make_devmath_hp.py with mpmath at 256 bits): log, exp and lgamma(n + 1) at the edge points of the device forms.
test_gpu_devmath.py holds the device to the BSM flavour bit for bit; this pins the BSM flavour itself to the true values,
so the GPU test needs nothing beyond numpy.  CPU only.

Bounds, in units in the last place of the correctly rounded result:
  log   documented: < 0.52 ulp (the Arm Optimized Routines algorithm glibc >= 2.28 ships)  -> at most 1 ulp apart
        measured on these 274 points: 0 (every point correctly rounded)
  exp   documented: < 0.52 ulp (same source)                                              -> at most 1 ulp apart
        measured on these 267 points: 0
  lgamma(n + 1), n >= 256 (lfact2's non-table branch): glibc's x86_64 ulps table allows 4 ulp for double lgamma
        measured on these 146 points: 1 (49 of them 1 ulp off)
The asserted bound is the measured one: all three within 1 ulp."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "devmath_hp.json")
BOUND = {"log": 1, "exp": 1, "lgamma_n1": 1}


def _load():
    d = json.load(open(GOLDEN))
    return {k: (np.array([a if k == "lgamma_n1" else float.fromhex(a) for a, _ in d[k]]), np.array([float.fromhex(b) for _, b in d[k]]))
            for k in BOUND}


def _ulps(a, b):
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


def test_golden_covers_the_edges():
    g = _load()
    lx = g["log"][0]
    assert (lx == float(np.uint64(0x3FEE000000000000).view(np.float64))).any() and (lx == float(np.uint64(0x3FF1090000000000).view(np.float64))).any()
    assert (lx < 2.0 ** -1022).any()
    ex = g["exp"][0]
    assert (ex == -700.0).any() and (ex == -512.0).any() and (ex == 2.0 ** -54).any() and (g["exp"][1] < 2.0 ** -1022).any()
    assert g["lgamma_n1"][0].min() == 256 and g["lgamma_n1"][0].max() == 2 ** 31 - 2


def test_bsm_flavour_within_the_bound(oracle, tables, libm_exact):
    g = _load()
    got = {"log": oracle.log_array(g["log"][0], oracle.BSM), "exp": oracle.exp_array(g["exp"][0], oracle.BSM),
           "lgamma_n1": oracle.lfact_array(g["lgamma_n1"][0], tables, oracle.BSM)}
    for k, b in BOUND.items():
        u = _ulps(got[k], g[k][1])
        assert u.max() <= b, (k, int(u.max()), g[k][0][np.argmax(u)])
    if libm_exact:  # the host's libm is what the reference runs on: the same values
        assert _ulps(oracle.log_array(g["log"][0], oracle.LIBM), got["log"]).max() == 0
        assert _ulps(oracle.lfact_array(g["lgamma_n1"][0], tables, oracle.LIBM), got["lgamma_n1"]).max() == 0
