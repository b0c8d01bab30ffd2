"""Writes tests/golden/devmath_hp.json: correctly rounded log(x), exp(x) and lgamma(n + 1) at the edge points of the device
math forms (csrc/callmath.h, csrc/bsmath.h), evaluated with mpmath at 256 bits and rounded once to double (subnormal
results to a multiple of 2^-1074).  Values are stored as float.hex strings.  tests/test_devmath_hp.py checks the bsmath.h
flavour of the oracle against them on the CPU; tests/test_gpu_devmath.py checks the device.

    python tools/make_devmath_hp.py            # rewrites the file (deterministic: fixed seed)
"""
import json
import math
import os

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "devmath_hp.json")


def _walk(x0, k):
    b = np.float64(x0).view(np.int64)
    return [float(v) for v in (b + np.arange(-k, k + 1, dtype=np.int64)).view(np.float64)]


def _cr(v):
    """v (an mpf at high precision) rounded to the nearest double, ties to even, subnormals included; None past DBL_MAX."""
    if v == 0:
        return 0.0
    if abs(v) < mpmath.mpf(2) ** -1022:
        q = int(mpmath.nint(v * mpmath.mpf(2) ** 1074))  # nint: round half to even
        return math.ldexp(float(q), -1074)
    with mpmath.workprec(53):
        r = +v
    f = float(r)
    return None if math.isinf(f) else f


def log_points(rng):
    near_lo, near_hi = float(np.uint64(0x3FEE000000000000).view(np.float64)), float(np.uint64(0x3FF1090000000000).view(np.float64))
    xs = _walk(near_lo, 3) + _walk(near_hi, 3) + _walk(1.0, 3)[:3] + _walk(1.0, 3)[4:] + _walk(2.0, 1) + _walk(0.5, 1)
    xs += [2.0 ** -1022, 2.0 ** -1074, 1e-310, float(np.finfo(np.float64).max), 1e300, 1e-300, 257.0, 4096.0 + 1.0]
    xs += [float(v) for v in rng.uniform(near_lo, near_hi, 120)]
    xs += [float(v) for v in np.exp(rng.uniform(-700, 700, 120))]
    return xs


def exp_points(rng):
    ovf = 709.782712893383973096
    xs = _walk(2.0 ** -54, 2) + [-v for v in _walk(2.0 ** -54, 2)] + _walk(512.0, 2) + [-v for v in _walk(512.0, 2)]
    xs += [-v for v in _walk(700.0, 2)] + _walk(ovf, 2)[:3] + _walk(-708.3964185322641, 2) + _walk(-745.1332191019411, 2)
    xs += [1.0, -1.0, 0.5, -0.5, 1e-10, -1e-10, 100.0, -100.0, -1000.0 + 255.0]
    xs += [float(v) for v in rng.uniform(-512, 512, 120)]
    xs += [float(v) for v in rng.uniform(-745, -512, 80)]
    xs += [float(v) for v in rng.uniform(512, 709.78, 20)]
    return xs


def lgamma_points(rng):
    ns = list(range(256, 270)) + [511, 512, 1000, 4096, 46340, 2 ** 20, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 30, 2 ** 31 - 3, 2 ** 31 - 2]
    ns += [int(v) for v in rng.integers(256, 2 ** 20, 60)] + [int(v) for v in rng.integers(2 ** 20, 2 ** 31 - 1, 60)]
    return ns


def main():
    rng = np.random.default_rng(20261016)
    mpmath.mp.prec = 256
    out = {"about": "correctly rounded values (mpmath, 256 bits) for tests/test_devmath_hp.py; tools/make_devmath_hp.py writes this file",
           "log": [], "exp": [], "lgamma_n1": []}
    for x in log_points(rng):
        y = _cr(mpmath.log(mpmath.mpf(x)))
        out["log"].append([x.hex(), y.hex()])
    for x in exp_points(rng):
        y = _cr(mpmath.exp(mpmath.mpf(x)))
        if y is not None:
            out["exp"].append([x.hex(), y.hex()])
    for n in lgamma_points(rng):
        y = _cr(mpmath.loggamma(mpmath.mpf(n + 1)))
        out["lgamma_n1"].append([n, y.hex()])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote %s: %d log, %d exp, %d lgamma points" % (OUT, len(out["log"]), len(out["exp"]), len(out["lgamma_n1"])))


if __name__ == "__main__":
    main()
