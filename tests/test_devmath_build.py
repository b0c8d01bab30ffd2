"""The device-math probe (tests/devmath/devmath_probe.hip, run by tests/test_gpu_devmath.py) builds for gfx950 from the
product headers with the product's flags, and its host entry points reject what they must; the call sites that
test_gpu_devmath.py relies on for the domain of exp_term_dev are the ones it names.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bs_call_amd", "csrc")


def _make(*args):
    return subprocess.run(["make", "-C", ROOT, "--no-print-directory"] + list(args), check=True, capture_output=True, text=True).stdout


def test_probe_cross_compiles_for_gfx950_with_the_product_flags(tmp_path):
    so = str(tmp_path / "libdevmath_probe.so")
    cmd = _make("-n", "-B", "devmath-probe", "DEVMATH_SO=" + so)
    hipflags = re.search(r"^HIPFLAGS = (.*)$", open(os.path.join(ROOT, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950")
    assert hipflags in cmd and "-ffp-contract=off" in hipflags, cmd
    _make("-B", "devmath-probe", "DEVMATH_SO=" + so)
    blob = open(so, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob, "no gfx950 code object in the probe"
    for fn in range(17):
        assert ("_Z9dm_kernelILi%dEE" % fn).encode() in blob, fn
    L = C.CDLL(so)
    k, m = C.c_int(), C.c_int()
    shapes = []
    for fn in range(17):
        assert L.devmath_probe_shape(fn, C.byref(k), C.byref(m)) == 1
        shapes.append((k.value, m.value))
    assert shapes[8] == (10, 10) and shapes[10] == (6, 3) and shapes[15] == (17, 4) and shapes[16] == (2, 101)
    assert L.devmath_probe_shape(17, C.byref(k), C.byref(m)) == 0 and L.devmath_probe_shape(-1, C.byref(k), C.byref(m)) == 0
    # rejected before any device call: an unknown function, a partial wave, missing tables (hipErrorInvalidValue = 1)
    L.devmath_probe_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    x, y, t = np.zeros(65), np.zeros(65), np.zeros(256)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.devmath_probe_run(17, p(x), p(y), 64, p(t), p(t), p(t)) == 1
    assert L.devmath_probe_run(0, p(x), p(y), 65, p(t), p(t), p(t)) == 1
    assert L.devmath_probe_run(0, p(x), p(y), 64, None, p(t), p(t)) == 1


def test_probe_is_not_part_of_the_product_library():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    link = re.search(r"^\$\(LIBDIR\)/libbscall_amd\.so: (.*)$", mk, re.M).group(1)
    assert "devmath" not in link
    assert re.search(r"^all: .*devmath-probe", mk, re.M), "build() (make all) must build the probe"


def test_exp_term_dev_call_sites_pass_differences_to_the_maximum():
    """test_gpu_devmath.test_exp_term_dev_outside_its_domain documents what exp_term_dev returns for x > 0, NaN and -inf; this
    pins that its only callers pass ll[g] - max (<= 0, finite): the two forms of the normalisation in call_body.inc, whose
    ten values are formed by `ll_g -= mx` after the first-max argmax.  A new call site fails here until it is reviewed."""
    calls = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".inc", ".hip", ".c")):
            for line in open(os.path.join(CSRC, f)):
                for a in re.findall(r"exp_term_dev\((.*?), \(const uint64_t \*\)s_exptab\)", line):
                    calls.append((f, a))
    assert sorted(calls) == [("call_body.inc", "act ? xs[e] : 0.0"), ("call_body.inc", "la[g]"), ("call_body.inc", "la[g]")], calls
    body = open(os.path.join(CSRC, "call_body.inc")).read()
    assert "ll0 -= mx; ll1 -= mx; ll2 -= mx; ll3 -= mx; ll4 -= mx; ll5 -= mx; ll6 -= mx; ll7 -= mx; ll8 -= mx; ll9 -= mx;" in body
    # xs[] / la[] hold exactly those ten differences when the exp loops read them
    assert "lg[0] = ll0; lg[1] = ll1;" in body and "la[0] = ll0; la[1] = ll1;" in body
