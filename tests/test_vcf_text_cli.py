"""bam2bcf --format on the CPU (what it refuses is refused before a context is created) and the host number formatter bsc_fmt_g,
the checker of the device's "%g" (csrc/fmtg_dev.h)."""
import os
import subprocess

import numpy as np
import pytest

from bs_call_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")
TIES = [100000.5, 100001.5, 1000005.0, 1000015.0, 999999.5, 999999.4375, 0.0001, 0.00001, 1e6, 999999.0, 123456.5, 123457.5, 0.5, 1.5, 2.5,
        0.0, -0.0, np.inf, -np.inf]


def _run(tmp_path, *args, env=None):
    assert os.path.exists(EXE), "run `make demo`"
    out = str(tmp_path / "out.vcf")
    r = subprocess.run([EXE, *args, str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), out, str(tmp_path / "rep.json")], capture_output=True,
                       text=True, timeout=60, env=dict(os.environ, **(env or {})))
    return r, out


def _refused(tmp_path, r, out):
    assert r.returncode == 2, r.stderr + r.stdout
    assert "--format" in r.stderr
    assert not os.path.exists(out) and not [f for f in os.listdir(tmp_path) if f.startswith("out.vcf")]


@pytest.mark.parametrize("value", ["x", "VCF", "vcf.gz", "v", ""])
def test_unknown_format_is_refused(tmp_path, value):
    r, out = _run(tmp_path, "--format", value)
    _refused(tmp_path, r, out)


@pytest.mark.parametrize("args", [("--format", "vcf", "--rank", "0", "--world", "2"), ("--rank", "1", "--world", "2", "--format", "vcf"),
                                  ("--format", "vcf", "--merge", "2"), ("-O", "u", "--merge", "3", "--format", "vcf")])
def test_text_output_of_a_sharded_run_is_refused(tmp_path, args):
    r, out = _run(tmp_path, *args)
    _refused(tmp_path, r, out)


@pytest.mark.parametrize("var", ["BAM2BCF_HOST_READER", "BAM2BCF_HOST_BCF", "BAM2BCF_HOST_PREP"])
def test_text_output_with_a_host_variant_is_refused(tmp_path, var):
    r, out = _run(tmp_path, "--format", "vcf", env={var: "1"})
    _refused(tmp_path, r, out)


def fmt_g(values):
    L = _lib.load()
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros((len(v), 16), dtype=np.uint8)
    assert L.bsc_fmt_g(v.ctypes.data, len(v), out.ctypes.data) == 0
    assert (out[:, 15] <= 12).all()
    return [bytes(o[: o[15]]) for o in out], out


def test_host_fmt_g_is_the_c_library_s():
    rng = np.random.default_rng(20260)
    bits = rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32)
    v = np.concatenate([bits.view(np.float32), np.array(TIES, dtype=np.float32)])
    v = v[~np.isnan(v)]
    got, slots = fmt_g(v)
    for f, g, s in zip(v, got, slots):
        assert g == ("%g" % float(f)).encode(), (f, g)
        assert not s[len(g) : 15].any()  # zero padding
    assert got[-len(TIES) :][:5] == [b"100000", b"100002", b"1e+06", b"1.00002e+06", b"1e+06"]


def test_host_fmt_g_spells_nan_by_the_sign_bit():
    v = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    assert fmt_g(v)[0] == [b"nan", b"-nan", b"nan", b"-nan"]


def test_fmt_g_refuses_null():
    L = _lib.load()
    assert L.bsc_fmt_g(None, 3, None) == -1
    assert L.bsc_fmt_g(None, 0, None) == 0
