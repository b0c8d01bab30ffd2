"""The dbSNP indexes the tests of the device-resident index share (tests/test_dbsnp_flat_host.py, tests/test_gpu_dbsnp_dev.py,
tests/test_dbsnp_cli.py), written by tools/make_dbsnp_index.py.

crafted_contigs(): every shape the flat form and its kernels have to get right — position 1; a bin with all 64 positions set and a full
bin next to it; bins with one entry at bit 0 and at bit 63; a gap of more than 65 536 bins (the 4-byte increment); names of 1, 2, 9, 10
and 41 digits (odd counts carry the filler); the fourth prefix, which takes the explicit two-byte index; fq on a tenth of the sites; a
second contig.  "chrZ" is the contig the index lacks."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_dbsnp_index", os.path.join(ROOT, "tools", "make_dbsnp_index.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

PREFIXES = ("rs", "ss", "x", "longprefix_")
ABSENT = "chrZ"
_DIGITS = ("7", "42", "123456789", "1234567890", "12345678901234567890123456789012345678901")  # 1, 2, 9, 10, 41 digits


def crafted_contigs():
    a = [(1, "1", False, 0)]
    k = 0
    for pos in list(range(128, 256)):  # bins 2 and 3: two full bins side by side
        a.append((pos, _DIGITS[k % 5][: 1 + k % 41] if k % 7 == 0 else str(5000 + k), k % 10 == 3, k % 4))
        k += 1
    a.append((64 * 10, _DIGITS[0], True, 3))            # one entry, bit 0
    a.append((64 * 11 + 63, _DIGITS[1], False, 3))      # one entry, bit 63
    a.append((64 * 12 + 5, _DIGITS[2], False, 1))
    a.append((64 * 12 + 6, _DIGITS[3], True, 2))
    a.append((64 * 12 + 7, _DIGITS[4], False, 3))
    a.append((64 * 100 + 31, _DIGITS[4], True, 0))      # distance 88 bins: the 2-byte increment
    a.append((64 * 500 + 1, "31", False, 0))            # distance 400: the 3-byte increment
    far = 64 * (500 + 66_000)                           # a gap of more than 65 536 bins: the 5-byte increment
    for i in range(40):
        a.append((far + 3 * i, _DIGITS[i % 5], i % 10 == 0, i % 4))
    b = [(5, "42", True, 0), (64 * 3 + 63, "777", False, 3), (64 * 4, "8", False, 1)] + [(1000 + 9 * i, str(90 + i), i % 10 == 1, i % 4) for i in range(300)]
    return {"chrA": a, "chrB": b}


def random_sites(length, spacing, seed):
    """about length / spacing sites at random positions of 1 .. length: random digit counts (1 .. 12), prefixes and fq flags (a tenth)"""
    rng = np.random.default_rng(seed)
    pos = np.unique(rng.integers(1, length + 1, size=length // spacing))
    nd = rng.integers(1, 13, size=len(pos))
    val = rng.integers(0, 10**12, size=len(pos))
    fq = rng.integers(0, 10, size=len(pos)) == 0
    pix = rng.integers(0, len(PREFIXES), size=len(pos))
    return [(int(p), ("%012d" % v)[:d], bool(f), int(q)) for p, d, v, f, q in zip(pos, nd, val, fq, pix)]


def write(path, contigs):
    W.write_index(str(path), contigs, prefixes=PREFIXES)
    return str(path)
