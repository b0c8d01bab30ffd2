"""The flat form of a loaded dbSNP contig (bsc_dev_dbsnp_flatten, csrc/dbsnp.c) and the statements the device kernels read it with
(csrc/dbsnpdev_core.h), on the CPU: tests/dbsnpdev/dbsnp_flat_host.c is compiled with csrc/dbsnp.c as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer and compares flags, counts, positions, lengths and name bytes with the reader's own
bsc_dbsnp_flags / bsc_dbsnp_name / bsc_dbsnp_names — for the crafted index of tests/dbsnp_crafted.py and for a random one."""
import os
import subprocess

import pytest

import dbsnp_crafted as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dbsnp_flat") / "dbsnp_flat_host")
    subprocess.run([os.environ.get("CC", "gcc"), "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "bs_call_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dbsnpdev", "dbsnp_flat_host.c"), os.path.join(ROOT, "bs_call_amd", "csrc", "dbsnp.c"), "-lz", "-o", out],
                   check=True)
    return out


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def test_crafted_index(exe, tmp_path):
    idx = K.write(tmp_path / "crafted.idx", K.crafted_contigs())
    p = _run(exe, idx, "chrA", "chrB", K.ABSENT, "chrA")
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:] + p.stderr[-3000:]


def test_random_index(exe, tmp_path):
    idx = K.write(tmp_path / "random.idx", {"chrR": K.random_sites(60_000, 3, 11), "chrT": [(p + 64 * 5000, d, f, q) for p, d, f, q in K.random_sites(40_000, 40, 12)]})
    p = _run(exe, idx, "chrR", "chrT")
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:] + p.stderr[-3000:]


def test_prefix_index_out_of_range_refuses_the_flattening(exe, tmp_path):
    ctgs = K.crafted_contigs()
    ctgs["chrBad"] = [(70, "11", False, 0), (64 * 9 + 17, "12345", False, len(K.PREFIXES))]  # an explicit index one behind the last prefix
    idx = K.write(tmp_path / "bad.idx", ctgs)
    p = _run(exe, "--refuse", idx, "chrBad")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "position %d names prefix %d of %d" % (64 * 9 + 17, len(K.PREFIXES), len(K.PREFIXES)) in p.stdout
    p = _run(exe, idx, "chrA")  # the file's other contigs flatten as before
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:] + p.stderr[-3000:]
