"""bam2bcf -D on the CPU: what it refuses is refused before the index is opened or a context is created (status 2, a message that names -D),
and an index that is missing or is not one ends the program with the reader's text before any device is asked for."""
import os
import subprocess

import pytest

import dbsnp_crafted as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")


def _run(tmp_path, *args, env=None):
    assert os.path.exists(EXE), "run `make demo`"
    out = str(tmp_path / "out.bcf")
    r = subprocess.run([EXE, *args, str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), out, str(tmp_path / "rep.json")], capture_output=True,
                       text=True, timeout=60, env=dict(os.environ, **(env or {})))
    return r, out


def _refused(tmp_path, r, out, *words):
    assert r.returncode == 2, r.stderr + r.stdout
    assert "-D" in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert not os.path.exists(out) and not [f for f in os.listdir(tmp_path) if f.startswith("out.bcf")]


@pytest.fixture()
def index(tmp_path):
    return K.write(tmp_path / "crafted.idx", K.crafted_contigs())


@pytest.mark.parametrize("args", [("--rank", "0", "--world", "2"), ("--world", "2"), ("--merge", "2"), ("-O", "u", "--merge", "3"), ("--format", "bcf", "--rank", "1", "--world", "4")])
@pytest.mark.parametrize("joined", [False, True])
def test_dbsnp_of_a_sharded_run_is_refused(tmp_path, index, args, joined):
    d = ("-D" + index,) if joined else ("-D", index)
    for order in (d + args, args + d):
        r, out = _run(tmp_path, *order)
        _refused(tmp_path, r, out, "sharded run", "--rank / --world / --merge")


@pytest.mark.parametrize("var", ["BAM2BCF_HOST_READER", "BAM2BCF_HOST_BCF", "BAM2BCF_HOST_PREP"])
def test_dbsnp_with_a_host_variant_is_refused(tmp_path, index, var):
    r, out = _run(tmp_path, "-D", index, env={var: "1"})
    _refused(tmp_path, r, out, "BAM2BCF_HOST_READER / _HOST_BCF / _HOST_PREP")


def test_missing_index_ends_with_the_reader_s_text(tmp_path):
    r, out = _run(tmp_path, "-D", str(tmp_path / "nothing.idx"))
    assert r.returncode not in (0, 2) and "bsc_dbsnp_open: cannot open" in r.stderr and "nothing.idx" in r.stderr, r.stderr
    assert not os.path.exists(out)


@pytest.mark.parametrize("content", [b"", b"not an index at all, but long enough to hold a header of 32 bytes", b"\x34\x84\x27\xd7" + b"\0" * 60])
def test_garbage_index_ends_with_the_reader_s_text(tmp_path, content):
    p = tmp_path / "garbage.idx"
    p.write_bytes(content)
    r, out = _run(tmp_path, "-O", "b", "-D", str(p))
    assert r.returncode not in (0, 2) and "bsc_dbsnp_open:" in r.stderr, r.stderr
    assert not os.path.exists(out)


def test_usage_names_the_option(tmp_path):
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[-D dbsnp.idx]" in r.stderr
