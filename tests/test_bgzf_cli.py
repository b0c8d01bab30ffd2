"""bam2bcf's output-type option (-O u|b) on the CPU: what it refuses is refused before a context is created, so no GPU is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bs_call_amd", "lib", "bam2bcf")


def _run(tmp_path, *args):
    assert os.path.exists(EXE), "run `make demo`"
    out = str(tmp_path / "out.bcf")
    r = subprocess.run([EXE, *args, str(tmp_path / "in.bam"), str(tmp_path / "ref.fa"), out, str(tmp_path / "rep.json")],
                       capture_output=True, text=True, timeout=60)
    return r, out


@pytest.mark.parametrize("args", [("-O", "b", "--rank", "0", "--world", "2"), ("--rank", "1", "--world", "2", "-O", "b"), ("-O", "b", "--merge", "2"),
                                  ("-Ob", "--merge", "3")])
def test_compressed_output_of_a_sharded_run_is_refused(tmp_path, args):
    r, out = _run(tmp_path, *args)
    assert r.returncode == 2, r.stderr + r.stdout
    assert "-O" in r.stderr
    assert not os.path.exists(out) and not [f for f in os.listdir(tmp_path) if f.startswith("out.bcf")]


@pytest.mark.parametrize("value", ["x", "z", "v", ""])
def test_unknown_output_type_is_refused(tmp_path, value):
    r, out = _run(tmp_path, "-O", value)
    assert r.returncode == 2, r.stderr + r.stdout
    assert "-O" in r.stderr
    assert not os.path.exists(out)
