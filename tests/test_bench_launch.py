"""`python bench.py --gpus N` starts its own ranks (one process per GPU — the reference's unit is one process per contig,
/root/reference README.md:73-76) without the parent touching a GPU: checked here on the CPU by intercepting the child
command."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_gpus_n_launches_one_rank_per_gpu(monkeypatch):
    import subprocess

    b = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5", "--warmup", "2"])
    # a torch import in the parent would be harmless, a torch.cuda call would not: main() must leave before either
    monkeypatch.setitem(sys.modules, "torch", None)
    try:
        b.main()
        code = None
    except SystemExit as e:
        code = e.code
    assert code == 7  # the child's exit code is the parent's
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-7] == os.path.join(ROOT, "bench.py") and cmd[-6:] == ["--gpus", "4", "--steps", "5", "--warmup", "2"]
    assert seen["env"]["MASTER_ADDR"] == "127.0.0.1" and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_under_a_launcher_bench_does_not_launch_again(monkeypatch):
    import subprocess

    b = _bench()
    monkeypatch.setattr(subprocess, "call", lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched again")))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setitem(sys.modules, "torch", None)  # the next statement after the launch decision is `import torch`
    try:
        b.main()
        raise AssertionError("expected the torch import to be reached")
    except ImportError:
        pass


def test_dump_outputs_writes_a_fixed_float64_sample(tmp_path):
    """--dump-outputs: the same seeded sample of positions every run, every array float64, the whole dump within 64 MB."""
    import numpy as np
    import torch

    b = _bench()
    n = 3_000_000
    g = torch.Generator().manual_seed(1)
    d_out = torch.randint(0, 256, (n * 200,), dtype=torch.uint8, generator=g)
    d_skip = torch.randint(0, 2, (n,), dtype=torch.uint8, generator=g)
    counters = np.arange(13, dtype=np.int64)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), d_out, d_skip, n, counters)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "position.npy" in names and "gt_meth_gt_prob.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and x.tobytes() == y.tobytes(), f
    pos = np.load(tmp_path / "a" / "position.npy").astype(np.int64)
    assert len(pos) == b.DUMP_SITES and pos.max() < n and (np.diff(pos) > 0).all()
    import bs_call_amd as B

    rec = d_out.view(n, 200)[torch.from_numpy(pos)].numpy().reshape(-1).view(B.GT_METH)
    assert (np.load(tmp_path / "a" / "gt_meth_counts.npy") == rec["counts"].astype(np.float64)).all()
    assert (np.load(tmp_path / "a" / "skip.npy") == d_skip.numpy()[pos]).all()
    assert (np.load(tmp_path / "a" / "counters.npy") == counters).all()


def test_dump_outputs_is_refused_for_config3(monkeypatch, capsys):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "3", "--dump-outputs", "x"])
    try:
        b.main()
        raise AssertionError("expected a usage error")
    except SystemExit as e:
        assert e.code == 2
    assert "--dump-outputs" in capsys.readouterr().err
