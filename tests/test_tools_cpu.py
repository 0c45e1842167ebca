"""CPU tests of the benchmark tooling: the scaling harness builds one torchrun per
N (127.0.0.1 rendezvous), parses bench.py's JSON line and computes weak-scaling
efficiency against N = 1."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import scaling  # noqa: E402


def test_commands():
    one = scaling.command(1, 10, 2, 29600, [])
    assert one[1].endswith("bench.py") and "--gpus" in one and "1" in one
    eight = scaling.command(8, 10, 2, 29601, ["--batch", "128"])
    assert "torch.distributed.run" in eight and "--nproc-per-node" in eight
    assert eight[eight.index("--master-addr") + 1] == "127.0.0.1"
    assert eight[-2:] == ["--batch", "128"]


def test_parse_and_table():
    def line(n, v):
        return json.dumps({"metric": "images/sec", "value": v, "unit": "images/sec", "n_gpus": n,
                           "ms_per_step": 28.0})
    out = "warning: x\n" + line(2, 18000.0) + "\n"
    r = scaling.parse_line(out)
    assert r["n_gpus"] == 2 and r["value"] == 18000.0
    assert scaling.parse_line("no json here") is None
    t = scaling.table([json.loads(line(1, 9000.0)), json.loads(line(2, 18000.0)), json.loads(line(8, 68400.0))])
    assert "| 2 | 18000.0 images/sec | 9000.0 |" in t and "100.0 %" in t and "95.0 %" in t


def test_bench_dump_outputs_is_reproducible(tmp_path):
    """``bench.py --dump-outputs DIR`` (CPU, the tiny plumbing model): the last timed
    step's loss and updated weights land as float32 ``.npy`` files, identical from run
    to run; ``--steps`` sets the timed steps and ``ms_per_step`` is in the result line.
    ``--full`` is accepted."""
    import subprocess
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    runs = []
    for d, extra in (("a", []), ("b", ["--full"])):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--device", "cpu", "--model", "resnet_tiny", "--batch", "4", "--image", "32",
               "--dump-outputs", str(tmp_path / d), *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        res = json.loads(p.stdout.strip().splitlines()[-1])
        assert res["steps"] == 2 and res["ms_per_step"] > 0
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["loss.npy", "weights_norms_biases.npy", "weights_weights.npy"]
        arrs = {f: np.load(tmp_path / d / f) for f in files}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert np.abs(arrs["weights_weights.npy"]).max() > 0
        assert abs(float(arrs["loss.npy"][0]) - res["config"]["loss"]) < 1e-6
        runs.append(arrs)
    for f in runs[0]:
        np.testing.assert_array_equal(runs[0][f], runs[1][f])


def test_bench_dump_samples_large_groups(tmp_path, monkeypatch):
    """A group larger than ``DUMP_SAMPLE`` is written as a fixed sample: sorted
    seeded indices, the same for every array of that length."""
    import types
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    big = types.SimpleNamespace(name="weights", data=torch.arange(5000.))
    same = types.SimpleNamespace(name="again", data=-torch.arange(5000.).bfloat16())
    small = types.SimpleNamespace(name="norms_biases", data=torch.ones(7))
    eng = types.SimpleNamespace(groups=[big, same, small], wait=lambda: None)
    bench.dump_outputs(eng, 1.5, str(tmp_path))
    w = np.load(tmp_path / "weights_weights.npy")
    assert w.dtype == np.float32 and w.shape == (100,)
    idx = w.astype(np.int64)
    assert (np.diff(idx) >= 0).all() and 0 <= idx.min() and idx.max() < 5000 and len(set(idx)) > 50
    np.testing.assert_array_equal(np.load(tmp_path / "weights_again.npy"),
                                  -torch.arange(5000.).bfloat16().float().numpy()[idx])
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "weights_again.npy", "weights_norms_biases.npy",
                                            "weights_weights.npy"]
    assert np.load(tmp_path / "weights_norms_biases.npy").shape == (7,)
    assert np.load(tmp_path / "loss.npy").tolist() == [1.5]


def test_dry_run_returns_zero(capsys):
    assert scaling.main(["--dry-run", "--gpus", "1", "2"]) == 0
    err = capsys.readouterr().err
    assert err.count("$ ") == 2
