"""bench.py's outputs: --dump-outputs writes the last timed step's loss and parameters as float .npy files within its budget (a
large array as a fixed sample of its rows), and a plain run -- no --full -- times the steps it is asked for and nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeEngine(object):
    """all_names() / param() as the engines have them; x_local is larger than one array of the dump may be."""

    def __init__(self, n_persons):
        self.n = n_persons

    def all_names(self):
        return ["b", "encoder$$$fc1.weight", "x_local"]

    def param(self, name):
        if name == "b":
            return torch.linspace(-1.0, 1.0, 7)
        if name == "encoder$$$fc1.weight":
            return torch.arange(12, dtype=torch.float64).reshape(3, 4)
        return torch.arange(self.n, dtype=torch.float32)[:, None].repeat(1, 2)      # row i holds i, i


def test_dump_outputs_writes_float_arrays_and_a_fixed_row_sample(tmp_path):
    import bench
    n = bench.DUMP_MAX_ELEMENTS                     # two values a row: twice what one array may hold
    eng = _FakeEngine(n)
    loss = torch.tensor(123.5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), eng, loss)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["loss.npy", "param.b.npy", "param.encoder.fc1.weight.npy", "param.x_local.npy"]
    for nm in names:
        a, b = np.load(str(tmp_path / "a" / nm)), np.load(str(tmp_path / "b" / nm))
        assert a.dtype in (np.float32, np.float64), (nm, a.dtype)
        np.testing.assert_array_equal(a, b)         # same arguments, same arrays, the same sampled rows
    assert np.load(str(tmp_path / "a" / "loss.npy")).tolist() == [123.5]
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "param.encoder.fc1.weight.npy")),
                                  np.arange(12, dtype=np.float32).reshape(3, 4))
    x = np.load(str(tmp_path / "a" / "param.x_local.npy"))
    assert x.shape == (n // 2, 2)
    rows = x[:, 0].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n    # distinct rows of the array, in order
    np.testing.assert_array_equal(x[:, 1], x[:, 0])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_them(tmp_path):
    """No --full: the line has the asked-for number of timed steps and ms_per_step, none of the figures --full adds; the dump
    holds the loss the line reports as loss_last."""
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--persons", "65536", "--dump-outputs", out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    for key in ("cpu_baseline", "board", "graph_replay_ms_per_step"):
        assert key not in d, key
    names = sorted(os.listdir(out))
    assert "loss.npy" in names and "param.a.npy" in names and "param.b.npy" in names, names
    assert np.load(os.path.join(out, "loss.npy")).tolist() == [d["loss_last"]]
    total = 0
    for nm in names:
        a = np.load(os.path.join(out, nm))
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), nm
        total += a.nbytes
    assert total <= 64 << 20
