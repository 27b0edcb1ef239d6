"""bench.py's command line: a plain run is the headline leg alone (--full off by default), and --dump-outputs
writes what VecTask.step returned as float32 .npy files."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_writes_the_step_result_as_float32(tmp_path):
    g = torch.Generator().manual_seed(3)
    obs = torch.randn(5, 188, generator=g)
    rew = torch.randn(5, generator=g)
    reset = torch.tensor([True, False, False, True, False])
    time_outs = torch.tensor([False, False, False, True, False])
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), ({"obs": obs}, rew, reset, {"time_outs": time_outs}), 0, 1)
    assert sorted(os.listdir(out)) == ["obs.npy", "reset.npy", "rew.npy", "time_outs.npy"]
    got = {n: np.load(out / f"{n}.npy") for n in ("obs", "rew", "reset", "time_outs")}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["obs"], obs.numpy()) and np.array_equal(got["rew"], rew.numpy())
    assert got["reset"].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0] and got["time_outs"].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]
    bench.dump_outputs(str(out), ({"obs": obs}, rew, reset, {"time_outs": time_outs}), 1, 2)
    assert os.path.exists(out / "obs.rank1.npy")
