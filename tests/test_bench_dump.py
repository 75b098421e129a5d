"""CPU: ``bench.py --dump-outputs DIR`` writes every output of the last timed step as float32 / float64 .npy files, within the
64 MB budget, cutting large arrays down to the same seeded sample on every run."""
import os
import sys
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_step_outputs_walk_the_loss_output_the_inference_outputs_and_the_state():
    @dataclass
    class Lo:
        loss: torch.Tensor
        reconstruction_loss: dict
        kl_local: dict
        extra_metrics: dict = field(default_factory=dict)

    class T:
        last_outputs = ({"private_stats": {0: {"loc": torch.ones(4, 2), "qz": torch.distributions.Normal(0.0, 1.0)}},
                         "library": {0: torch.zeros(4, 1, dtype=torch.float64)}}, {"px": None})

    module = torch.nn.BatchNorm1d(3)
    lo = Lo(torch.tensor(2.5), {"rec_1": torch.arange(4.0).to(torch.bfloat16)}, {"kl_1": torch.ones(4)})
    a = bench.step_outputs(lo, T(), module)
    assert set(a) == {"loss", "reconstruction_loss.rec_1", "kl_local.kl_1", "inference.private_stats.0.loc", "inference.library.0",
                      "state.weight", "state.bias", "state.running_mean", "state.running_var", "state.num_batches_tracked"}
    assert a["loss"].shape == () and a["loss"].dtype == np.float32 and float(a["loss"]) == 2.5
    assert a["reconstruction_loss.rec_1"].dtype == np.float32 and a["reconstruction_loss.rec_1"].tolist() == [0, 1, 2, 3]
    assert a["inference.library.0"].dtype == np.float64 and a["state.num_batches_tracked"].dtype == np.float64


def test_small_outputs_are_written_whole(tmp_path):
    arrays = {"loss": np.float32(1.5).reshape(()), "z": np.arange(12, dtype=np.float32).reshape(3, 4), "w": np.ones(5)}
    info = bench.dump_outputs(str(tmp_path), arrays)
    got = _load(tmp_path)
    assert set(got) == set(arrays) and info["sampled"] == [] and info["sample_fraction"] == 1.0
    for k, v in arrays.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v)


def test_large_outputs_are_a_fixed_seeded_sample_within_the_budget(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"loss": np.float32(3.0).reshape(()), "small": rng.random(1000).astype(np.float32),
              "big_a": rng.random(300_000).astype(np.float32), "big_b": rng.random((400, 500))}
    budget = 1_000_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget
    assert np.array_equal(a["small"], arrays["small"]) and float(a["loss"]) == 3.0
    for k in ("big_a", "big_b"):
        assert np.array_equal(a[k], b[k]) and a[k].dtype == arrays[k].dtype
        assert 0 < a[k].size < arrays[k].size and np.isin(a[k], arrays[k].reshape(-1)).all()


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    assert bench.parse(["--steps", "7", "--dump-outputs", "out"]).dump_outputs == "out"
