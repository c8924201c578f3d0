"""bench.py --dump-outputs on CPU tensors: size cap, dtypes, and the same sample positions in every run."""
import json
import os

import numpy as np
import torch


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones(tmp_path):
    import bench

    g = torch.Generator().manual_seed(3)
    outs = {"cost_volume": torch.randn(32, 64, 96, 128, generator=g), "lowest": torch.randn(32, 96, 128, generator=g),
            "mask": torch.rand(32, 96, 128, generator=g) > 0.5, "planes": torch.linspace(0.25, 5.0, 64, dtype=torch.float64)}
    for d in ("a", "b"):
        bench._dump_outputs(outs, str(tmp_path / d))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20, total
    man = json.load(open(tmp_path / "a" / "manifest.json"))
    assert sorted(man) == sorted(outs)
    for name, t in outs.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert np.array_equal(a, b), name
        if man[name]["sample"] is None:
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.to(torch.float64 if t.dtype == torch.float64 else torch.float32).numpy())
    s = man["cost_volume"]["sample"]
    assert s is not None and s["of"] == outs["cost_volume"].numel() and 0 < s["elements"] < s["of"]
    idx = torch.randperm(s["of"], generator=torch.Generator().manual_seed(s["seed"]))[:s["elements"]].sort().values
    assert np.array_equal(np.load(tmp_path / "a" / "cost_volume.npy"), outs["cost_volume"].reshape(-1)[idx].numpy())
    assert man["mask"]["sample"] is None and man["mask"]["dtype"] == "bool"


def test_bench_steps_must_be_positive():
    import pytest

    import bench

    assert bench.parse(["--steps", "7"]).steps == 7 and not bench.parse([]).full and bench.parse([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
