"""CPU checks of bench.py's command line: a plain run leaves every side measurement to --full, and --dump-outputs writes the timed path's
outputs as float32 / float64 .npy files within the size budget, the same ones from run to run."""
import os

import numpy as np
import pytest
import torch


def test_plain_run_leaves_side_measurements_to_full():
    import bench

    side = ("no_cpu_baseline", "no_profile", "no_live_traffic", "no_strict_fp32", "no_secondary", "no_parity_check")
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)
    assert all(getattr(a, k) for k in side)
    a = bench.parse(["--full"])
    assert a.full and not any(getattr(a, k) for k in side)
    a = bench.parse(["--full", "--no-secondary", "--dump-outputs", "out"])
    assert a.no_secondary and not a.no_profile and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_types_budget_and_seeded_sample(tmp_path):
    import bench

    g = torch.Generator().manual_seed(3)
    small = torch.randn((2, 3, 4, 5), generator=g)
    big = torch.randn((64, 1000), generator=g)
    K = torch.tensor([150, 7, 0], dtype=torch.int32)
    outs = {"small": small, "big": big, "K": K}
    budget = 3 * 16000  # a share of 16000 bytes each: `big` (256000 bytes as float32) is sampled
    info = bench.dump_outputs(outs, str(tmp_path / "a"), budget=budget)
    bench.dump_outputs(outs, str(tmp_path / "b"), budget=budget)
    files = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in outs}
    assert files["small"].dtype == np.float32 and np.array_equal(files["small"], small.numpy())
    assert files["K"].dtype == np.float64 and files["K"].tolist() == [150.0, 7.0, 0.0]
    assert files["big"].dtype == np.float32 and files["big"].size == 16000 // 4
    assert np.isin(files["big"], big.numpy()).all()
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") - 128 for n in outs) <= budget  # (128-byte .npy header each)
    for n in outs:  # the same arguments give the same files
        assert np.array_equal(files[n], np.load(tmp_path / "b" / f"{n}.npy"))
    assert info["small"]["written"] == "all" and info["big"]["written"].startswith("seeded sample")
    assert info["big"]["shape"] == [64, 1000]
