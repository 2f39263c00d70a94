"""bench.py's command line: --dump-outputs writes the last timed step's outputs as .npy files
(fp32 / fp64, a fixed sample where an array is over its share of the budget), and a plain run
skips the legs that --full adds (cpu_baseline, alt_modes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_full_and_dump_options_default_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")


def test_dump_outputs_types_and_whole_arrays(tmp_path):
    T = np.arange(16, dtype=np.float64).reshape(4, 4) / 3.0
    idx = torch.arange(10, dtype=torch.int32).reshape(5, 2) + (1 << 30)
    h = torch.linspace(0, 1, 7, dtype=torch.float16)
    bench.dump_outputs(str(tmp_path), {"T": T, "err": 0.125, "idx": idx, "h": h})
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("T", "err", "idx", "h")}
    assert got["T"].dtype == np.float64 and np.array_equal(got["T"], T)
    assert got["err"].dtype == np.float64 and got["err"].tolist() == [0.125]
    assert got["idx"].dtype == np.float64 and np.array_equal(got["idx"], idx.numpy().astype(np.float64))
    assert got["h"].dtype == np.float32 and np.array_equal(got["h"], h.float().numpy())


def test_dump_outputs_samples_within_budget_and_repeats(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)  # two arrays: 2000 B each
    big = torch.arange(3000, dtype=torch.float32).reshape(1000, 3)  # 12 B rows -> 166 rows kept
    ids = torch.arange(1000, dtype=torch.int64)                     # 8 B rows -> 250 kept
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "ids": ids})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (166, 3) and a.dtype == np.float32 and np.array_equal(a, b)
    rows = (a[:, 0] / 3).astype(int)
    assert np.array_equal(a, big.numpy()[rows]) and np.all(np.diff(rows) >= 0)
    i = np.load(tmp_path / "a" / "ids.npy")
    assert i.shape == (250,) and i.dtype == np.float64 and np.all(np.diff(i) >= 0)
    assert a.nbytes + i.nbytes <= 4000


@pytest.mark.gpu
def test_plain_run_dumps_the_pose_it_reports(tmp_path):
    """A plain 1-GPU run at a small size: exactly --steps timed steps, no CPU baseline or
    alt_modes, and T.npy is the pose whose distance from the truth the line quotes."""
    from pointcloudprocess_amd import synth
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--points", "1000000", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=120).stdout
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "Mcorrespondences/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    # value and ms_per_step are the same measurement (ms_per_step is rounded to 1e-3 ms, a step takes > 0.5 ms)
    assert line["value"] == pytest.approx(1e6 * 20 / line["ms_per_step"] / 1e3, rel=2e-3)
    assert line["cpu_baseline"] is None and line["alt_modes"] is None
    assert sorted(os.listdir(tmp_path)) == ["T.npy", "err.npy", "guard_ok.npy"]
    T, err, ok = (np.load(tmp_path / n) for n in ("T.npy", "err.npy", "guard_ok.npy"))
    assert T.shape == (4, 4) and T.dtype == np.float64 and err.dtype == np.float64
    assert float(np.abs(T - synth.rigid()).max()) == line["icp_max_abs_T_err_vs_truth"]
    assert round(float(err[0]), 6) == line["icp_final_rms_m"] and bool(ok[0]) == line["halo_guard_ok"]
