"""bench.py's command line: a plain run (headline only) vs ``--full``, and ``--dump-outputs``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default_and_steps_must_be_positive():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--steps", "2", "--full", "--dump-outputs", "out_dir"])
    assert a.full and a.dump_outputs == "out_dir"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_sample_keeps_small_arrays_and_samples_large_ones_at_fixed_positions():
    import bench
    small = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    s = bench.dump_sample("small", small)
    assert s.dtype == np.float32 and s.shape == (3, 4) and (s == small.numpy()).all()
    big = torch.randn(bench.DUMP_CAP + 1000, generator=torch.Generator().manual_seed(0))
    a, b = bench.dump_sample("big", big), bench.dump_sample("big", big.clone())
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_CAP,) and (a == b).all()        # same positions every run
    assert not (bench.dump_sample("other", big) == a).all()                               # the seed follows the name
    assert np.isin(a, big.numpy()).all()


@pytest.mark.gpu
def test_plain_bench_run_prints_the_contract_fields_and_dumps_the_last_step(tmp_path):
    """A plain run at a small shape: the contract fields only (nothing measured beside the headline), exactly --steps timed
    steps, and the last step's output, loss / MCD and parameters as float .npy files within 64 MB."""
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "8", "--channels", "8", "--timepoints", "100", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - 8 / (line["ms_per_step"] * 1e-3)) < 1e-2 * line["value"]
    assert not {"roofline", "cpu_baseline", "gpu_state", "step0", "c2_lite", "c5", "signal_c5"} & set(line)
    files = sorted(os.listdir(out_dir))
    assert "out.npy" in files and "loss_mcd.npy" in files and any(f.startswith("param.") for f in files)
    total = 0
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(out_dir / "out.npy").shape == (8, 80)
    loss, mcd = np.load(out_dir / "loss_mcd.npy")
    assert loss > 0 and mcd > 0
