"""bench.py end to end on a small catalogue that still takes the int8 cascade (>= 262,144 items): the plain run prints the
headline line and dumps the last timed step's lists; --full adds the oracle parity check of that same step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--users", "20000", "--items", "300000", "--steps", "2", "--warmup", "1"]


def _run(args, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def _load(d):
    return [np.load(os.path.join(d, n)) for n in ("topk_values.npy", "topk_ids.npy", "user_ids.npy")]


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_step_and_full_run_checks_it(tmp_path):
    plain = _run(SMALL + ["--dump-outputs", str(tmp_path / "plain")], tmp_path)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["dtype"] == "i8/bf16/fp32"
    assert abs(plain["value"] - 20000 * 300000 / (plain["ms_per_step"] * 1e-3)) <= 1e-3 * plain["value"]
    assert "topk_ids_bit_exact" not in plain["config"]["checks"] and plain["cpu_baseline"] is None   # (--full only)
    v, i, u = _load(str(tmp_path / "plain"))
    assert v.shape == i.shape == (20000, 10) and v.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(u, np.arange(20000)) and np.all(i == np.round(i)) and i.min() >= 0 and i.max() < 300000
    assert np.all(np.diff(v, axis=1) <= 0)

    full = _run(SMALL + ["--full", "--configs", "headline", "--no-fit", "--no-cpu-baseline", "--no-fp32-mode", "--no-k1-multi",
                         "--parity-users", "256", "--dump-outputs", str(tmp_path / "full")], tmp_path)
    checks = full["config"]["checks"]
    assert checks["topk_ids_bit_exact"] is True and checks["topk_values_bit_exact"] is True and checks["parity_users"] == 256
    # same arguments -> same inputs -> the same lists, and those are the ones the oracle check passed
    for a, b in zip(_load(str(tmp_path / "plain")), _load(str(tmp_path / "full"))):
        assert np.array_equal(a, b)
