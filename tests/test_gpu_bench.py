"""bench.py on the GPU, at a tiny size: a plain run prints the headline alone, `--full` adds the figures measured by runs of
their own, and what the timed steps computed (--dump-outputs) does not depend on which of the two ran."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "step_times", "whole_job_alg_GBps_per_gpu", "end_to_end", "value_end_to_end")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--windows", "4", *extra],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--dump-outputs", str(tmp_path / "full"), "--no-cpu-baseline", "--no-orb", "--no-sweeps",
                  "--inertial-windows", "0", "--e2e-batches", "2")
    for out in (plain, full):
        assert all(k in out for k in HEADLINE)
        assert out["unit"] == "windows/s" and out["dtype"] == "f64" and out["higher_is_better"] is True
        assert abs(out["value"] - 4 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert plain["metric"] == full["metric"]
    assert not [k for k in FULL_ONLY if k in plain]
    assert all(k in full for k in FULL_ONLY)
    a = {p.name: np.load(p) for p in (tmp_path / "plain").glob("*.npy")}
    b = {p.name: np.load(p) for p in (tmp_path / "full").glob("*.npy")}
    assert a and a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
