"""bench.py's plain run: the headline record and nothing that --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_plain_run_prints_the_headline_only(tmp_path):
    """`python bench.py --steps 2 --warmup 1 --dump-outputs DIR`: one JSON line with the contract's keys, none of the --full keys,
    and the last timed step's losses written"""
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--dump-outputs", out]
    r = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    rec = json.loads(lines[0])
    assert rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["config"]["parallelism"] == "dp1"
    assert rec["value"] > 0 and rec["value"] == pytest.approx(4.0 * 1e3 / rec["ms_per_step"], rel=1e-3)
    for k in ("roofline", "step_launch", "ranks_in_sync", "fp32_ms_per_step", "b2_ms_per_step", "cpu_baseline"):
        assert k not in rec, k
    losses = [f for f in os.listdir(out) if not f.startswith("param.")]
    assert losses and all(np.isfinite(np.load(os.path.join(out, f))).all() for f in losses)
