"""A plain bench.py run does only what its headline figure needs; --full adds the companion measurements and checks
(sustained rate, the other backward arithmetics, forward-only rate, roofline launches, CPU baseline) after the same timed
steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANIONS = ("sustained", "fp32_class", "exact_weight_chain", "render_only_value", "roofline", "roofline_inference",
              "cpu_baseline")


def _bench(extra_args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--rays", "1024"] + extra_args, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only():
    out = _bench([])
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0 and out["config"]["full"] is False
    assert [k for k in COMPANIONS if out.get(k) is not None] == []


def test_full_run_adds_the_companions():
    out = _bench(["--full", "--sustained-seconds", "0.1"])
    assert out["steps"] == 3 and out["value"] > 0 and out["config"]["full"] is True
    assert [k for k in COMPANIONS if out.get(k) is None] == []
    assert out["sustained"]["steps"] >= 100
    for k in ("fp32_class", "exact_weight_chain"):
        assert out[k]["ms_per_step"] > 0 and out[k]["sustained"]["steps"] >= 100
    assert out["roofline"]["launch_ms"] > 0 and out["cpu_baseline"]["value"] > 0
