"""bench.py --dump-outputs on the real timed path: the last timed step's result dict, loss, gradients and updated
parameters land in the directory, finite, with the step count the command asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(extra_args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--rays", "1024",
                        "--no-extras", "--sustained-seconds", "0"] + extra_args,
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_train_dump(tmp_path):
    out = _bench(["--steps", "3", "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    d = out["dump_outputs"]
    assert d["rays_written"] == 1024 and d["bytes"] <= 64 << 20
    files = os.listdir(tmp_path)
    assert len(files) == d["arrays"]
    for k in ("rgb_coarse", "rgb_fine", "weights_fine", "loss", "param.fine.static_rgb.0.weight", "grad.coarse.static_sigma.0.weight"):
        assert k + ".npy" in files, k
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    assert np.load(tmp_path / "rgb_fine.npy").shape == (1024, 3)
    from nerf_fl_amd import synth
    init = synth.make_field_params(12, "sharp", typ="fine")["static_rgb.0.weight"]
    assert not np.array_equal(np.load(tmp_path / "param.fine.static_rgb.0.weight.npy"), init.numpy())     # after Adam, not before


def test_render_dump(tmp_path):
    out = _bench(["--steps", "2", "--mode", "render", "--dump-outputs", str(tmp_path)])
    files = os.listdir(tmp_path)
    assert out["dump_outputs"]["arrays"] == len(files) and "rgb_fine.npy" in files
    assert not [f for f in files if f.startswith(("param.", "grad."))]
