"""bench.py --dump-outputs on stand-in tensors (no GPU): which arrays a train / render step writes, their dtypes, and
the size budget with its fixed ray sample."""
import argparse
import os

import numpy as np
import pytest
import torch

import bench


def _step(R, seed=0):
    torch.manual_seed(seed)
    models = {"coarse": torch.nn.Linear(4, 3), "fine": torch.nn.Linear(4, 3)}
    emb = {"xyz": None, "dir": None, "a": torch.nn.Embedding(5, 2)}
    for m in list(models.values()) + [emb["a"]]:
        for p in m.parameters():
            p.grad = torch.randn_like(p)
    ray_id = torch.arange(R, dtype=torch.float32)
    res = {"rgb_fine": ray_id[:, None].repeat(1, 3), "weights_fine": ray_id[:, None].repeat(1, 128),
           "_nerfw_terms": torch.rand(4), "_nerfw_loss": torch.rand(()).requires_grad_()}
    return models, emb, res


def _args(**kw):
    return argparse.Namespace(**dict(dict(mode="train", graph=False), **kw))


def test_train_step_dump_holds_result_loss_params_and_grads(tmp_path):
    R = 16
    models, emb, res = _step(R)
    loss = res["_nerfw_loss"] * 2
    info = bench.dump_outputs(str(tmp_path), bench.last_step_outputs(_args(), (res, loss), models, emb, R), R)
    names = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert info["arrays"] == len(names) and info["rays_written"] == R and info["ray_sample_seed"] is None
    for k in ("rgb_fine", "weights_fine", "_nerfw_terms", "_nerfw_loss", "loss", "param.coarse.weight",
              "grad.fine.bias", "param.embedding_a.weight", "grad.embedding_a.weight"):
        assert k in names, k
    for f in os.listdir(tmp_path):
        assert np.load(tmp_path / f).dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "param.coarse.weight.npy"), models["coarse"].weight.detach().numpy())
    assert np.array_equal(np.load(tmp_path / "grad.fine.bias.npy"), models["fine"].bias.grad.numpy())
    assert np.load(tmp_path / "loss.npy") == pytest.approx(float(loss.detach()))
    assert sum(np.load(tmp_path / f).nbytes for f in os.listdir(tmp_path)) == info["bytes"]


def test_render_and_graphed_steps(tmp_path):
    R = 8
    models, emb, res = _step(R)
    bench.dump_outputs(str(tmp_path / "r"), bench.last_step_outputs(_args(mode="render"), res, models, emb, R), R)
    assert not [f for f in os.listdir(tmp_path / "r") if f.startswith(("param.", "grad."))]     # render moves no weights
    last = (torch.tensor(0.5), torch.tensor(21.0, dtype=torch.float64))
    bench.dump_outputs(str(tmp_path / "g"), bench.last_step_outputs(_args(graph=True), last, models, emb, R), R)
    assert np.load(tmp_path / "g" / "psnr.npy").dtype == np.float64
    assert os.path.exists(tmp_path / "g" / "param.fine.weight.npy")


def test_budget_keeps_one_fixed_sample_of_rays(tmp_path, monkeypatch):
    R = 1000
    models, emb, res = _step(R)
    outs = bench.last_step_outputs(_args(mode="render"), res, models, emb, R)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 10)
    a = bench.dump_outputs(str(tmp_path / "a"), outs, R)
    b = bench.dump_outputs(str(tmp_path / "b"), outs, R)
    assert a["bytes"] <= 64 << 10 and 0 < a["rays_written"] < R and a["ray_sample_seed"] is not None
    rows = np.load(tmp_path / "a" / "rgb_fine.npy")[:, 0]
    assert np.all(np.diff(rows) > 0)                                                      # distinct rays, in ray order
    assert np.array_equal(np.load(tmp_path / "a" / "weights_fine.npy")[:, 0], rows)        # the same rays in every array
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))   # and the same on every run
    assert np.load(tmp_path / "a" / "_nerfw_terms.npy").shape == (4,)                     # not per-ray: whole


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    assert bench.parse_args(["--steps", "7"]).steps == 7
