"""CPU side of the trainer's run state: parallel.broadcast_tensors_ over gloo at world size 2 and 4, the parameter order a
reference Lightning checkpoint's optimiser state is indexed by (pinned by a fixture written from the reference's own
modules and get_parameters), rank_seed and the warm-up scheduler's state dict."""
import io
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

from nerf_fl_amd import parallel
from nerf_fl_amd.nerf import NeRF
from nerf_fl_amd.poses import LearnPose
from nerf_fl_amd.train import make_scheduler, rank_seed, reference_parameter_names

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_ref_param_order.json")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tensors(rank):
    """Mixed fp32 / int32, awkward sizes, a non-contiguous one; different values on every rank."""
    g = torch.Generator().manual_seed(100 + rank)
    return [nn.Parameter(torch.randn(5, 3, generator=g)), torch.randint(-9, 9, (7,), generator=g, dtype=torch.int32),
            torch.randn(4, 6, generator=g).t(), torch.randn(1, generator=g),
            torch.randint(0, 100, (2, 2), generator=g, dtype=torch.int32), torch.zeros(0)]


def _bcast_worker(rank, world, port, src, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ts = _tensors(rank)
    ptrs, versions = [t.data_ptr() for t in ts], [t._version for t in ts]
    calls = []
    real = dist.broadcast

    def counting(tensor, *a, **k):
        calls.append(tensor.dtype)
        return real(tensor, *a, **k)

    dist.broadcast = counting
    try:
        parallel.broadcast_tensors_(ts, src=src)
    finally:
        dist.broadcast = real
    out[rank] = dict(values=[t.detach().clone() for t in ts], calls=[str(c) for c in calls],
                     same_storage=[t.data_ptr() == p for t, p in zip(ts, ptrs)],
                     moved=[t._version > v for t, v in zip(ts, versions)], grad=ts[0].requires_grad)
    dist.destroy_process_group()


@pytest.mark.parametrize("world,src", [(2, 0), (4, 2)])
def test_broadcast_tensors_world(world, src):
    out = mp.Manager().dict()
    mp.spawn(_bcast_worker, args=(world, _free_port(), src, out), nprocs=world, join=True)
    expect = _tensors(src)
    for r in range(world):
        o = out[r]
        assert all(torch.equal(a, b.detach()) and a.dtype == b.dtype for a, b in zip(o["values"], expect)), r
        assert sorted(o["calls"]) == ["torch.float32", "torch.int32"], o["calls"]      # one collective per dtype
        assert all(o["same_storage"]) and o["grad"]                                     # in place, still a Parameter
        if r != src:
            assert all(o["moved"][:5]), o["moved"]     # every destination's version counter moved (render_rays re-packs)


def test_broadcast_tensors_without_a_process_group_is_a_noop():
    assert not dist.is_initialized()
    ts = _tensors(3)
    before = [(t.detach().clone(), t._version) for t in ts]
    parallel.broadcast_tensors_(ts)
    parallel.broadcast_tensors_([])
    assert all(torch.equal(t, b) and t._version == v for t, (b, v) in zip(ts, before))


def _modules(cfg, n):
    """RayTrainer's `modules` for a configuration (same constructors, same prefixes), on the CPU."""
    ms = {}
    if cfg["encode_a"]:
        ms["embedding_a"] = nn.Embedding(n["N_vocab"], n["N_a"])
    if cfg["encode_t"]:
        ms["embedding_t"] = nn.Embedding(n["N_vocab"], n["N_tau"])
    cx, cd = 6 * n["N_emb_xyz"] + 3, 6 * n["N_emb_dir"] + 3
    ms["nerf_coarse"] = NeRF("coarse", in_channels_xyz=cx, in_channels_dir=cd, refine_pose=cfg["refine_pose"])
    if cfg["N_importance"] > 0:
        ms["nerf_fine"] = NeRF("fine", in_channels_xyz=cx, in_channels_dir=cd, encode_appearance=cfg["encode_a"],
                               in_channels_a=n["N_a"], encode_transient=cfg["encode_t"], in_channels_t=n["N_tau"],
                               refine_pose=cfg["refine_pose"])
    if cfg["refine_pose"]:
        ms["learn_poses"] = LearnPose(n["n_cams"], True, True, torch.eye(4).repeat(n["n_cams"], 1, 1))
    return ms


with open(GOLDEN) as _f:
    _FIX = json.load(_f)


@pytest.mark.parametrize("name", sorted(_FIX["configs"]))
def test_reference_parameter_order(name):
    """The names resume() assumes for a reference checkpoint's optimiser positions are the reference's own, shapes
    included; and the trainable ones, in that order, are RayTrainer.params' order."""
    cfg, n = _FIX["configs"][name], _FIX["settings"]
    ms = _modules(cfg, n)
    names = reference_parameter_names(ms)
    assert names == [p[0] for p in cfg["params"]]
    params = dict((f"{k}.{pn}", p) for k, m in ms.items() for pn, p in m.named_parameters())
    for pname, shape, _trainable in cfg["params"]:
        if pname in params:
            assert list(params[pname].shape) == shape, pname
        else:
            assert pname.startswith("learn_poses.") and not cfg["refine_pose"]
    ref_trainable = [p[0] for p in cfg["params"] if p[2]]
    ours = [f"{k}.{pn}" for k, m in ms.items() for pn, p in m.named_parameters() if p.requires_grad]
    assert ours == ref_trainable


def test_rank_seed_differs_per_rank_and_epoch():
    seeds = {rank_seed(s, r, e) for s in (0, 1, 7) for r in range(16) for e in range(4)}
    assert len(seeds) == 3 * 16 * 4
    assert all(0 <= x < 2 ** 63 for x in seeds)


@pytest.mark.parametrize("sched", ["cosine", "steplr", "poly"])
def test_warmup_scheduler_state_loads_weights_only(sched):
    """The warm-up wrapper's state dict holds values only (the follower as a state dict), so a checkpoint with it loads
    with weights_only=True, and the loaded schedule continues with the same rates."""
    def make():
        p = nn.Parameter(torch.zeros(3))
        opt = torch.optim.Adam([p], lr=1e-3)
        return opt, make_scheduler(opt, sched, num_epochs=6, decay_step=(3,), warmup_epochs=2, warmup_multiplier=2.0)

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o1, s1 = make()
        for _ in range(3):
            s1.step()
        buf = io.BytesIO()
        torch.save({"s": s1.state_dict(), "o": o1.state_dict()}, buf)
        buf.seek(0)
        ck = torch.load(buf, weights_only=True)
        o2, s2 = make()
        o2.load_state_dict(ck["o"])
        s2.load_state_dict(ck["s"])
        for _ in range(4):
            s1.step()
            s2.step()
            assert o1.param_groups[0]["lr"] == o2.param_groups[0]["lr"]
