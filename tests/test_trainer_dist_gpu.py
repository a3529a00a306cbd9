"""RayTrainer under a process group of two ranks, both on the one GPU over gloo, each rank a fresh child process (as
tests/test_bench_launcher.py starts bench.py's ranks): the ranks are built with DIFFERENT seeds and must still start
from rank 0's weights, draw different random numbers, stay bit-identical through eager and graphed training on
different shards, agree on a sharded validation, write one checkpoint, and come out of resume() identical although only
rank 0 can read the file.  (RCCL with more than one GPU is not exercised: it needs a multi-GPU node.)"""
import os
import socket
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORLD = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, out):
    import datetime

    import torch.distributed as dist

    from nerf_fl_amd import parallel
    from nerf_fl_amd.train import RayTrainer
    from oracle import nerfw_oracle as orc
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    dev = "cuda:0"
    spec = orc.FieldSpec("coarse")
    teacher = orc.make_field_params(spec, 21, "sharp")
    rays, val = orc.make_rays(2048, 31), orc.make_rays(600, 32)
    with torch.no_grad():
        kw = dict(n_samples=48, white_back=True, noise_std=0.0)
        rgb = orc.render_rays(spec, teacher, None, None, rays, **kw)["rgb_coarse"].to(dev)
        vrgb = orc.render_rays(spec, teacher, None, None, val, **kw)["rgb_coarse"].to(dev)
    rays, val = rays.to(dev), val.to(dev)
    ts, vts = torch.zeros(2048, dtype=torch.long, device=dev), torch.zeros(600, dtype=torch.long, device=dev)
    lo, hi = parallel.shard_bounds(2048, rank, world)
    shard = (rays[lo:hi], rgb[lo:hi], ts[lo:hi])
    res = {}
    cpu = lambda tr: {k: v.detach().cpu().clone() for k, v in tr.state_dict().items()}
    for graph in (False, True):
        tag = "graph" if graph else "eager"
        tr = RayTrainer(dev, N_samples=32, N_importance=32, batch_size=256, lr=1e-3, lr_scheduler="cosine",
                        num_epochs=6, seed=10 + 7 * rank, use_graph=graph)
        res[f"{tag}_init"] = cpu(tr)
        if not graph:
            # what render_rays draws first (stratified jitter) and the first permutation, on this rank
            res["draw"] = torch.rand(16, 32, device=dev).cpu()
            res["perm"] = torch.randperm(1024, device=dev, generator=tr.gen).cpu()
        for _ in range(3):
            tr.fit_epoch(*shard)
        res[f"{tag}_fit"] = cpu(tr)
        res[f"{tag}_val_shard"] = tr.validate(val, vrgb, vts, shard=True)
        res[f"{tag}_val_full"] = tr.validate(val, vrgb, vts)
        path = os.path.join(out, f"{tag}_rank{rank}.ckpt")
        tr.save(path, epoch=2)
        tr.fit_epoch(*shard)                     # the run moves on ...
        if rank == 1:
            with torch.no_grad():                # ... and rank 1's replica drifts away
                for p in tr.params:
                    p.add_(0.01)
            tr.opt.param_groups[0]["lr"] = 1.0
        # only rank 0 holds a readable checkpoint (rank 1's path does not exist)
        tr.resume(os.path.join(out, "eager_rank0.ckpt" if not graph else "graph_rank0.ckpt") if rank == 0
                  else os.path.join(out, "missing", "none.ckpt"))
        res[f"{tag}_resumed"] = cpu(tr)
        res[f"{tag}_resumed_opt"] = [t.detach().cpu().clone() for p in tr.params for t in
                                     (tr.opt.state[p]["exp_avg"], tr.opt.state[p]["exp_avg_sq"])]
        res[f"{tag}_resumed_meta"] = (tr.current_epoch, tr.global_step, tr.opt.param_groups[0]["lr"],
                                      [int(tr.opt.state[p]["step"]) for p in tr.params])
        tr.fit_epoch(*shard)
        res[f"{tag}_after"] = cpu(tr)
    torch.save(res, os.path.join(out, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_two_ranks_stay_identical_and_resume(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    logs = [tmp_path / f"rank{r}.log" for r in range(WORLD)]
    procs = []
    try:
        for r in range(WORLD):
            with open(logs[r], "w") as f:
                procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), str(r), str(WORLD),
                                               str(tmp_path)], env=env, stdout=f, stderr=subprocess.STDOUT))
        for p in procs:
            p.wait(timeout=600)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{logs[r].read_text()[-3000:]}"
    res = [torch.load(str(tmp_path / f"rank{r}.pt"), weights_only=False) for r in range(WORLD)]
    a, b = res
    assert not torch.equal(a["draw"], b["draw"]) and not torch.equal(a["perm"], b["perm"])
    for tag in ("eager", "graph"):
        assert _same(a[f"{tag}_init"], b[f"{tag}_init"]), f"{tag}: construction left the replicas apart"
        assert _same(a[f"{tag}_fit"], b[f"{tag}_fit"]), f"{tag}: training moved the replicas apart"
        assert not _same(a[f"{tag}_init"], a[f"{tag}_fit"])
        assert a[f"{tag}_val_shard"] == b[f"{tag}_val_shard"]
        assert abs(a[f"{tag}_val_shard"] - a[f"{tag}_val_full"]) <= 1e-4, (a[f"{tag}_val_shard"], a[f"{tag}_val_full"])
        assert abs(b[f"{tag}_val_full"] - a[f"{tag}_val_full"]) <= 1e-4
        assert (tmp_path / f"{tag}_rank0.ckpt").exists() and not (tmp_path / f"{tag}_rank1.ckpt").exists()
        ck = torch.load(str(tmp_path / f"{tag}_rank0.ckpt"), map_location="cpu", weights_only=True)
        assert ck["nerf_fl_amd"]["world_size"] == WORLD and ck["nerf_fl_amd"]["current_epoch"] == 3
        assert _same(a[f"{tag}_resumed"], b[f"{tag}_resumed"]) and _same(a[f"{tag}_resumed"], a[f"{tag}_fit"])
        assert _same(ck["state_dict"], a[f"{tag}_resumed"])
        assert all(torch.equal(x, y) for x, y in zip(a[f"{tag}_resumed_opt"], b[f"{tag}_resumed_opt"]))
        assert a[f"{tag}_resumed_meta"] == b[f"{tag}_resumed_meta"] and a[f"{tag}_resumed_meta"][0] == 3
        assert _same(a[f"{tag}_after"], b[f"{tag}_after"]), f"{tag}: replicas apart after resuming"


if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]
    _worker(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
