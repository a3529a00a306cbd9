"""nfl_gather_batch / ImageBank / RayTrainer.fit_epoch(bank) on the device: the kernel against the reference's fixtures
(tests/golden/make_data_golden.py) with the CPU bounds of test_data_cpu.py, against nfl_gen_rays bit for bit, against the
numpy restatement of the permutation, and training from a bank against training from the materialised tensors."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import data_util as du

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _data():
    from nerf_fl_amd import data
    return data


def _photo_bank():
    g, kw = du.photo_inputs()
    return g, _data().ImageBank(**kw, device=DEV)


@pytest.mark.parametrize("tag,pert", [("plain", ()), ("pert", ("color", "occ"))])
def test_gather_small_blender_scene(tag, pert):
    g = du.golden("g23_data_small.npz")
    bank = _data().ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), pert, device=DEV)
    rays, rgbs, ts = bank.materialise()
    ref = torch.from_numpy(g[f"rays_{tag}"])
    assert torch.equal(rgbs.cpu(), torch.from_numpy(g[f"rgbs_{tag}"]))
    assert torch.equal(ts.cpu(), ref[:, 8].long())
    print("small", tag, "max ray err", du.check_rays(rays, ref[:, :8]))


def test_gather_800_blender_scene_with_color_and_occluders():
    g = du.golden("g23_data_big.npz")
    bank = _data().ImageBank.from_blender(du.SCENE, "train", (800, 800), ("color", "occ"), device=DEV)
    rays, rgbs, ts = bank.materialise()
    rows = torch.from_numpy(g["rows"]).to(DEV)
    assert torch.equal(rgbs[rows].cpu(), torch.from_numpy(g["rgbs"]))
    assert torch.equal(ts[rows].cpu(), torch.from_numpy(g["rays"][:, 8]).long())
    print("big max ray err", du.check_rays(rays[rows], torch.from_numpy(g["rays"][:, :8])))


@pytest.mark.parametrize("layout,key", [("camera", "cam_rows"), ("world", "world_rows")])
def test_gather_unequal_rgb_images(layout, key):
    g, bank = _photo_bank()
    rays, rgbs, ts = bank.materialise(layout)
    assert rays.shape == (bank.n_pixels, 5 if layout == "camera" else 8)
    assert torch.equal(rgbs.cpu(), torch.from_numpy(g["rgbs"]))
    assert torch.equal(ts.cpu(), torch.from_numpy(g["cam_rows"][:, 5]).long())
    ref = torch.from_numpy(g[key])
    du.check_rays(rays, ref[:, :5] if layout == "camera" else ref, layout)


def test_camera_layout_of_rgba_images():
    """RGBA pixels and the camera layout together: rows against the restatement on the bank's own host arrays."""
    data = _data()
    host = data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), ("color",))
    exp = du.expected_rows(host.host_table, host.host_pixels, np.arange(host.n_pixels), "camera")
    bank = data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), ("color",), device=DEV)
    rays, rgbs, ts = bank.materialise("camera")
    assert torch.equal(rgbs.cpu(), exp[1]) and torch.equal(ts.cpu(), exp[2])
    du.check_rays(rays, exp[0], "camera")


def test_frame_rays_equal_gen_rays_bit_for_bit():
    from nerf_fl_amd import eval as ev
    g, bank = _photo_bank()
    off = 0
    for i, (h, w) in enumerate(g["sizes"]):
        rays, rgbs, ts = bank.frame(i)
        exp = ev.frame_rays(torch.from_numpy(g["c2w"][i]), torch.from_numpy(g["K"][i]), int(h), int(w), g["near"][i],
                            g["far"][i], DEV)
        assert torch.equal(rays, exp)
        assert torch.equal(rgbs.cpu(), torch.from_numpy(g["rgbs"][off:off + h * w])) and (ts == int(g["ids"][i])).all()
        cam = bank.frame(i, "camera")[0]
        du.check_rays(cam, torch.from_numpy(g["cam_rows"][off:off + h * w, :5]), "camera")
        off += h * w


@pytest.mark.parametrize("key", [1, 0x9E3779B97F4A7C15, 2 ** 64 - 1])
def test_keyed_order_equals_the_restatement(key):
    g, bank = _photo_bank()
    n = bank.n_pixels
    full = bank.materialise()
    for start, count in ((0, n), (100, 517), (n - 1, 1)):
        q = torch.from_numpy(du.perm(key, n, np.arange(start, start + count))).to(DEV)
        got = bank.gather(start, count, key)
        for a, b in zip(got, full):
            assert torch.equal(a, b[q])
    # a larger, equal-size bank (n = 3 * 576, and the 800 x 800 one below 2^21)
    big = _data().ImageBank.from_blender(du.SCENE, "train", (800, 800), (), device=DEV)
    ts = big.gather(0, big.n_pixels, key, out=(None, None, torch.empty(big.n_pixels, dtype=torch.int64, device=DEV)))[2]
    q = du.perm(key, big.n_pixels, np.arange(big.n_pixels))
    assert np.array_equal(ts.cpu().numpy(), q // 640000)


def test_out_buffers_null_outputs_and_ranges_across_images():
    g, bank = _photo_bank()
    host = _data().ImageBank(**du.photo_inputs()[1])
    sizes = g["sizes"][:, 0] * g["sizes"][:, 1]
    start, count = int(sizes[0]) - 150, 150 + int(sizes[1]) + 60          # from the middle of image 0 into image 2
    exp = du.expected_rows(host.host_table, host.host_pixels, np.arange(start, start + count))
    assert len(set(exp[2].tolist())) == 3
    pad = 37
    out = (torch.full((count + pad, 8), -7.0, device=DEV), torch.full((count + pad, 3), -7.0, device=DEV),
           torch.full((count + pad,), -7, dtype=torch.int64, device=DEV))
    ptrs = [t.data_ptr() for t in out]
    got = bank.gather(start, count, out=out)
    assert [t.data_ptr() for t in got] == ptrs
    assert torch.equal(out[1][:count].cpu(), exp[1]) and torch.equal(out[2][:count].cpu(), exp[2])
    du.check_rays(out[0][:count], exp[0])
    for t in out:
        assert (t[count:] == -7).all()
    # NULL outputs are skipped: colours only (validation)
    rgb = torch.full((count, 3), -7.0, device=DEV)
    res = bank.gather(start, count, out=(None, rgb, None))
    assert res[0] is None and res[2] is None and torch.equal(rgb.cpu(), exp[1])
    with pytest.raises(ValueError):
        bank.gather(0, 8, out=(torch.empty(4, 8, device=DEV), None, None))      # too few rows
    with pytest.raises(ValueError):
        bank.gather(bank.n_pixels - 4, 8)


def _trainer(graph, seed=3, bs=256):
    from nerf_fl_amd.train import RayTrainer
    return RayTrainer(DEV, N_samples=32, N_importance=32, batch_size=bs, lr=1e-3, seed=seed, use_graph=graph)


def _params(tr):
    return {k: v.detach().clone() for k, v in tr.state_dict().items()}


@pytest.mark.parametrize("graph", [False, True])
def test_fit_epoch_from_a_bank_equals_training_on_materialised_tensors(graph):
    data = _data()
    bank = data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), ("color",), device=DEV)
    n, bs = bank.n_pixels, 256
    steps = n // bs
    assert steps == 6
    a = _trainer(graph)
    before = _params(a)
    a.fit_epoch(bank)
    got = _params(a)
    assert a.global_step == steps and a.current_epoch == 1

    rays, rgbs, ts = bank.materialise()
    key = data.epoch_key(3, 0)
    b = _trainer(graph)
    gs = None
    for s in range(steps):
        q = torch.from_numpy(du.perm(key, n, np.arange(s * bs, (s + 1) * bs))).to(DEV)
        if graph:
            if gs is None:
                gs = b.graphed_step(rays[q], ts[q], rgbs[q])
            gs.load(rays[q], ts[q], rgbs[q])
            gs.replay()
        else:
            b.step(rays[q], rgbs[q], ts[q])
    exp = _params(b)
    assert set(got) == set(exp)
    assert any(not torch.equal(got[k], before[k]) for k in got)
    for k in got:
        assert torch.equal(got[k], exp[k]), k


def test_an_epoch_allocates_nothing_in_proportion_to_the_bank():
    data = _data()
    rng = np.random.default_rng(5)

    def bank_of(n_img):
        imgs = [rng.integers(0, 256, (32, 32, 4), dtype=np.uint8) for _ in range(n_img)]
        c2w = np.tile(np.eye(4)[None, :3], (n_img, 1, 1))
        c2w[:, :, 3] = rng.standard_normal((n_img, 3))
        K = np.array([[40.0, 0, 16], [0, 40.0, 16], [0, 0, 1]])
        return data.ImageBank(imgs, c2w, K, 2.0, 6.0, device=DEV)

    small, large = bank_of(4), bank_of(16)
    assert large.n_pixels == 4 * small.n_pixels
    for b in (small, large):
        assert b.nbytes == b.n_pixels * 4 + b.n_images * data.RECORD.itemsize
        assert b.pixels.numel() * b.pixels.element_size() + b.table.numel() == b.nbytes
    for graph in (False, True):
        tr = _trainer(graph)
        tr.fit_epoch(small)                      # optimiser state, graph capture: once
        peaks = []
        for b in (small, large):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            tr.fit_epoch(b)
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated() - base)
        print("graph" if graph else "eager", "peak above the resident state:", peaks)
        assert peaks[0] == peaks[1], peaks


def test_validate_takes_a_frame():
    data = _data()
    bank = data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), (), device=DEV)
    tr = _trainer(False)
    v = tr.validate(*bank.frame(1))
    assert np.isfinite(v)


# ---- two ranks on the one GPU (as tests/test_trainer_dist_gpu.py) ------------------------------------------------
WORLD = 2


def _worker(rank, world, out):
    import datetime

    import torch.distributed as dist

    from nerf_fl_amd import data
    from nerf_fl_amd.train import RayTrainer
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    bank = data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), ("color",), device=DEV)
    tr = RayTrainer(DEV, N_samples=32, N_importance=32, batch_size=256, lr=1e-3, seed=11)
    seen = []
    real = bank.gather

    def spy(start, count, key=0, layout="world", out=None):
        res = real(start, count, key, layout, out)
        seen.append((int(start), int(count), int(key), res[2].cpu().clone(), res[1].cpu().clone()))
        return res

    bank.gather = spy
    tr.fit_epoch(bank)
    torch.save(dict(seen=seen, params={k: v.detach().cpu() for k, v in tr.state_dict().items()},
                    steps=tr.global_step), os.path.join(out, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_take_disjoint_batches_and_stay_identical(tmp_path):
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
            p.wait(timeout=300)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{logs[r].read_text()[-3000:]}"
    a, b = [torch.load(str(tmp_path / f"rank{r}.pt"), weights_only=False) for r in range(WORLD)]
    n, bs = 3 * 576, 256
    assert a["steps"] == b["steps"] == n // (bs * WORLD) == 3
    key = _data().epoch_key(11, 0)
    starts = sorted(s[0] for s in a["seen"] + b["seen"])
    assert starts == list(range(0, 3 * WORLD * bs, bs))
    for r, res in enumerate((a, b)):
        assert [s[0] for s in res["seen"]] == [(i * WORLD + r) * bs for i in range(3)]
        assert all(s[1] == bs and s[2] == key for s in res["seen"])
    # disjoint pixels: the positions are disjoint and the permutation is a bijection; seen through the image ids and colours
    q = [du.perm(key, n, np.arange(s[0], s[0] + bs)) for s in a["seen"] + b["seen"]]
    assert np.unique(np.concatenate(q)).size == 6 * bs
    for s, qq in zip(a["seen"] + b["seen"], q):
        assert np.array_equal(s[3].numpy(), qq // 576)
    assert set(a["params"]) == set(b["params"]) and all(torch.equal(a["params"][k], b["params"][k]) for k in a["params"])


if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]
    _worker(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
