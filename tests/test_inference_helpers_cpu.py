"""The inference layer's shared helpers on CPU tensors (eval._chunks, eval._fill_padded, rendering._capture_mode,
rendering._pe_weights), and where the backward's three argument structs may be instantiated."""
import os
import re

import pytest
import torch

from nerf_fl_amd import BarfPosEmbedding, NeRF, PosEmbedding
from nerf_fl_amd import rendering as rnd
from nerf_fl_amd.eval import _chunks, _fill_padded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_walk_bounds_and_per_ray_kwargs():
    B, chunk = 150, 64
    rays = torch.arange(B * 8, dtype=torch.float32).reshape(B, 8)
    ts = torch.arange(B)
    full, one = torch.arange(B * 5, dtype=torch.float32).reshape(B, 5), torch.tensor([[1.0, 2.0, 3.0]])
    got = list(_chunks(rays, ts, chunk, dict(a_embedded=full, view_dir=one, t_embedded=None)))
    assert [(lo, hi) for lo, hi, *_ in got] == [(0, 64), (64, 128), (128, 150)]
    for lo, hi, r, t, kw in got:
        assert torch.equal(r, rays[lo:hi]) and torch.equal(t, ts[lo:hi])
        assert sorted(kw) == ["a_embedded", "view_dir"]                     # a None entry is dropped
        assert torch.equal(kw["a_embedded"], full[lo:hi])
        assert kw["view_dir"].shape == (hi - lo, 3) and torch.equal(kw["view_dir"], one.expand(hi - lo, 3))
    assert [kw["view_dir"].shape[0] for *_, kw in got] == [64, 64, 22]


def test_chunk_walk_without_ts_and_without_rays():
    rays = torch.zeros(150, 8)
    assert all(t is None and kw == {} for _, _, _, t, kw in _chunks(rays, None, 64))
    assert list(_chunks(rays[:0], None, 64, dict(view_dir=torch.zeros(0, 3)))) == []
    # B == 1: the one row is the whole batch
    (lo, hi, r, t, kw), = _chunks(rays[:1], torch.tensor([7]), 64, dict(view_dir=torch.ones(1, 3)))
    assert (lo, hi, r.shape[0], t.tolist(), kw["view_dir"].shape) == (0, 1, 1, [7], (1, 3))


def test_chunk_walk_slices_camera_rays():
    cam = rnd.CameraRays(torch.eye(4)[:3], torch.eye(3), 10, 15, 2.0, 6.0, "cpu")
    got = [(lo, hi, r.start, r.count, r.cam.pix0) for lo, hi, r, _, _ in _chunks(cam, None, 64)]
    assert got == [(0, 64, 0, 64, 0), (64, 128, 64, 64, 64), (128, 150, 128, 22, 128)]


def test_fill_padded():
    v = torch.arange(12, dtype=torch.float32).reshape(4, 3) + 1
    buf = torch.zeros(4, 3)
    _fill_padded(buf, v, 4)                                 # n equal to the buffer's length
    assert torch.equal(buf, v)
    buf = torch.zeros(7, 3)
    _fill_padded(buf, v, 4)                                 # n < length: the last row is repeated
    assert torch.equal(buf[:4], v) and torch.equal(buf[4:], v[3:].expand(3, 3))
    buf = torch.zeros(7, 3)
    _fill_padded(buf, v[1:2], 1)                            # a 1-row input fills every row
    assert torch.equal(buf, v[1:2].expand(7, 3))
    ids = torch.zeros(5, dtype=torch.long)
    _fill_padded(ids, torch.tensor([3, 9]), 2)              # 1-D: `ts`
    assert ids.tolist() == [3, 9, 9, 9, 9]


def test_capture_mode_follows_the_process_group(monkeypatch):
    import torch.distributed as dist
    assert rnd._capture_mode() == {}
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    assert rnd._capture_mode() == dict(capture_error_mode="thread_local")
    monkeypatch.setattr(dist, "is_available", lambda: False)
    assert rnd._capture_mode() == {}


def test_pe_weights():
    cpu = torch.device("cpu")
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    assert rnd._pe_weights({"coarse": NeRF("coarse")}, emb, dict(current_epoch=3), cpu) == (None, None)
    barf = {"xyz": BarfPosEmbedding(9, 10, 2, 8), "dir": BarfPosEmbedding(3, 4, 2, 8)}
    models = {"coarse": NeRF("coarse", refine_pose=True)}
    with pytest.raises(KeyError, match="current_epoch"):
        rnd._pe_weights(models, barf, {}, cpu)
    w_xyz, w_dir = rnd._pe_weights(models, barf, dict(current_epoch=5), cpu)
    assert torch.equal(w_xyz, rnd._barf_weights(barf["xyz"], 5)) and w_xyz.shape == (10,)
    assert torch.equal(w_dir, rnd._barf_weights(barf["dir"], 5)) and w_dir.shape == (4,)
    own = (torch.ones(10), torch.ones(4))
    got = rnd._pe_weights(models, barf, dict(barf_weights=own, current_epoch=5), cpu)       # the caller's buffers win
    assert got[0].data_ptr() == own[0].data_ptr() and got[1].data_ptr() == own[1].data_ptr()
    with pytest.raises(ValueError, match=re.escape("`barf_weights[1]` must be a 16-byte aligned, contiguous fp32 (4,) tensor on cpu")):
        rnd._pe_weights(models, barf, dict(barf_weights=(torch.ones(10), torch.ones(5))), cpu)
    with pytest.raises(ValueError, match=re.escape("`barf_weights[0]`")):
        rnd._pe_weights(models, barf, dict(barf_weights=(torch.ones(10, dtype=torch.float64), torch.ones(4))), cpu)


def _sources(folder):
    for base, _, names in os.walk(os.path.join(ROOT, folder)):
        for n in names:
            if n.endswith(".py"):
                with open(os.path.join(base, n)) as f:
                    yield os.path.relpath(os.path.join(base, n), ROOT), f.read()


def test_backward_structs_are_instantiated_in_rendering_only():
    pat = re.compile(r"(?<!class )\b(?:CompBwdArgs|DgradArgs|FieldGrads)\(")      # (_lib.py declares them: `class X(`)
    assert sorted(p for p, s in _sources("nerf_fl_amd") if pat.search(s)) == [os.path.join("nerf_fl_amd", "rendering.py")]
    # test_capi_cpu.py checks nfl_mlp_dgrad's own argument validation with a struct of made-up pointers, below any wrapper
    assert [p for p, s in _sources("tests") if pat.search(s)] == [os.path.join("tests", "test_capi_cpu.py")]
    assert len(pat.findall(dict(_sources("nerf_fl_amd"))[os.path.join("nerf_fl_amd", "rendering.py")])) == 3
