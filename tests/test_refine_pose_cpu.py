"""CPU side of --refine_pose: the pose kernels' status bit and argument checks (nfl_pose_args and the signatures are held to
the header in tests/test_abi_cpu.py), the id -> row table, the BARF buffer helper and RayTrainer's refine_pose argument
checks (which run before it asks for a device)."""
import ctypes as C

import pytest
import torch

from nerf_fl_amd import BarfPosEmbedding, _lib
from nerf_fl_amd.poses import row_table
from nerf_fl_amd.rendering import fill_barf_weights
from nerf_fl_amd.train import RayTrainer


def test_pose_status_bit_is_its_own():
    assert not _lib.NFL_STATUS_POSE_ID & (_lib.NFL_STATUS_RANGE | _lib.NFL_STATUS_NONFINITE)


def test_pose_entry_points_reject_bad_arguments_without_a_device():
    L = _lib.lib()
    a = _lib.PoseArgs()
    a.n_cams, a.n_ids, a.n_rays, a.cam_stride = 2, 2, 4, 5
    assert L.nfl_pose_rays(C.byref(a), None) == -1                 # NULL inputs
    assert L.nfl_pose_rays_backward(C.byref(a), None) == -1
    a.n_rays, a.cam_stride = 0, 4
    assert L.nfl_pose_rays(C.byref(a), None) == -1                 # fewer than 5 camera-frame columns


def test_row_table():
    tab = row_table([5, 2, 9])
    assert tab.dtype == torch.int64 and tab.tolist() == [-1, -1, 1, -1, -1, 0, -1, -1, -1, 2]
    assert row_table(range(4)).tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        row_table([1, 1])
    with pytest.raises(ValueError):
        row_table([-1, 0])


@pytest.mark.parametrize("epoch", [0, 4, 5, 6, 8, 9, 30])
def test_fill_barf_weights_matches_the_embedding(epoch):
    emb = {"xyz": BarfPosEmbedding(9, 10, 4, 8), "dir": BarfPosEmbedding(3, 4, 4, 8)}
    bufs = (torch.full((10,), float("nan")), torch.full((4,), float("nan")))
    out = fill_barf_weights(emb, epoch, bufs)
    assert out[0] is bufs[0] and out[1] is bufs[1]                  # in place
    assert torch.equal(bufs[0], emb["xyz"].weights(epoch)) and torch.equal(bufs[1], emb["dir"].weights(epoch))


def test_trainer_refine_pose_arguments_are_checked_before_the_device():
    eye = torch.eye(4).repeat(3, 1, 1)
    with pytest.raises(ValueError, match="refine_pose"):
        RayTrainer("cpu", init_c2w=eye)                             # poses without refine_pose
    with pytest.raises(ValueError, match="refine_pose"):
        RayTrainer("cpu", image_ids=[0, 1, 2])
    with pytest.raises(ValueError, match="init_c2w"):
        RayTrainer("cpu", refine_pose=True, init_c2w=torch.eye(4).repeat(3, 1, 1)[:, :2])
    with pytest.raises(ValueError, match="image_ids"):
        RayTrainer("cpu", refine_pose=True, init_c2w=eye, image_ids=[0, 1])
    with pytest.raises(ValueError, match="distinct"):
        RayTrainer("cpu", refine_pose=True, init_c2w=eye, image_ids=[0, 1, 1])
    with pytest.raises(ValueError, match=">= 0"):
        RayTrainer("cpu", refine_pose=True, image_ids=[-1, 1, 2])
    for kw in (dict(), dict(refine_pose=True, init_c2w=eye[:, :3]), dict(refine_pose=True, image_ids=[4, 7])):
        with pytest.raises(RuntimeError, match="ROCm device"):      # valid arguments: only the device is missing
            RayTrainer("cpu", **kw)
