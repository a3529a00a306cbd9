"""Learnable camera poses and ray generation for `--refine_pose` training (the callers either side of
render_rays when poses are optimised: reference models/poses.py, utils/lie_group_helper.py:50-84,
datasets/ray_utils.py:5-55, train.py:86-98).

`LearnPose.forward`, `make_c2w` and `get_rays` are plain PyTorch: the reference-shaped API and the test oracle.
The training path is `posed_rays`: the same pose -> ray step in two HIP launches (nfl_pose_rays and its backward,
include/nerf_fl_amd.h), graph-capturable, with (r, t) gradients summed in a fixed order (bit-reproducible) and, with a
GradArena, written over the arena's views like every other gradient of the step.
"""
import torch
from torch import nn

__all__ = ["so3_exp", "make_c2w", "LearnPose", "get_ray_directions", "get_rays", "posed_rays", "row_table"]


def _skew(v):
    z = torch.zeros_like(v[..., 0])
    return torch.stack([torch.stack([z, -v[..., 2], v[..., 1]], -1),
                        torch.stack([v[..., 2], z, -v[..., 0]], -1),
                        torch.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def so3_exp(r):
    """Rodrigues: axis-angle (..., 3) -> rotation (..., 3, 3), with the reference's +1e-15 in the norm
    (lie_group_helper.py:63-72)."""
    K = _skew(r)
    n = r.norm(dim=-1) + 1e-15
    a = (torch.sin(n) / n)[..., None, None]
    b = ((1 - torch.cos(n)) / n ** 2)[..., None, None]
    eye = torch.eye(3, dtype=r.dtype, device=r.device).expand(K.shape)
    return eye + a * K + b * (K @ K)


def make_c2w(r, t):
    """(..., 3), (..., 3) -> (..., 4, 4) (lie_group_helper.py:75-84)."""
    top = torch.cat([so3_exp(r), t[..., None]], -1)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=r.dtype, device=r.device).expand(*top.shape[:-2], 1, 4)
    return torch.cat([top, bottom], -2)


class LearnPose(nn.Module):
    """Per-camera (r, t) delta composed with the initial pose (reference models/poses.py:9-34);
    `forward(cam_id)` accepts a scalar id (reference behaviour) or a tensor of ids (batched)."""

    def __init__(self, num_cams, learn_R, learn_t, init_c2w=None):
        super().__init__()
        self.num_cams = num_cams
        self.init_c2w = nn.Parameter(init_c2w, requires_grad=False) if init_c2w is not None else None
        self.r = nn.Parameter(torch.zeros(num_cams, 3), requires_grad=learn_R)
        self.t = nn.Parameter(torch.zeros(num_cams, 3), requires_grad=learn_t)

    def forward(self, cam_id):
        c2w = make_c2w(self.r[cam_id], self.t[cam_id])
        if self.init_c2w is not None:
            c2w = c2w @ self.init_c2w[cam_id]
        return c2w


def get_ray_directions(H, W, K, device=None):
    """(H, W, 3) camera-frame directions, no half-pixel centring (ray_utils.py:5-26)."""
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=device),
                          torch.arange(W, dtype=torch.float32, device=device), indexing="ij")
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)


def get_rays(directions, c2w):
    """directions (B, 3) camera frame, c2w (B, 3|4, 4) or (3|4, 4) -> unit world directions and origins
    (ray_utils.py:29-55: rotate, normalise, origin = translation column)."""
    if c2w.dim() < 3:
        c2w = c2w[None]
    directions = directions.reshape(-1, 3)
    R, t = c2w[:, :3, :3], c2w[:, :3, 3]
    rays_d = (directions[:, None, :] @ R.transpose(1, 2))[:, 0, :]
    rays_d = rays_d / rays_d.norm(dim=-1, keepdim=True)
    rays_o = t.expand(rays_d.shape)
    return rays_o, rays_d


def row_table(image_ids, device=None):
    """The image id -> pose row table `posed_rays` takes, for poses stored in the order of `image_ids` (the reference's
    `enumerate(poses_dict.keys())`, train.py:84): int64, -1 for ids that have no pose."""
    ids = torch.as_tensor(image_ids, dtype=torch.int64).reshape(-1)
    if ids.numel() and int(ids.min()) < 0:
        raise ValueError("image ids must be >= 0")
    if ids.unique().numel() != ids.numel():
        raise ValueError("image ids must be distinct")
    table = torch.full((int(ids.max()) + 1 if ids.numel() else 0,), -1, dtype=torch.int64)
    table[ids] = torch.arange(ids.numel(), dtype=torch.int64)
    return table.to(device) if device is not None else table


class _PosedRaysFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose, rays_cam, ts, row_of_id, arena, r, t):
        import ctypes as C

        from . import _lib
        from .rendering import _status_word
        dev = rays_cam.device
        a = _lib.PoseArgs()
        init = pose.init_c2w
        keep = [r.detach(), t.detach(), None if init is None else init.detach(), row_of_id, ts, rays_cam]
        a.d_r, a.d_t = keep[0].data_ptr(), keep[1].data_ptr()
        a.d_init_c2w = None if init is None else keep[2].data_ptr()
        a.d_row_of_id, a.d_ts, a.d_rays_cam = row_of_id.data_ptr(), ts.data_ptr(), rays_cam.data_ptr()
        a.n_cams, a.n_ids, a.n_rays, a.cam_stride = r.shape[0], row_of_id.shape[0], rays_cam.shape[0], rays_cam.shape[1]
        out = torch.empty(rays_cam.shape[0], 8, dtype=torch.float32, device=dev)
        rows = torch.empty(rays_cam.shape[0], dtype=torch.int32, device=dev)
        a.d_rays, a.d_rows, a.d_status = out.data_ptr(), rows.data_ptr(), _status_word(dev).data_ptr()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().nfl_pose_rays(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "nfl_pose_rays")
        ctx.args, ctx.keep, ctx.rows, ctx.arena, ctx.rt = a, keep, rows, arena, (r, t)
        ctx.mark_non_differentiable(rows)
        return out, rows

    @staticmethod
    def backward(ctx, g_rays, _g_rows):
        import ctypes as C

        from . import _lib
        r, t = ctx.rt
        want_r, want_t = ctx.needs_input_grad[5], ctx.needs_input_grad[6]
        if g_rays is None or not (want_r or want_t):
            return None, None, None, None, None, None, None
        g_rays = g_rays.to(torch.float32).contiguous()
        arena = ctx.arena

        def target(p, want):
            if not want:
                return None, False
            v = arena.view(p) if arena is not None else None
            return (v, True) if v is not None else (torch.empty_like(p), False)

        (g_r, r_in_arena), (g_t, t_in_arena) = target(r, want_r), target(t, want_t)
        a = ctx.args
        a.d_g_rays = g_rays.data_ptr()
        a.d_g_r = None if g_r is None else g_r.data_ptr()
        a.d_g_t = None if g_t is None else g_t.data_ptr()
        with torch.cuda.device(g_rays.device):
            _lib.check(_lib.lib().nfl_pose_rays_backward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "nfl_pose_rays_backward")
        if arena is not None:
            arena.attach()
        return (None, None, None, None, None, None if r_in_arena else g_r, None if t_in_arena else g_t)


def posed_rays(pose, rays_cam, ts, row_of_id, grad_arena=None):
    """Camera-frame rays -> world rays through the learnable poses, in HIP (nfl_pose_rays): the reference's
    `learn_poses(i)` -> `get_rays` -> `cat([o, d, near, far])` of train.py:86-98, for a whole batch in one launch.

    pose: LearnPose (r, t of shape (C, 3), optional init_c2w (C, 4, 4)); rays_cam (R, >= 5) fp32: camera-frame direction,
    near, far (further columns are ignored); ts (R,) image ids; row_of_id: int64 device table image id -> pose row
    (`row_table`).  Returns (R, 8) = origin, unit direction, near, far, differentiable w.r.t. pose.r / pose.t.
    An id without a pose gives a NaN ray and sets NFL_STATUS_POSE_ID in the status word `check_status()` reads.
    With a `grad_arena` holding pose.r / pose.t the backward WRITES their arena views (overwrite, as every gradient of the
    step); otherwise it returns fresh tensors for autograd to accumulate."""
    if not (isinstance(rays_cam, torch.Tensor) and rays_cam.is_cuda):
        raise RuntimeError("nerf_fl_amd.poses.posed_rays: device tensors only (this build has no CPU path)")
    if rays_cam.dim() != 2 or rays_cam.shape[1] < 5 or rays_cam.dtype != torch.float32:
        raise ValueError("rays_cam must be fp32 (R, >= 5): camera-frame direction, near, far")
    r, t = pose.r, pose.t
    dev = rays_cam.device
    for name, x in (("pose.r", r), ("pose.t", t)):
        if x.device != dev or x.dtype != torch.float32 or tuple(x.shape) != (pose.num_cams, 3) or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp32 ({pose.num_cams}, 3) tensor on {dev}")
    init = pose.init_c2w
    if init is not None and (init.device != dev or init.dtype != torch.float32 or tuple(init.shape) != (pose.num_cams, 4, 4)
                             or not init.is_contiguous()):
        raise ValueError(f"pose.init_c2w must be a contiguous fp32 ({pose.num_cams}, 4, 4) tensor on {dev}")
    if row_of_id.device != dev or row_of_id.dtype != torch.int64 or row_of_id.dim() != 1 or not row_of_id.is_contiguous():
        raise ValueError("row_of_id must be a contiguous int64 (n_ids,) tensor on the rays' device (poses.row_table)")
    rays_cam = rays_cam.detach().contiguous()
    ts = ts.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    if ts.shape[0] != rays_cam.shape[0]:
        raise ValueError(f"ts must be ({rays_cam.shape[0]},)")
    out, _ = _PosedRaysFn.apply(pose, rays_cam, ts, row_of_id, grad_arena, r, t)
    return out
