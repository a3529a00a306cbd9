"""RayTrainer(refine_pose=True): the reference's --refine_pose training (LearnPose deltas -> world rays -> BARF-encoded
render -> NerfWLoss -> one Adam over fields and poses) on the HIP pose kernels, eager and graph-captured."""
import ctypes as C
import math
import os

import pytest
import torch

import gpu_util
from nerf_fl_amd.poses import LearnPose, get_ray_directions, get_rays
from nerf_fl_amd.train import Adam, RayTrainer
from oracle import nerfw_oracle as orc

pytestmark = pytest.mark.gpu
DEV = gpu_util.DEV
GTOL = 1e-2                      # the end-to-end pose-gradient tolerance of tests/test_grad_variants_gpu.py
IMAGE_IDS = [5, 2, 9]            # pose row -> image id (the reference's enumerate(poses_dict.keys()))
S = I = 32


def _scene(n_per_cam=24, width=7):
    """Three cameras ~4 from the origin looking down -z, `n_per_cam` pixels each, interleaved; the fork's training layout
    (camera-frame direction, near, far, one extra column) and the image id of every ray."""
    Kmat = torch.tensor([[7.0, 0, 3.0], [0, 7.0, 3.0], [0, 0, 1]])
    dirs = get_ray_directions(width, width, Kmat).reshape(-1, 3)[:n_per_cam]
    init = torch.eye(4)[None].repeat(3, 1, 1)
    init[:, :3, 3] = torch.tensor([[0.1, -0.1, 4.0], [0.3, 0.2, 4.2], [-0.2, 0.1, 3.9]])
    row = torch.arange(3 * n_per_cam) % 3
    cam_dirs = dirs[torch.arange(3 * n_per_cam) // 3]
    extra = torch.randn(3 * n_per_cam, 1, generator=torch.Generator().manual_seed(4))
    rays_cam = torch.cat([cam_dirs, torch.tensor([2.0, 6.0]).expand(3 * n_per_cam, 2), extra], 1)
    ts = torch.tensor(IMAGE_IDS)[row]
    target = torch.rand(3 * n_per_cam, 3, generator=torch.Generator().manual_seed(3))
    return init, row, rays_cam, ts, target


DELTA_R = torch.tensor([[0.02, -0.01, 0.03], [-0.02, 0.01, 0.0], [0.0, 0.0, 0.0]])
DELTA_T = torch.tensor([[0.01, 0.0, -0.02], [0.0, 0.02, 0.01], [0.0, 0.0, 0.0]])


def _trainer(init, P_c, P_f, lr=5e-4, **kw):
    tr = RayTrainer(DEV, N_samples=S, N_importance=I, perturb=0.0, noise_std=0.0, white_back=True, lr=lr,
                    batch_size=kw.pop("batch_size", 72), refine_pose=True, init_c2w=init, image_ids=IMAGE_IDS,
                    N_vocab=16, **kw)
    tr.models["coarse"].load_state_dict(P_c)
    tr.models["fine"].load_state_dict(P_f)
    with torch.no_grad():
        tr.pose.r.copy_(DELTA_R)
        tr.pose.t.copy_(DELTA_T)
    return tr


def _fields():
    spec_c, spec_f = orc.FieldSpec("coarse"), orc.FieldSpec("fine")
    return spec_c, orc.make_field_params(spec_c, 71, "sharp"), spec_f, orc.make_field_params(spec_f, 72, "sharp")


def test_first_step_pose_gradients_match_the_oracle():
    """(a) at epoch 6, where the BARF weights are fractional"""
    spec_c, P_c, spec_f, P_f = _fields()
    init, row, rays_cam, ts, target = _scene()
    epoch = 6
    pose_o = LearnPose(3, True, True, init_c2w=init)
    with torch.no_grad():
        pose_o.r.copy_(DELTA_R)
        pose_o.t.copy_(DELTA_T)
    o, d = get_rays(rays_cam[:, :3], pose_o(row))
    rays = torch.cat([o, d, rays_cam[:, 3:5]], 1)
    res = orc.render_rays(spec_c, P_c, spec_f, P_f, rays, n_samples=S, n_importance=I, noise_std=0.0, white_back=True,
                          pe_w_xyz=orc.barf_weights(10, epoch), pe_w_dir=orc.barf_weights(4, epoch))
    sum(orc.nerfw_loss(res, target).values()).backward()

    tr = _trainer(init, P_c, P_f)
    tr.current_epoch = epoch
    tr.step(rays_cam.to(DEV), target.to(DEV), ts.to(DEV))
    for name in ("r", "t"):
        g_h, g_o = getattr(tr.pose, name).grad.cpu(), getattr(pose_o, name).grad
        assert g_o.abs().max() > 0
        err = (g_h - g_o).abs().max().item() / g_o.abs().max().item()
        print(f"first-step d{name}: max err / max|g| = {err:.2e}")
        assert err <= GTOL, (name, g_h, g_o)


def test_pose_gradients_do_not_accumulate_across_steps():
    """(b) the second step's pose gradient is a fresh one, not the sum of both steps"""
    _, P_c, _, P_f = _fields()
    init, _, rays_cam, ts, target = _scene()
    tr = _trainer(init, P_c, P_f, lr=0.0)             # lr 0: the second step sees the same parameters
    tr.current_epoch = 6
    args = (rays_cam.to(DEV), target.to(DEV), ts.to(DEV))
    tr.step(*args)
    g1 = (tr.pose.r.grad.clone(), tr.pose.t.grad.clone())
    tr.step(*args)
    for g_first, g_second in zip(g1, (tr.pose.r.grad, tr.pose.t.grad)):
        scale = g_first.abs().max().item()
        assert scale > 0
        assert (g_second - g_first).abs().max().item() <= 1e-3 * scale
    assert tr.pose.r.grad is tr.arena.view(tr.pose.r)


def test_graphed_replays_follow_the_epoch():
    """(c) replays of the captured step read the BARF buffers refilled between them: same loss and pose gradients as an
    eager step on the same batch (lr 0, perturb 0, noise 0: no parameter change, no random draw)"""
    _, P_c, _, P_f = _fields()
    init, _, rays_cam, ts, target = _scene()
    tr = _trainer(init, P_c, P_f, lr=0.0, use_graph=True)
    args = (rays_cam.to(DEV), target.to(DEV), ts.to(DEV))
    tr.current_epoch = 5
    gs = tr.graphed_step(args[0], args[2], args[1])
    losses = []
    for epoch in (5, 6, 9):
        tr.current_epoch = epoch
        tr._sync_barf()
        gs.load(args[0], args[2], args[1])
        loss_g = gs.replay()[0].item()
        g_graph = (tr.pose.r.grad.clone(), tr.pose.t.grad.clone())
        loss_e = tr.step(*args)[0].item()
        assert abs(loss_g - loss_e) <= 1e-6 * abs(loss_e), (epoch, loss_g, loss_e)
        for a, b in zip(g_graph, (tr.pose.r.grad, tr.pose.t.grad)):
            assert (a - b).abs().max().item() <= 1e-3 * b.abs().max().item(), epoch
        losses.append(loss_e)
    assert len(set(losses)) == 3, losses              # the epochs' weights differ, so the replays did follow them


def _graph_nodes(graph_ptr):
    import torch as _t
    path = os.path.join(os.path.dirname(_t.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipGraphChildGraphNodeGetGraph.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    types = []

    def walk(g):
        n = C.c_size_t(0)
        assert hip.hipGraphGetNodes(C.c_void_p(g), None, C.byref(n)) == 0
        nodes = (C.c_void_p * n.value)()
        assert hip.hipGraphGetNodes(C.c_void_p(g), nodes, C.byref(n)) == 0
        for node in nodes:
            ty = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(ty)) == 0
            types.append(ty.value)
            if ty.value == 4:                               # hipGraphNodeTypeGraph: walk the child graph
                child = C.c_void_p()
                assert hip.hipGraphChildGraphNodeGetGraph(C.c_void_p(node), C.byref(child)) == 0
                walk(child.value)

    walk(graph_ptr)
    return types


def test_captured_step_has_no_memset_or_memcpy_node():
    """(d) NeRF-W fields + poses: the whole captured step is kernels (a memset node ran out of order under a second
    process; host -> device copies would freeze the BARF weights / make_c2w's constant row)"""
    init, _, rays_cam, ts, target = _scene()
    tr = RayTrainer(DEV, N_samples=S, N_importance=I, encode_a=True, encode_t=True, N_vocab=16, batch_size=72,
                    refine_pose=True, init_c2w=init, image_ids=IMAGE_IDS, use_graph=True)
    tr.current_epoch = 6
    gs = tr.graphed_step(rays_cam.to(DEV), ts.to(DEV), target.to(DEV), keep_graph=True)
    types = _graph_nodes(gs.graph.raw_cuda_graph())
    print(f"captured step: {len(types)} nodes, types {sorted(set(types))}")
    assert types.count(0) >= 10                               # kernels
    bad = [t for t in types if t in (1, 2, 12, 13)]           # memcpy, memset, memcpy from / to symbol
    assert not bad, bad
    loss, _ = gs.replay()
    assert math.isfinite(loss.item())


def _look_at(centres):
    """camera-to-world (C, 4, 4) for cameras at `centres` looking at the origin (camera -z forward, +y up)"""
    out = torch.eye(4).repeat(len(centres), 1, 1)
    for k, p in enumerate(centres):
        z = p / p.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z)
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        out[k, :3, :3] = torch.stack([x, y, z], 1)
        out[k, :3, 3] = p
    return out


def test_pose_recovery_on_a_frozen_trained_field():
    """(e) targets rendered at the true poses by the reference-trained coarse field (tests/golden/w_trained.npz), poses
    started ~2 deg / ~2 % of the camera distance off, poses-only Adam at epoch 10: both errors at most half the start"""
    import golden_util as gu
    P_c = gu.trained_params(orc.FieldSpec("coarse"))
    centres = torch.tensor([[0.0, 0.0, 4.0], [1.2, 0.3, 3.8], [-1.0, 0.8, 3.8], [0.4, -1.1, 3.8]])
    init = _look_at(centres)
    W = 24
    Kmat = torch.tensor([[W / 0.7, 0, W / 2], [0, W / 0.7, W / 2], [0, 0, 1]])
    dirs = get_ray_directions(W, W, Kmat).reshape(-1, 3)
    C_ = len(centres)
    rays_cam = torch.cat([dirs.repeat(C_, 1), torch.tensor([2.0, 6.0]).expand(C_ * W * W, 2)], 1).to(DEV)
    ts = torch.arange(C_).repeat_interleave(W * W).to(DEV)
    tr = RayTrainer(DEV, N_samples=64, N_importance=0, perturb=0.0, noise_std=0.0, white_back=True, batch_size=C_ * W * W,
                    refine_pose=True, init_c2w=init)
    tr.models["coarse"].load_state_dict(P_c)
    tr.current_epoch = 10
    from nerf_fl_amd import render_rays
    from nerf_fl_amd.poses import posed_rays
    tr._sync_barf()
    with torch.no_grad():                                     # targets at the true poses (r = t = 0)
        target = render_rays(tr.models, tr.embeddings, posed_rays(tr.pose, rays_cam, ts, tr.row_of_id), ts, 64, False,
                             0, 0, 0, 32768, True, False, barf_weights=tr.barf_w)["rgb_coarse"].clone()
    g = torch.Generator().manual_seed(11)
    axis = torch.randn(C_, 3, generator=g)
    dirn = torch.randn(C_, 3, generator=g)
    with torch.no_grad():
        tr.pose.r.copy_(axis / axis.norm(dim=-1, keepdim=True) * math.radians(2.0))
        tr.pose.t.copy_(dirn / dirn.norm(dim=-1, keepdim=True) * 0.02 * 4.0)

    def errors():
        with torch.no_grad():
            c2w = tr.c2w(torch.arange(C_))
            rot = torch.stack([torch.arccos(((torch.trace(c2w[k, :, :3] @ init[k, :3, :3].T.to(DEV)) - 1) / 2).clamp(-1, 1))
                               for k in range(C_)])
            tra = (c2w[:, :, 3] - init[:, :3, 3].to(DEV)).norm(dim=-1)
        return rot.mean().item(), tra.mean().item()

    rot0, tra0 = errors()
    tr.opt = Adam([tr.pose.r, tr.pose.t], lr=1e-3, eps=1e-8)   # the field stays frozen: only the poses are optimised
    field = [p.detach().clone() for p in tr.models["coarse"].parameters()]
    for _ in range(300):
        tr.step(rays_cam, target, ts)
    rot1, tra1 = errors()
    print(f"pose recovery: rotation {math.degrees(rot0):.3f} -> {math.degrees(rot1):.3f} deg (ratio {rot1 / rot0:.3f}), "
          f"camera centre {tra0:.4f} -> {tra1:.4f} (ratio {tra1 / tra0:.3f})")
    assert all(torch.equal(a, b) for a, b in zip(field, tr.models["coarse"].parameters()))
    assert rot1 <= 0.5 * rot0 and tra1 <= 0.5 * tra0


def test_checkpoint_round_trip_with_learn_poses_keys(tmp_path):
    """(f) learn_poses.r / .t / .init_c2w, as in a Lightning checkpoint of the reference"""
    _, P_c, _, P_f = _fields()
    init, _, _, _, _ = _scene()
    tr = _trainer(init, P_c, P_f)
    sd = tr.state_dict()
    assert {"learn_poses.r", "learn_poses.t", "learn_poses.init_c2w"} <= set(sd)
    path = os.path.join(tmp_path, "ckpt", "last.ckpt")
    tr.save(path)
    tr2 = RayTrainer(DEV, N_samples=S, N_importance=I, refine_pose=True, init_c2w=torch.eye(4).repeat(3, 1, 1),
                     image_ids=IMAGE_IDS, N_vocab=16)
    tr2.load(path)
    for k, v in tr2.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    assert torch.equal(tr2.c2w([0, 1, 2]).cpu(), tr.c2w([0, 1, 2]).cpu())
    ref = LearnPose(3, True, True, init_c2w=init)
    ref.load_state_dict({k[len("learn_poses."):]: v.cpu() for k, v in sd.items() if k.startswith("learn_poses.")})
    with torch.no_grad():
        assert torch.allclose(tr.c2w([2, 0]).cpu(), ref(torch.tensor([2, 0]))[:, :3], atol=1e-6)
