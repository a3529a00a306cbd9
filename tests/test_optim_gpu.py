"""The one-launch SGD / Adam-with-weight-decay / RAdam / Ranger (C ABI nfl_optim_step, nfl_optim_step_dev) on the MI355X:
against torch's optimisers on identical parameters and gradients, captured against eager (bitwise), load_state_dict under
a captured graph, version counters, state-dict interchange, and the captured train step with Ranger."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 14          # RAdam turns rectified at t = 6; Ranger's lookahead syncs at t = 6 and t = 12
SHAPES = [(256, 63), (256,), (3, 128), (1,), (100, 48), (7,)] + [(17, 5)] * 66       # > 64 tensors: two launches


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    import gpu_util
    return [torch.randn(*s, generator=g).to(gpu_util.DEV) for s in SHAPES], g


def _grad(shape, g):
    import gpu_util
    return (torch.randn(*shape, generator=g) * 10.0 ** float(torch.randint(-6, 2, (1,), generator=g))).to(gpu_util.DEV)


class _Lookahead:
    """torch.optim.RAdam + the Lookahead of torch_optimizer 0.3's Ranger, written out: slow = p at state creation; after
    the update of step t (the parameter's own count), t % k == 0: slow += alpha (p - slow), p = slow."""

    def __init__(self, params, lr, wd, alpha=0.5, k=6):
        self.inner = torch.optim.RAdam(params, lr=lr, betas=(0.95, 0.999), eps=1e-8, weight_decay=wd,
                                       decoupled_weight_decay=True)
        self.param_groups = self.inner.param_groups
        self.alpha, self.k = alpha, k
        self.slow = {p: p.detach().clone() for p in params}

    @torch.no_grad()
    def step(self):
        self.inner.step()
        for p in self.slow:
            st = self.inner.state.get(p)
            if p.grad is not None and st and int(st["step"]) % self.k == 0:
                s = self.slow[p]
                s.add_(p - s, alpha=self.alpha)
                p.copy_(s)


def _pair(kind, ref, mine, wd, capturable=False):
    from nerf_fl_amd import train
    if kind == "sgd":
        return (torch.optim.SGD(ref, lr=1e-2, momentum=0.9, weight_decay=wd),
                train.SGD(mine, lr=1e-2, momentum=0.9, weight_decay=wd, capturable=capturable))
    if kind == "sgd0":
        return (torch.optim.SGD(ref, lr=1e-2, weight_decay=wd),
                train.SGD(mine, lr=1e-2, weight_decay=wd, capturable=capturable))
    if kind == "adam":
        return (torch.optim.Adam(ref, lr=5e-4, eps=1e-8, weight_decay=wd),
                train.Adam(mine, lr=5e-4, eps=1e-8, weight_decay=wd, capturable=capturable))
    if kind == "radam":
        return (torch.optim.RAdam(ref, lr=1e-3, eps=1e-8, weight_decay=wd, decoupled_weight_decay=True),
                train.RAdam(mine, lr=1e-3, eps=1e-8, weight_decay=wd, capturable=capturable))
    return _Lookahead(ref, 1e-3, wd), train.Ranger(mine, lr=1e-3, eps=1e-8, weight_decay=wd, capturable=capturable)


KINDS = ["sgd", "sgd0", "adam", "radam", "ranger"]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("kind", KINDS)
def test_one_launch_optimizer_matches_torch(kind, wd):
    """14 steps over 72 tensors of mixed shapes (two launches), a learning-rate change at step 8 and a parameter without
    a gradient at step 3."""
    base, g = _params(11)
    ref = [torch.nn.Parameter(b.clone()) for b in base]
    mine = [torch.nn.Parameter(b.clone()) for b in base]
    o_ref, o_mine = _pair(kind, ref, mine, wd)
    for step in range(STEPS):
        if step == 7:
            for o in (o_ref, o_mine):
                o.param_groups[0]["lr"] *= 0.3
        for k, (a, b) in enumerate(zip(ref, mine)):
            if step == 2 and k == 1:
                a.grad = b.grad = None
                continue
            gr = _grad(a.shape, g)
            a.grad, b.grad = gr.clone(), gr.clone()
        o_ref.step()
        o_mine.step()
    worst = 0.0
    for a, b in zip(ref, mine):
        err, tol = (a - b).abs().max().item(), 1e-6 * max(1.0, a.abs().max().item())
        worst = max(worst, err / tol)
        assert err <= tol, (kind, wd, err, tol)
    assert any(not torch.equal(a.detach(), b0) for a, b0 in zip(ref, base))      # something moved
    print(f"{kind} wd={wd}: worst error {worst:.3f} x tolerance")


def test_adam_kernel_without_weight_decay_is_bit_identical_to_nfl_adam_step():
    """nfl_optim_step(NFL_OPT_ADAM, wd = 0) against nfl_adam_step on the same tensors, 14 steps, aligned and unaligned
    (offset views: the scalar path) tensors."""
    import gpu_util
    from nerf_fl_amd import _lib
    L = _lib.lib()
    dev = gpu_util.DEV
    g = torch.Generator().manual_seed(4)
    sizes = [4096, 1, 257, 3 * 1024 + 3]
    mk = lambda: [torch.randn(n + 1, generator=g).to(dev)[1:] if i % 2 else torch.randn(n, generator=g).to(dev)
                  for i, n in enumerate(sizes)]
    p = mk()
    q = [x.clone() for x in p]
    sa = [(torch.zeros_like(x), torch.zeros_like(x)) for x in p]
    sb = [(torch.zeros_like(x), torch.zeros_like(x)) for x in p]
    for t in range(1, STEPS + 1):
        grads = [_grad(x.shape, g) for x in p]
        ta, tb = _lib.AdamTensors(), _lib.OptimTensors()
        for k, x in enumerate(p):
            ta.param[k], ta.grad[k], ta.exp_avg[k], ta.exp_avg_sq[k] = (x.data_ptr(), grads[k].data_ptr(), sa[k][0].data_ptr(),
                                                                        sa[k][1].data_ptr())
            tb.param[k], tb.grad[k], tb.state0[k], tb.state1[k] = (q[k].data_ptr(), grads[k].data_ptr(), sb[k][0].data_ptr(),
                                                                   sb[k][1].data_ptr())
            ta.numel[k] = tb.numel[k] = x.numel()
        lr = 5e-4 if t < 8 else 1e-4
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.nfl_adam_step(C.byref(ta), len(p), lr, 0.9, 0.999, 1e-8, t, s) == 0
        hyper = (C.c_float * _lib.NFL_OPT_HYPER)(lr, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 0.0)
        assert L.nfl_optim_step(C.byref(tb), len(p), _lib.NFL_OPT_ADAM, hyper, t, s) == 0
    torch.cuda.synchronize()
    for k in range(len(p)):
        assert torch.equal(p[k], q[k]) and torch.equal(sa[k][0], sb[k][0]) and torch.equal(sa[k][1], sb[k][1]), k


def _twins(kind, wd, seed):
    base, g = _params(seed)
    a = [torch.nn.Parameter(b.clone()) for b in base]
    b = [torch.nn.Parameter(x.clone()) for x in base]
    _, oa = _pair(kind, [torch.nn.Parameter(x.clone()) for x in base], a, wd)
    _, ob = _pair(kind, [torch.nn.Parameter(x.clone()) for x in base], b, wd, capturable=True)
    return a, b, oa, ob, g


def _feed(a, b, g):
    """the same fresh gradient into the eager twin (new tensors) and the captured one (in place: the graph reads them)"""
    for x, y in zip(a, b):
        gr = _grad(x.shape, g)
        x.grad = gr.clone()
        if y.grad is None:
            y.grad = gr.clone()
        else:
            y.grad.copy_(gr)


def _capture(opt):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    return graph


def _replay(graph, opt):
    opt.sync_hyper()
    graph.replay()
    opt.note_replay()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("kind", KINDS)
def test_captured_step_equals_the_eager_one_bitwise(kind, wd):
    """one eager step, then step() captured once and replayed 13 times (lr changed through sync_hyper at replay 7),
    against an eager twin fed the same gradients"""
    a, b, oa, ob, g = _twins(kind, wd, 3)
    _feed(a, b, g)
    oa.step()
    ob.step()
    graph = _capture(ob)
    for i in range(STEPS - 1):
        if i == 6:
            for o in (oa, ob):
                o.param_groups[0]["lr"] *= 0.5
        _feed(a, b, g)
        oa.step()
        _replay(graph, ob)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach())
    for x, y in zip(a, b):
        for k, v in oa.state[x].items():
            assert (torch.equal(v, ob.state[y][k]) if torch.is_tensor(v) else v == ob.state[y][k]), k


@pytest.mark.parametrize("kind,wd", [("adam", 0.0), ("adam", 1e-2), ("sgd", 1e-2), ("radam", 0.0), ("ranger", 1e-2)])
def test_load_state_dict_under_a_captured_graph(kind, wd):
    """load_state_dict resets the state a captured step() reads IN PLACE: after loading an older checkpoint (and the
    parameters), replays continue from it exactly like an eager twin that never left it."""
    a, b, oa, ob, g = _twins(kind, wd, 8)
    _feed(a, b, g)
    oa.step()
    ob.step()
    graph = _capture(ob)
    for _ in range(3):
        _feed(a, b, g)
        oa.step()
        _replay(graph, ob)
    ckpt, pa = copy.deepcopy(oa.state_dict()), [x.detach().clone() for x in a]
    for _ in range(3):                            # the captured twin moves on ...
        _feed(a, b, g)
        _replay(graph, ob)
    ob.load_state_dict(copy.deepcopy(ckpt))       # ... and is put back to the checkpoint
    with torch.no_grad():
        for y, x in zip(b, pa):
            y.copy_(x)
    for _ in range(8):                            # crosses a Ranger sync (t = 12) and the RAdam rectification
        _feed(a, b, g)
        oa.step()
        _replay(graph, ob)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize("kind", KINDS)
def test_step_moves_parameter_versions(kind):
    import gpu_util
    from nerf_fl_amd import train
    p = torch.nn.Parameter(torch.ones(8, device=gpu_util.DEV))
    o = {"sgd": lambda: train.SGD([p], lr=0.1, momentum=0.9), "sgd0": lambda: train.SGD([p], lr=0.1),
         "adam": lambda: train.Adam([p], lr=0.1, weight_decay=1e-2), "radam": lambda: train.RAdam([p], lr=0.1),
         "ranger": lambda: train.Ranger([p], lr=0.1)}[kind]()
    p.grad = torch.ones_like(p)
    v0 = p._version
    o.step()
    assert p._version > v0 and not torch.equal(p.detach().cpu(), torch.ones(8))


@pytest.mark.parametrize("kind", ["sgd", "radam"])
def test_state_dicts_load_into_torch(kind):
    """SGD's state dict continues in torch.optim.SGD, RAdam's in torch.optim.RAdam(decoupled_weight_decay=True)."""
    base, g = _params(21)
    mine = [torch.nn.Parameter(b.clone()) for b in base]
    o = _pair(kind, [torch.nn.Parameter(b.clone()) for b in base], mine, 1e-2)[1]
    for _ in range(7):
        for p in mine:
            p.grad = _grad(p.shape, g)
        o.step()
    sd = copy.deepcopy(o.state_dict())
    assert set(sd["state"][0]) == ({"momentum_buffer"} if kind == "sgd" else {"step", "exp_avg", "exp_avg_sq"})
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    t = (torch.optim.SGD(theirs, lr=1e-2, momentum=0.9, weight_decay=1e-2) if kind == "sgd" else
         torch.optim.RAdam(theirs, lr=1e-3, eps=1e-8, weight_decay=1e-2, decoupled_weight_decay=True))
    t.load_state_dict(sd)
    for p, q in zip(mine, theirs):
        p.grad = _grad(p.shape, g)
        q.grad = p.grad.clone()
    o.step()
    t.step()
    for p, q in zip(mine, theirs):
        assert (p - q).abs().max().item() <= 1e-6 * max(1.0, q.abs().max().item())


def test_graphed_train_step_with_ranger_has_no_memset_or_memcpy_node():
    """Ranger's slow buffers are created by the eager warm-up steps: the captured step is kernels only"""
    import math

    import gpu_util
    from nerf_fl_amd.train import RayTrainer, Ranger
    from oracle import nerfw_oracle as orc
    from test_refine_pose_train_gpu import _graph_nodes
    dev = gpu_util.DEV
    tr = RayTrainer(dev, N_samples=16, N_importance=16, encode_a=True, encode_t=True, N_vocab=8, batch_size=256,
                    optimizer="ranger", weight_decay=1e-4, use_graph=True)
    assert isinstance(tr.opt, Ranger) and tr.opt.capturable
    rays = orc.make_rays(256, 5).to(dev)
    ts = torch.randint(0, 8, (256,), device=dev)
    rgbs = torch.rand(256, 3, device=dev)
    gs = tr.graphed_step(rays, ts, rgbs, keep_graph=True)
    types = _graph_nodes(gs.graph.raw_cuda_graph())
    print(f"captured step with Ranger: {len(types)} nodes, types {sorted(set(types))}")
    assert types.count(0) >= 10
    bad = [t for t in types if t in (1, 2, 12, 13)]           # memcpy, memset, memcpy from / to symbol
    assert not bad, bad
    loss, _ = gs.replay()
    assert math.isfinite(loss.item())
