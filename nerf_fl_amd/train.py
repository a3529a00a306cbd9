"""A thin training harness for the HIP renderer (the role of the reference's NeRFSystem +
Lightning Trainer, train.py:33-241, without Lightning).

What it keeps from the reference:
  * modules and their checkpoint key prefixes -- `nerf_coarse.*`, `nerf_fine.*`, `embedding_a.*`,
    `embedding_t.*` (train.py:51-76) -- so `utils.load_ckpt` (utils/__init__.py:67-88) and this
    harness can exchange weights;
  * the optimisers of --optimizer sgd | adam | radam | ranger with --momentum / --weight_decay (utils/__init__.py:24-42),
    the per-epoch schedules steplr / cosine / poly with the linear warm-up (utils/__init__.py:44-61,
    utils/warmup_scheduler.py), NerfWLoss (losses.py:18-50), PSNR = -10 log10(mse) (metrics.py:12-13).
What it does differently, because the renderer is ~10^3 x faster than the data path around it:
  * rays / colours / image ids live on the GPU as flat tensors; a batch is a slice of a device-side
    permutation (no DataLoader workers, no per-item collation: train.py:144-149);
  * rays are the upstream 8-column Blender contract (o, d, near, far) handed straight to render_rays; with
    refine_pose=True they are the fork's camera-frame layout, turned into world rays by the HIP pose kernels
    (poses.posed_rays) inside the step;
  * multi-GPU: every rank shuffles its own shard; gradients are averaged with one flat all-reduce.
"""
import ctypes as C
import math
import os

import torch
from torch import nn

from . import _lib, parallel
from .eval import _chunks
from .nerf import BarfPosEmbedding, NeRF, PosEmbedding
from .poses import LearnPose, posed_rays, row_table
from .rendering import fill_barf_weights, render_rays

__all__ = ["NerfWLoss", "psnr", "Adam", "SGD", "RAdam", "Ranger", "GradualWarmupLR", "make_optimizer", "make_scheduler",
           "RayTrainer", "GraphedTrainStep", "rank_seed", "reference_parameter_names"]


class NerfWLoss(nn.Module):
    """Equation 13 of NeRF-W as the reference implements it (losses.py:18-50): c_l, f_l, b_l (+3), s_l."""

    def __init__(self, coef=1.0, lambda_u=0.01):
        super().__init__()
        self.coef, self.lambda_u = coef, lambda_u

    def forward(self, inputs, targets):
        """The terms through the C ABI (nfl_loss_forward / nfl_loss_backward): two launches instead of ~16.  Device tensors
        only, like everything in this package (the CPU restatement of the loss is oracle/nerfw_oracle.py: nerfw_loss)."""
        if not targets.is_cuda:
            raise RuntimeError("nerf_fl_amd.train.NerfWLoss: device tensors only (this build has no CPU path)")
        rgb_f, beta = inputs.get("rgb_fine"), inputs.get("beta")
        tsig = inputs.get("transient_sigmas") if beta is not None else None
        c_l, f_l, b_l, s_l = _FusedNerfWLoss.apply(inputs["rgb_coarse"], rgb_f, beta, tsig, targets, float(self.coef),
                                                   float(self.lambda_u))
        ret = {"c_l": c_l}
        if rgb_f is not None:
            ret["f_l"] = f_l
            if beta is not None:
                ret["b_l"], ret["s_l"] = b_l, s_l
        return ret


def _ptr(t):
    return None if t is None else t.data_ptr()


class _FusedNerfWLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb_c, rgb_f, beta, tsig, targets, coef, lambda_u):
        ctx.set_materialize_grads(False)
        f32c = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
        ctx.inputs = rgb_c, rgb_f, beta, tsig, targets = f32c(rgb_c), f32c(rgb_f), f32c(beta), f32c(tsig), f32c(targets)
        ctx.args = a = _lib.LossArgs()          # the backward fills in only its gradient pointers
        a.d_rgb_coarse, a.d_rgb_fine, a.d_beta, a.d_transient_sigmas, a.d_target = map(_ptr, ctx.inputs)
        a.n_rays, a.n_samples = rgb_c.shape[0], (tsig.shape[1] if tsig is not None else 0)
        a.coef, a.lambda_u = coef, lambda_u
        losses = torch.empty(4, dtype=torch.float32, device=targets.device)
        a.d_losses = losses.data_ptr()
        with torch.cuda.device(targets.device):
            _lib.check(_lib.lib().nfl_loss_forward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_loss_forward")
        return losses[0], losses[1], losses[2], losses[3]

    @staticmethod
    def backward(ctx, *go):
        rgb_c, rgb_f, beta, tsig, targets = ctx.inputs
        a = ctx.args
        keep = [None if g is None else g.to(torch.float32).contiguous() for g in go]
        for k in range(4):
            a.d_grad_loss[k] = _ptr(keep[k])
        g_c = torch.empty_like(rgb_c)
        g_f = torch.empty_like(rgb_f) if rgb_f is not None else None
        g_b = torch.empty_like(beta) if beta is not None else None
        g_s = torch.empty_like(tsig) if tsig is not None else None
        a.d_g_rgb_coarse, a.d_g_rgb_fine, a.d_g_beta, a.d_g_transient_sigmas = _ptr(g_c), _ptr(g_f), _ptr(g_b), _ptr(g_s)
        with torch.cuda.device(targets.device):
            _lib.check(_lib.lib().nfl_loss_backward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_loss_backward")
        return g_c, g_f, g_b, g_s, None, None, None


def psnr(pred, gt):
    return -10.0 * torch.log10(((pred - gt) ** 2).mean())


class _OneLaunchOptimizer(torch.optim.Optimizer):
    """Shared machinery of this package's optimisers: each (param group, device, step) is updated by ONE kernel launch per
    NFL_ADAM_MAX_TENSORS tensors, the parameters' version counters are moved after it (render_rays re-packs its weight
    streams on that), and with capturable=True the launch reads its hyper-parameters and the step count from device
    memory, so that `step()` can be captured in a HIP graph (GraphedTrainStep).  A regular torch Optimizer otherwise:
    param_groups (LR schedulers work) and per-parameter state under torch's names.

    capturable=True: the device-side step count is ONE counter per (param group, device), seeded from the largest host-side
    step of the group: all tensors of a group share their bias corrections (torch counts per parameter; the two agree
    whenever every parameter of a group receives a gradient at every step, which is how this package trains).
    `sync_hyper()` uploads the current param_groups' values; `note_replay()` counts a replayed captured step."""

    _name = "optimizer"
    _state_keys = ()          # per-parameter state tensors, created as zeros on the first step
    _counts_steps = True      # state[p]["step"] (torch.optim.SGD keeps none)

    def __init__(self, params, defaults, capturable):
        self._dev = {}            # (group index, device) -> dict(hyper=float[8] tensor, step=int32 tensor, host=tuple)
        self._captured = set()    # id(p) of the parameters a captured step() updates
        super().__init__(params, defaults)
        self.capturable = bool(capturable)

    # ---- per-kind hooks ----------------------------------------------------------------------------------------
    def _hyper(self, group):
        """The NFL_OPT_HYPER floats of a group: lr, beta1 | momentum, beta2, eps, weight_decay, alpha, k, threshold."""
        raise NotImplementedError

    def _kind(self, group):
        raise NotImplementedError

    def _init_state(self, p, st, group):
        if self._counts_steps:
            st["step"] = 0
        for k in self._state_keys:
            st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format)

    def _state_ptrs(self, st):
        """(state0, state1, state2) of nfl_optim_tensors, None where the kind has none."""
        ptrs = [st[k] if st.get(k) is not None else None for k in self._state_keys]
        return tuple(ptrs + [None] * (3 - len(ptrs)))

    # ---- device-side state ------------------------------------------------------------------------------------
    def _dev_state(self, gi, group, dev):
        k = (gi, str(dev))
        if k not in self._dev:
            self._dev[k] = dict(hyper=torch.zeros(_lib.NFL_OPT_HYPER, dtype=torch.float32, device=dev),
                                step=torch.full((1,), self._group_step(group), dtype=torch.int32, device=dev), host=None)
        return self._dev[k]

    def device_state(self, dev, groups=None):
        """(groups, tensors): the device-side step and hyper-parameter tensors on `dev` of param groups `groups` (default:
        every group that has them), created where missing, as [step, hyper] per group in `groups` order, for a caller
        that overwrites them in place (RayTrainer.broadcast).  The cached host values are cleared, so the next
        sync_hyper() uploads again."""
        if groups is None:
            groups = sorted(gi for gi, d in self._dev if d == str(dev))
        tensors = []
        for gi in groups:
            ds = self._dev_state(gi, self.param_groups[gi], dev)
            ds["host"] = None
            tensors += [ds["step"], ds["hyper"]]
        return groups, tensors

    def _group_step(self, group):
        steps = [int(self.state[p]["step"]) for p in group["params"] if "step" in self.state.get(p, {})]
        return max(steps) if steps else 0

    def load_state_dict(self, state_dict):
        """torch's loader, then the loaded values are copied INTO the state tensors this optimizer already had, and the
        device-side step counters are reset in place from the loaded steps (hyper-parameters re-uploaded by the next
        sync_hyper()): a step() captured before keeps reading and writing live memory, and continues from the checkpoint."""
        old = {p: {k: v for k, v in st.items() if torch.is_tensor(v) and k in self._state_keys}
               for p, st in self.state.items()}
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            if "step" in st:
                st["step"] = int(st["step"])             # torch.optim.RAdam / SGD checkpoints hold tensors
            for k, t in old.get(p, {}).items():
                new = st.get(k)
                if torch.is_tensor(new) and new.shape == t.shape:
                    t.copy_(new)
                    st[k] = t
        for (gi, _dev), ds in self._dev.items():
            ds["step"].fill_(self._group_step(self.param_groups[gi]))
            ds["host"] = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if getattr(self, "_dev", None):
            self._dev = {}

    def sync_hyper(self):
        """Upload the hyper-parameters of every param group to the device copies the captured launches read (host -> device
        copies: call it outside graph capture; GraphedTrainStep.replay() does)."""
        for (gi, _dev), st in self._dev.items():
            host = tuple(float(x) for x in self._hyper(self.param_groups[gi]))
            if st["host"] != host:
                st["hyper"].copy_(torch.tensor(host, dtype=torch.float32))
                st["host"] = host

    def note_replay(self):
        """A captured step() was replayed: advance the host-side step counts (state_dict compatibility) of the parameters
        the captured launch updates (those that had a gradient when it was captured)."""
        if not self._counts_steps:
            return
        for group in self.param_groups:
            for p in group["params"]:
                if self.state.get(p) and (not self._captured or id(p) in self._captured):
                    self.state[p]["step"] = int(self.state[p]["step"]) + 1

    # ---- the step ---------------------------------------------------------------------------------------------
    def _launch(self, L, group, chunk, step, ds, last, stream):
        t = _lib.OptimTensors()
        for k, (p, g, st) in enumerate(chunk):
            s0, s1, s2 = self._state_ptrs(st)
            t.param[k], t.grad[k] = p.data_ptr(), g.data_ptr()
            t.state0[k], t.state1[k], t.state2[k] = (x.data_ptr() if x is not None else None for x in (s0, s1, s2))
            t.numel[k] = p.numel()
        kind = self._kind(group)
        if ds is not None:
            _lib.check(L.nfl_optim_step_dev(C.byref(t), len(chunk), kind, C.c_void_p(ds["hyper"].data_ptr()),
                                            C.c_void_p(ds["step"].data_ptr()), int(last), stream), "nfl_optim_step_dev")
        else:
            hyper = (C.c_float * _lib.NFL_OPT_HYPER)(*self._hyper(group))
            _lib.check(L.nfl_optim_step(C.byref(t), len(chunk), kind, hyper, max(1, step), stream), "nfl_optim_step")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        who = f"nerf_fl_amd.train.{type(self).__name__}"
        capturing = self.capturable and torch.cuda.is_current_stream_capturing()
        for gi, group in enumerate(self.param_groups):
            if self.capturable:                  # device-side counters start from the steps ALREADY taken
                for dev in {p.device for p in group["params"] if p.grad is not None}:
                    self._dev_state(gi, group, dev)
            todo = {}                            # (device, step) -> list of (p, grad, state)
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or p.grad.is_sparse:
                    raise RuntimeError(f"{who}: dense fp32 parameters on a ROCm device only")
                if not p.is_contiguous():
                    raise RuntimeError(f"{who}: parameters must be contiguous")
                st = self.state[p]
                if any(st.get(k) is None for k in self._state_keys) or (self._counts_steps and "step" not in st):
                    if capturing:                # no allocation or copy inside a capture: the state exists before it
                        raise RuntimeError(f"{who}: run one eager step() before capture")
                    self._init_state(p, st, group)
                if self._counts_steps:
                    if not capturing:            # a captured launch runs at replay time: note_replay() counts it
                        st["step"] = int(st["step"]) + 1
                if capturing:
                    self._captured.add(id(p))
                # capturable: one device-side counter per (group, device), so all of a group's tensors step together
                key = 0 if self.capturable or not self._counts_steps else st["step"]
                todo.setdefault((p.device, key), []).append((p, p.grad.contiguous(), st))
            for (dev, step), items in todo.items():
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                    ds = None
                    if self.capturable:
                        ds = self._dev_state(gi, group, dev)
                        if not capturing:
                            self.sync_hyper()
                        elif ds["host"] is None:
                            raise RuntimeError(f"{who}: run one eager step() (or sync_hyper()) before capture")
                    for i0 in range(0, len(items), _lib.NFL_ADAM_MAX_TENSORS):
                        chunk = items[i0:i0 + _lib.NFL_ADAM_MAX_TENSORS]
                        self._launch(L, group, chunk, step, ds, i0 + _lib.NFL_ADAM_MAX_TENSORS >= len(items), stream)
                        # the kernel wrote the parameters behind autograd's back: bump their version counters, which
                        # is what tells render_rays to re-pack the weight streams (and autograd to refuse stale graphs)
                        torch.autograd.graph.increment_version([p for p, _, _ in chunk])
        return loss


class Adam(_OneLaunchOptimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay) -- coupled L2 weight decay, no amsgrad; the reference's settings are
    lr, eps=1e-8 and --weight_decay (utils/__init__.py:30-32) -- with the whole step in ONE kernel launch.
    state[p] = {step, exp_avg, exp_avg_sq} with torch's names, so state_dict()s are interchangeable with torch.optim.Adam's.
    weight_decay == 0 runs C ABI `nfl_adam_step` (`_dev` when capturable), otherwise `nfl_optim_step(NFL_OPT_ADAM)`; a
    captured step keeps the launch it was captured with."""

    _name = "Adam"
    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False):
        """capturable=True: learning rate, betas, eps, weight decay and the step count are kept in device memory and read
        by the kernel, so `step()` can be captured in a HIP graph and replayed while a scheduler changes the rate."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), capturable)

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return (group["lr"], b1, b2, group["eps"], group["weight_decay"], 0.0, 0.0, 0.0)

    def _kind(self, group):
        return _lib.NFL_OPT_ADAM

    def _launch(self, L, group, chunk, step, ds, last, stream):
        if group["weight_decay"] != 0:
            return super()._launch(L, group, chunk, step, ds, last, stream)
        t = _lib.AdamTensors()
        for k, (p, g, st) in enumerate(chunk):
            t.param[k], t.grad[k] = p.data_ptr(), g.data_ptr()
            t.exp_avg[k], t.exp_avg_sq[k] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            t.numel[k] = p.numel()
        if ds is not None:       # the hyper vector's first four floats are nfl_adam_step_dev's {lr, beta1, beta2, eps}
            _lib.check(L.nfl_adam_step_dev(C.byref(t), len(chunk), C.c_void_p(ds["hyper"].data_ptr()),
                                           C.c_void_p(ds["step"].data_ptr()), int(last), stream), "nfl_adam_step_dev")
        else:
            b1, b2 = group["betas"]
            _lib.check(L.nfl_adam_step(C.byref(t), len(chunk), float(group["lr"]), float(b1), float(b2),
                                       float(group["eps"]), step, stream), "nfl_adam_step")


class SGD(_OneLaunchOptimizer):
    """torch.optim.SGD(lr, momentum, dampening=0, weight_decay), no nesterov (the reference's --optimizer sgd,
    utils/__init__.py:27-29), one launch of `nfl_optim_step(NFL_OPT_SGD)`.  state[p] = {momentum_buffer} (none without
    momentum), loadable by torch.optim.SGD.  The buffer starts at zero, which makes the first update buf = g exactly."""

    _name = "SGD"
    _counts_steps = False

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, capturable=False):
        if momentum < 0.0:
            raise ValueError(f"momentum must be >= 0, got {momentum}")
        self._state_keys = ("momentum_buffer",) if momentum != 0.0 else ()
        # dampening / nesterov: torch.optim.SGD's fixed settings here, in the groups so that its step() can continue them
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0, nesterov=False),
                         capturable)

    def _hyper(self, group):
        return (group["lr"], group["momentum"], 0.0, 0.0, group["weight_decay"], 0.0, 0.0, 0.0)

    def _kind(self, group):
        return _lib.NFL_OPT_SGD


class RAdam(_OneLaunchOptimizer):
    """torch_optimizer.RAdam (0.3; the reference's --optimizer radam, utils/__init__.py:33-35): rectified Adam with
    decoupled weight decay, un-rectified while N_sma < 5.  Arithmetic in include/nerf_fl_amd.h (NFL_OPT_RADAM); the same
    algorithm as torch.optim.RAdam(decoupled_weight_decay=True).  state[p] = {step, exp_avg, exp_avg_sq}; state_dict()
    stores the steps as tensors, so it loads into torch.optim.RAdam.  Per-group step sizes (torch_optimizer caches them
    across groups)."""

    _name = "RAdam"
    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False):
        # decoupled_weight_decay: what torch.optim.RAdam needs to continue this state with the same algorithm
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True),
                         capturable)

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return (group["lr"], b1, b2, group["eps"], group["weight_decay"], 0.0, 0.0, 5.0)

    def _kind(self, group):
        return _lib.NFL_OPT_RADAM

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {i: {k: (torch.tensor(float(v), dtype=torch.float32) if k == "step" else v) for k, v in st.items()}
                       for i, st in sd["state"].items()}
        return sd


class Ranger(RAdam):
    """torch_optimizer.Ranger (0.3; the reference's --optimizer ranger, utils/__init__.py:36-38): RAdam (rectified while
    N_sma > N_sma_threshhold = 5) plus Lookahead -- every k-th step slow += alpha (p - slow), p = slow, with slow a copy
    of p taken when the state is created.  No gradient centralisation (0.3's Ranger has none).
    state[p] = {step, exp_avg, exp_avg_sq, slow_buffer}."""

    _name = "Ranger"
    _state_keys = ("exp_avg", "exp_avg_sq", "slow_buffer")

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, betas=(0.95, 0.999), eps=1e-8, weight_decay=0.0,
                 capturable=False):
        if not 0.0 <= alpha <= 1.0 or int(k) < 1:
            raise ValueError(f"Ranger needs 0 <= alpha <= 1 and k >= 1, got alpha={alpha}, k={k}")
        _OneLaunchOptimizer.__init__(self, params, dict(lr=lr, alpha=alpha, k=int(k), N_sma_threshhold=5, betas=betas,
                                                        eps=eps, weight_decay=weight_decay), capturable)

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return (group["lr"], b1, b2, group["eps"], group["weight_decay"], group["alpha"], group["k"],
                group["N_sma_threshhold"])

    def _kind(self, group):
        return _lib.NFL_OPT_RANGER

    def _init_state(self, p, st, group):
        super()._init_state(p, st, group)
        st["slow_buffer"] = p.detach().clone(memory_format=torch.contiguous_format)


OPTIMIZERS = ("sgd", "adam", "radam", "ranger")
LR_SCHEDULERS = (None, "steplr", "cosine", "poly")


def make_optimizer(name, params, lr=5e-4, momentum=0.9, weight_decay=0.0, eps=1e-8, capturable=False):
    """The reference's get_optimizer (utils/__init__.py:24-42) over this package's one-launch optimisers: `name` is
    opt.py's --optimizer (sgd | adam | radam | ranger); sgd takes `momentum`, the others eps=1e-8 as the reference
    passes it."""
    if name == "sgd":
        return SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay, capturable=capturable)
    if name == "adam":
        return Adam(params, lr=lr, eps=eps, weight_decay=weight_decay, capturable=capturable)
    if name == "radam":
        return RAdam(params, lr=lr, eps=eps, weight_decay=weight_decay, capturable=capturable)
    if name == "ranger":
        return Ranger(params, lr=lr, eps=eps, weight_decay=weight_decay, capturable=capturable)
    raise ValueError(f"optimizer not recognized: {name!r} (one of {', '.join(OPTIMIZERS)})")


class GradualWarmupLR(torch.optim.lr_scheduler.LRScheduler):
    """Linear learning-rate warm-up per epoch, then another scheduler (the behaviour of the reference's
    GradualWarmupScheduler, utils/warmup_scheduler.py, as get_scheduler drives it):
      epochs e = 0 .. T:  lr = base ((multiplier - 1) e / T + 1);
      epoch T + 1:        `after` takes over with its base lrs scaled by `multiplier`: the rate is its own update rule
                          evaluated once at its epoch 0 from the current rate base multiplier (that rate itself for
                          MultiStepLR and poly; CosineAnnealingLR's recursive form gives slightly more, x1.0062 at
                          T_max = 20 -- what the reference computes);
      later epochs:       each step() steps `after` (so its own epoch count, e.g. MultiStepLR's milestones, starts at
                          T + 1).  Without `after` the rate stays at base multiplier."""

    def __init__(self, optimizer, multiplier, warmup_epochs, after=None):
        if multiplier < 1.0:
            raise ValueError(f"warmup multiplier must be >= 1, got {multiplier}")
        if warmup_epochs < 1:
            raise ValueError(f"warmup_epochs must be >= 1, got {warmup_epochs}")
        self.multiplier, self.warmup_epochs, self.after = float(multiplier), int(warmup_epochs), after
        self.handed_over = False
        super().__init__(optimizer)

    def get_lr(self):
        e = self.last_epoch
        if e <= self.warmup_epochs:
            return [b * ((self.multiplier - 1.0) * e / self.warmup_epochs + 1.0) for b in self.base_lrs]
        if self.after is None:
            return [b * self.multiplier for b in self.base_lrs]
        import warnings
        self.after.base_lrs = [b * self.multiplier for b in self.base_lrs]
        self.handed_over = True
        with warnings.catch_warnings():          # torch warns about get_lr() outside the follower's own step()
            warnings.simplefilter("ignore")
            return list(self.after.get_lr())

    def step(self, epoch=None):
        if epoch is not None:
            raise ValueError("GradualWarmupLR steps one epoch at a time")
        if self.handed_over:
            self.after.step()
            self._last_lr = self.after.get_last_lr()
        else:
            super().step()

    def state_dict(self):
        """Plain values only (the follower as its own state dict, not the object and its optimizer), so that a checkpoint
        holding it loads with torch.load(weights_only=True)."""
        sd = {k: v for k, v in self.__dict__.items() if k not in ("optimizer", "after")}
        sd["after"] = None if self.after is None else self.after.state_dict()
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        after = sd.pop("after", None)
        self.__dict__.update(sd)
        if self.after is not None and after is not None:
            self.after.load_state_dict(after)


def make_scheduler(opt, name, num_epochs=16, decay_step=(20,), decay_gamma=0.1, poly_exp=0.9, warmup_multiplier=1.0,
                   warmup_epochs=0, optimizer="adam"):
    """The reference's get_scheduler (utils/__init__.py:44-61), stepped once per epoch: `name` is opt.py's --lr_scheduler
    (steplr | cosine | poly) or None (a constant rate); warmup_epochs > 0 wraps it in GradualWarmupLR, for the sgd and
    adam optimisers only (radam and ranger ignore it, as in the reference).  poly is LambdaLR((1 - e / num_epochs) ^
    poly_exp), the reference's evident intent (its get_scheduler never imports LambdaLR)."""
    if name not in LR_SCHEDULERS:
        raise ValueError(f"scheduler not recognized: {name!r} (one of steplr, cosine, poly or None)")
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer not recognized: {optimizer!r} (one of {', '.join(OPTIMIZERS)})")
    sched = None
    if name == "steplr":
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(decay_step), gamma=decay_gamma)
    elif name == "cosine":
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=num_epochs, eta_min=1e-8)
    elif name == "poly":
        sched = torch.optim.lr_scheduler.LambdaLR(
            opt, lambda e: max(0.0, 1.0 - e / num_epochs) ** poly_exp)
    if warmup_epochs > 0 and optimizer in ("sgd", "adam"):
        sched = GradualWarmupLR(opt, warmup_multiplier, warmup_epochs, after=sched)
    return sched


def rank_seed(seed, rank, epoch=0):
    """The seed of rank `rank`'s random streams in a run of more than one rank: (seed * 1000003 + rank) * 1000003 + epoch,
    modulo 2**63 -- distinct for every rank (and epoch) below 1000003.  Under a process group RayTrainer seeds the device's
    default generator (stratified jitter, sigma noise, importance u) with it and its permutation generator with it + 1:
    at construction with epoch 0, and again on ranks other than 0 after resume(), with the epoch resumed at.  A single
    process keeps `seed` and `seed + 1`, as before."""
    return ((int(seed) * 1000003 + int(rank)) * 1000003 + int(epoch)) % (1 << 63)


def reference_parameter_names(modules):
    """Checkpoint names of the parameters of the reference's optimiser, in its order: get_parameters(models_to_train)
    (utils/__init__.py:11-22) over [embedding_a, embedding_t, {coarse, fine}, learn_poses] (train.py:46-76, 134-136).
    Its `optimizer_states[0]` is indexed by position in this list.  `modules` maps checkpoint prefixes to modules whose
    parameters carry the reference's names in the reference's order (RayTrainer.modules; nerf_fl_amd.NeRF does).
    `learn_poses` is always there in the reference, with init_c2w and, frozen unless --refine_pose, r and t."""
    names = []
    for prefix in ("embedding_a", "embedding_t", "nerf_coarse", "nerf_fine"):
        if prefix in modules:
            names += [f"{prefix}.{n}" for n, _ in modules[prefix].named_parameters()]
    return names + ["learn_poses.init_c2w", "learn_poses.r", "learn_poses.t"]


def _rank_world():
    import torch.distributed as dist
    return (dist.get_rank(), dist.get_world_size()) if dist.is_initialized() else (0, 1)


def _loss_backward(models, embeddings, hp, rays, ts, target, arena, loss_fn=None, loss_coef=1.0, lambda_u=0.01,
                   pose=None, row_of_id=None, barf_weights=None):
    """The body of a training step up to the gradients, eager or captured: rays through the learned poses (with `pose`),
    render_rays with the sampling hyper-parameters `hp` (N_samples, N_importance, use_disp, perturb, noise_std,
    white_back), the loss and its backward into `arena`.  `loss_fn=None`: NerfWLoss(loss_coef, lambda_u) fused into the
    render kernels' per-ray epilogue, whose backward seeds with it; otherwise sum(loss_fn(result, target).values()).
    Returns (loss, psnr) as device scalars."""
    if pose is not None:
        rays = posed_rays(pose, rays, ts, row_of_id, grad_arena=arena)
    res = render_rays(models, embeddings, rays, ts, hp["N_samples"], hp["use_disp"], hp["perturb"], hp["noise_std"],
                      hp["N_importance"], 32768, hp["white_back"], False, grad_arena=arena, barf_weights=barf_weights,
                      loss_target=target if loss_fn is None else None, loss_coef=loss_coef, lambda_u=lambda_u)
    total = res["_nerfw_loss"] if loss_fn is None else sum(loss_fn(res, target).values())
    total.backward()
    key = "rgb_fine" if "rgb_fine" in res else "rgb_coarse"
    return total.detach(), psnr(res[key].detach(), target)


class GraphedTrainStep:
    """One fixed-shape optimisation step -- weight re-pack, render_rays forward, NerfWLoss, the HIP backward, Adam --
    captured ONCE into a HIP graph and replayed: a step becomes one graph launch (~35 kernel launches, ~25 allocations
    and their Python disappear from the host's critical path; what matters at the README batch of 1024 rays, where the
    kernels take ~1.3 ms).  Random draws come from torch's graph-safe Philox generator, so every replay draws afresh.

    `opt` must be one of this module's optimisers (Adam, SGD, RAdam, Ranger) built with capturable=True; `loss_fn=None` uses the loss fused into the render kernels.  Batches are
    loaded into the static buffers with `load()`.
    Construction runs `warmup` REAL steps eagerly (kernel attributes, optimizer state) before capturing.
    With `all_reduce=True` (ranks > 1) the step is two graphs with the flat gradient all-reduce between them."""

    def __init__(self, models, embeddings, params, opt, loss_fn, rays, ts, target, N_samples, N_importance,
                 use_disp=False, perturb=1.0, noise_std=1.0, white_back=True, all_reduce=False, warmup=2,
                 loss_coef=1.0, lambda_u=0.01, arena=None, capture_all_reduce=None, force_all_reduce=False,
                 pose=None, row_of_id=None, barf_weights=None, keep_graph=False):
        """loss_coef / lambda_u: NerfWLoss's constants for the fused loss (loss_fn=None); with a loss_fn they are its own.
        arena: the GradArena that holds the parameters' gradients (created here when None): the backward writes into it
        and the all-reduce runs on it in place.
        capture_all_reduce: record the collective INSIDE the one graph (RCCL supports stream capture); None = yes for
        the nccl backend, no otherwise (gloo cannot be captured: the step is then two graphs around an eager collective).
        force_all_reduce: issue the collective at world size 1 too (exercises RCCL on a single GPU).
        pose / row_of_id: learnable poses (poses.LearnPose, its parameters in `params`) and the image id -> pose row table:
        `rays` is then the camera-frame layout (direction, near, far, ...) and `ts` the image ids, and the pose forward and
        backward (poses.posed_rays) are captured with the rest of the step.
        barf_weights: (w_xyz, w_dir) device buffers for fields built with refine_pose=True (rendering.fill_barf_weights
        refills them between replays).
        keep_graph: keep the captured graph after instantiation (torch.cuda.CUDAGraph(keep_graph=True)), so that it can be
        inspected through raw_cuda_graph()."""
        if not getattr(opt, "capturable", False):
            raise ValueError("GraphedTrainStep needs one of nerf_fl_amd.train's optimisers (Adam, SGD, RAdam, Ranger) "
                             "built with capturable=True")
        import torch.distributed as dist
        self.params, self.opt, self.all_reduce = list(params), opt, bool(all_reduce)
        self.rays, self.ts, self.target = rays.detach().clone(), ts.detach().clone(), target.detach().clone()
        self.arena = arena if arena is not None else parallel.GradArena(self.params)
        self.force = bool(force_all_reduce)
        if capture_all_reduce is None:
            capture_all_reduce = self.all_reduce and dist.is_initialized() and dist.get_backend() == "nccl"
        self.captured_collective = bool(capture_all_reduce) and self.all_reduce
        dev = self.rays.device
        hp = dict(N_samples=N_samples, N_importance=N_importance, use_disp=use_disp, perturb=perturb, noise_std=noise_std,
                  white_back=white_back)

        def fwd_bwd():
            # (parameters the backward never reaches keep the zeros the arena was created with)
            return _loss_backward(models, embeddings, hp, self.rays, self.ts, self.target, self.arena, loss_fn, loss_coef,
                                  lambda_u, pose, row_of_id, barf_weights)

        def reduce():
            self.arena.all_reduce(force=self.force)

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                fwd_bwd()
                if self.all_reduce:
                    reduce()
                opt.step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        missing = [i for i, p in enumerate(self.params) if p.requires_grad and p.grad is None]
        if missing:      # a captured opt.step() would skip them for ever
            raise RuntimeError(f"GraphedTrainStep: {len(missing)} trainable parameters have no gradient after the warm-up "
                               f"steps (first: index {missing[0]}); pass only parameters the step reaches")
        self.graph = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
        self.graph_opt = None
        from . import rendering
        self.rounding_seed = rendering._rounding_seed      # a by-value kernel argument: replays keep this one
        mode = rendering._capture_mode()
        with torch.cuda.graph(self.graph, **mode):
            self.out = fwd_bwd()
            if self.all_reduce and self.captured_collective:
                reduce()
            if not self.all_reduce or self.captured_collective:
                opt.step()
        if self.all_reduce and not self.captured_collective:
            self.graph_opt = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_opt, pool=self.graph.pool(), **mode):
                opt.step()
        if keep_graph:
            self.graph.instantiate()
            if self.graph_opt is not None:
                self.graph_opt.instantiate()

    def load(self, rays, ts, target):
        self.rays.copy_(rays)
        self.ts.copy_(ts)
        self.target.copy_(target)

    def replay(self):
        """Run the captured step on the loaded batch; returns (loss, psnr) as device scalars (valid until the next replay)."""
        self.opt.sync_hyper()
        self.graph.replay()
        if self.graph_opt is not None:
            self.arena.all_reduce(force=self.force)      # eager, in place on the arena the two graphs read and write
            self.graph_opt.replay()
        self.opt.note_replay()
        # the parameters changed behind autograd's back: move their version counters so that any eager render_rays
        # (validation) re-packs its weight streams
        torch.autograd.graph.increment_version(self.params)
        return self.out


class RayTrainer:
    """Fit coarse+fine fields to (rays, rgbs, ts) tensors that are already on the device, or to a data.ImageBank of
    uint8 images kept there (fit_epoch(bank))."""

    def __init__(self, device, N_emb_xyz=10, N_emb_dir=4, N_samples=64, N_importance=64, use_disp=False,
                 perturb=1.0, noise_std=1.0, white_back=True, encode_a=False, encode_t=False, N_vocab=100,
                 N_a=48, N_tau=16, beta_min=0.1, lr=5e-4, batch_size=1024, lr_scheduler=None, num_epochs=16,
                 decay_step=(20,), decay_gamma=0.1, seed=0, use_graph=False, refine_pose=False, init_c2w=None,
                 image_ids=None, optimizer="adam", momentum=0.9, weight_decay=0.0, poly_exp=0.9, warmup_multiplier=1.0,
                 warmup_epochs=0):
        """use_graph: run the steps of fit_epoch from one captured HIP graph (GraphedTrainStep).  At the README batch of
        1024 rays the ~35 launches of an eager step are the critical path (1.9 vs 1.67 ms per step); at 4096 rays it
        makes no difference.  The first fit_epoch call spends two extra steps on its first batch (warm-up before the capture).

        refine_pose: the reference's --refine_pose (train.py:42-44, 84-98, 136): BARF embeddings BarfPosEmbedding(N-1, N, 4, 8),
        fields built with refine_pose=True, and a LearnPose(C, True, True, init_c2w) under the checkpoint prefix
        `learn_poses`, trained by the same Adam through the same GradArena.  `step` / `fit_epoch` then take the fork's
        training layout: rays = camera-frame direction, near, far (further columns ignored), ts = image ids; the BARF
        weights follow `current_epoch` (0 in the first fit_epoch call, as Lightning's).
        init_c2w: (C, 3|4, 4) initial camera-to-world poses (None: identity, C = len(image_ids) or N_vocab).
        image_ids: the image id of each pose row (the reference's `enumerate(poses_dict.keys())`); default 0 .. C-1.

        optimizer (sgd | adam | radam | ranger), momentum (sgd), weight_decay, lr_scheduler (None | steplr | cosine | poly),
        num_epochs, decay_step, decay_gamma, poly_exp, warmup_multiplier, warmup_epochs: opt.py's flags of the same names
        (make_optimizer / make_scheduler; the scheduler steps once per fit_epoch).  The defaults are this trainer's: Adam
        without weight decay and a constant rate.

        Under a process group of more than one rank the trainer is built as above, then every parameter and buffer of
        `modules` (learn_poses.init_c2w included) is broadcast from rank 0, and the device's default generator and the
        permutation generator are re-seeded with rank_seed(seed, rank) and rank_seed(seed, rank) + 1: every rank starts
        from rank 0's weights and draws its own jitter, noise and importance samples.  Without one, or at world size 1,
        nothing of this happens."""
        self.refine_pose = bool(refine_pose)
        if not self.refine_pose and (init_c2w is not None or image_ids is not None):
            raise ValueError("init_c2w / image_ids are the poses of refine_pose=True")
        if self.refine_pose:
            init_c2w = self._init_poses(init_c2w, image_ids, N_vocab)
            n_cams = init_c2w.shape[0] if init_c2w is not None else (len(image_ids) if image_ids is not None else int(N_vocab))
            ids = list(range(n_cams)) if image_ids is None else [int(i) for i in image_ids]
            if len(ids) != n_cams:
                raise ValueError(f"image_ids has {len(ids)} entries for {n_cams} poses")
            row_of_id = row_table(ids)                 # validates: distinct, >= 0
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("nerf_fl_amd.train.RayTrainer needs a ROCm device (this build has no CPU path)")
        self.use_graph = bool(use_graph)
        self._graphed = None
        self.hp = dict(N_samples=N_samples, N_importance=N_importance, use_disp=use_disp, perturb=perturb,
                       noise_std=noise_std, white_back=white_back)      # GraphedTrainStep's sampling arguments
        self.batch_size = int(batch_size)
        self.seed, self.optimizer_name = int(seed), optimizer
        self._sched_args = dict(name=lr_scheduler, num_epochs=num_epochs, decay_step=decay_step, decay_gamma=decay_gamma,
                                poly_exp=poly_exp, warmup_multiplier=warmup_multiplier, warmup_epochs=warmup_epochs,
                                optimizer=optimizer)
        torch.manual_seed(seed)
        # draws of the backward's stochastic rounding: a function of the trainer's seed, and another stream on every rank
        import torch.distributed as dist
        from .rendering import set_rounding_seed
        set_rounding_seed(seed * 1000003 + (dist.get_rank() if dist.is_initialized() else 0))
        if self.refine_pose:
            self.embeddings = {"xyz": BarfPosEmbedding(N_emb_xyz - 1, N_emb_xyz, 4, 8),
                               "dir": BarfPosEmbedding(N_emb_dir - 1, N_emb_dir, 4, 8)}
        else:
            self.embeddings = {"xyz": PosEmbedding(N_emb_xyz - 1, N_emb_xyz), "dir": PosEmbedding(N_emb_dir - 1, N_emb_dir)}
        self.modules = {}                                   # checkpoint prefix -> module (train.py:48-76)
        if encode_a:
            self.embeddings["a"] = self.modules["embedding_a"] = nn.Embedding(N_vocab, N_a).to(self.dev)
        if encode_t:
            self.embeddings["t"] = self.modules["embedding_t"] = nn.Embedding(N_vocab, N_tau).to(self.dev)
        cx, cd = 6 * N_emb_xyz + 3, 6 * N_emb_dir + 3
        rp = self.refine_pose
        self.models = {"coarse": NeRF("coarse", in_channels_xyz=cx, in_channels_dir=cd, refine_pose=rp).to(self.dev)}
        self.modules["nerf_coarse"] = self.models["coarse"]
        if N_importance > 0:
            self.models["fine"] = NeRF("fine", in_channels_xyz=cx, in_channels_dir=cd, encode_appearance=encode_a,
                                       in_channels_a=N_a, encode_transient=encode_t, in_channels_t=N_tau,
                                       beta_min=beta_min, refine_pose=rp).to(self.dev)
            self.modules["nerf_fine"] = self.models["fine"]
        self.pose = self.row_of_id = self.barf_w = None
        self.current_epoch = 0                              # Lightning's current_epoch: fit_epoch counts it
        self.global_step = 0                                # Lightning's global_step: optimisation steps taken
        self._barf_epoch = None
        if rp:
            self.pose = self.modules["learn_poses"] = LearnPose(n_cams, True, True, init_c2w).to(self.dev)
            self.row_of_id = row_of_id.to(self.dev)
            self.barf_w = (torch.zeros(N_emb_xyz, dtype=torch.float32, device=self.dev),
                           torch.zeros(N_emb_dir, dtype=torch.float32, device=self.dev))
        # trainable parameters only (learn_poses.init_c2w is a frozen Parameter, as in the reference)
        self.params = [p for m in self.modules.values() for p in m.parameters() if p.requires_grad]
        # one-launch optimisers (Adam by default).  (torch's own fused=True Adam is not an option here: it updates the
        # parameters without moving their version counters, so render_rays never re-packed its weight streams and kept rendering with
        # the initial weights -- tests/test_train_gpu.py: validation PSNR 26.89 -> 26.93 instead of 35.9)
        self.opt = make_optimizer(optimizer, self.params, lr=lr, momentum=momentum, weight_decay=weight_decay, eps=1e-8,
                                  capturable=self.use_graph)
        self.sched = make_scheduler(self.opt, lr_scheduler, num_epochs=num_epochs, decay_step=decay_step,
                                    decay_gamma=decay_gamma, poly_exp=poly_exp, warmup_multiplier=warmup_multiplier,
                                    warmup_epochs=warmup_epochs, optimizer=optimizer)
        self.arena = parallel.GradArena(self.params)      # flat gradient memory: written by the backward, all-reduced in place
        self.loss = NerfWLoss()         # its constants, fused into the render kernels (render_rays: loss_target)
        self.gen = torch.Generator(device=self.dev).manual_seed(seed + 1)
        rank, world = _rank_world()
        if world > 1:
            parallel.broadcast_tensors_(self._module_tensors(), src=0)
            self._seed_streams(rank_seed(seed, rank))

    def _seed_streams(self, s):
        torch.manual_seed(s)
        self.gen.manual_seed(s + 1)

    def _module_tensors(self):
        return [t for m in self.modules.values() for t in list(m.parameters()) + list(m.buffers())]

    def param_names(self):
        """Checkpoint names of `params` (the trainable parameters), in their order."""
        return [f"{prefix}.{n}" for prefix, m in self.modules.items() for n, p in m.named_parameters() if p.requires_grad]

    @staticmethod
    def _init_poses(init_c2w, image_ids, n_vocab):
        """(C, 3|4, 4) -> (C, 4, 4) fp32 on the host (convert3x4_4x4, utils/lie_group_helper.py:28-47), validated."""
        if init_c2w is None:
            return None
        c2w = torch.as_tensor(init_c2w).detach().to("cpu", torch.float32)
        if c2w.dim() != 3 or c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4 or c2w.shape[0] < 1:
            raise ValueError(f"init_c2w must be (C, 3|4, 4), got {tuple(c2w.shape)}")
        if c2w.shape[1] == 3:
            c2w = torch.cat([c2w, torch.zeros_like(c2w[:, :1])], 1)
            c2w[:, 3, 3] = 1.0
        return c2w.contiguous()

    def _sync_barf(self):
        """Refill the BARF weight buffers when current_epoch changed (a host -> device copy: outside graph capture)."""
        if self.refine_pose and self._barf_epoch != self.current_epoch:
            fill_barf_weights(self.embeddings, self.current_epoch, self.barf_w)
            self._barf_epoch = self.current_epoch

    def c2w(self, rows):
        """Refined (len(rows), 3, 4) camera-to-world poses of pose rows `rows` (make_c2w(r, t) @ init_c2w), e.g. for
        eval.render_frame."""
        if not self.refine_pose:
            raise RuntimeError("RayTrainer.c2w: poses are learned only with refine_pose=True")
        rows = torch.as_tensor(rows, dtype=torch.int64, device=self.dev).reshape(-1)
        with torch.no_grad():
            return self.pose(rows)[:, :3].clone()

    # ---- one optimisation step on a ready batch ------------------------------------------------
    def step(self, rays, rgbs, ts):
        """rays: (R, 8) world rays, or with refine_pose the training layout (camera-frame direction, near, far, ...)."""
        self.arena.attach()          # parameters the backward never reaches keep the zeros the arena was created with
        self._sync_barf()
        out = _loss_backward(self.models, self.embeddings, self.hp, rays, ts, rgbs, self.arena, loss_coef=self.loss.coef,
                             lambda_u=self.loss.lambda_u, pose=self.pose, row_of_id=self.row_of_id, barf_weights=self.barf_w)
        self.arena.all_reduce()
        self.opt.step()
        self.global_step += 1
        return out

    # ---- one epoch over device-resident data (this rank's shard) -------------------------------
    def fit_epoch(self, rays, rgbs=None, ts=None):
        """One epoch over (rays, rgbs, ts) tensors (this rank's shard, in a random order drawn from the trainer's
        permutation generator), or fit_epoch(bank) over a data.ImageBank: the order is the computed permutation keyed
        by data.epoch_key(seed, current_epoch), the same on every rank (build the ranks with the same `seed`); step s of
        rank r of P takes its positions [(s P + r) bs, (s P + r + 1) bs), n_pixels // (bs P) steps, the tail dropped."""
        from .data import ImageBank
        if isinstance(rays, ImageBank):
            if rgbs is not None or ts is not None:
                raise ValueError("fit_epoch(bank) takes the bank alone")
            return self._fit_epoch_bank(rays)
        n, bs = rays.shape[0], self.batch_size
        perm = torch.randperm(n, device=self.dev, generator=self.gen)
        log = []
        self._sync_barf()
        for i in range(0, n - bs + 1, bs):
            idx = perm[i:i + bs]
            if self.use_graph:
                if self._graphed is None:
                    self._graphed = self.graphed_step(rays[idx], ts[idx], rgbs[idx])
                self._graphed.load(rays[idx], ts[idx], rgbs[idx])
                log.append(tuple(x.clone() for x in self._graphed.replay()))      # the outputs live in the graph's pool
                self.global_step += 1
            else:
                log.append(self.step(rays[idx], rgbs[idx], ts[idx]))
        self._end_epoch()
        return torch.stack([torch.stack(x) for x in log]).mean(0).tolist() if log else [math.nan, math.nan]

    def _end_epoch(self):
        if self.sched is not None:
            self.sched.step()
        self.current_epoch += 1
        from .rendering import check_status
        check_status(self.dev)              # fp16 range audit of the epoch's render passes (raises FloatingPointError)

    def _fit_epoch_bank(self, bank):
        from .data import batch_range, epoch_key
        rank, world = _rank_world()
        bs, key = self.batch_size, epoch_key(self.seed, self.current_epoch)
        layout = "camera" if self.refine_pose else "world"
        steps = bank.n_pixels // (bs * world)
        total = torch.zeros(2, dtype=torch.float32, device=self.dev)     # a running sum: nothing grows with the epoch
        self._sync_barf()
        for s in range(steps):
            start = batch_range(s, rank, world, bs)
            if self.use_graph:
                if self._graphed is None:
                    rays, rgbs, ts = bank.gather(start, bs, key, layout)
                    self._graphed = self.graphed_step(rays, ts, rgbs)
                g = self._graphed
                bank.gather(start, bs, key, layout, out=(g.rays, g.target, g.ts))   # one launch into the static buffers
                total += torch.stack(g.replay())
                self.global_step += 1
            else:
                rays, rgbs, ts = bank.gather(start, bs, key, layout)
                total += torch.stack(self.step(rays, rgbs, ts))
        self._end_epoch()
        return (total / steps).tolist() if steps else [math.nan, math.nan]

    def graphed_step(self, rays, ts, rgbs, **kw):
        """The GraphedTrainStep fit_epoch replays (use_graph=True), captured on this batch; `kw` go to GraphedTrainStep."""
        import torch.distributed as dist
        self._sync_barf()
        return GraphedTrainStep(
            self.models, self.embeddings, self.params, self.opt, None, rays, ts, rgbs, **self.hp,
            all_reduce=dist.is_initialized() and dist.get_world_size() > 1,
            loss_coef=self.loss.coef, lambda_u=self.loss.lambda_u, arena=self.arena,
            pose=self.pose, row_of_id=self.row_of_id, barf_weights=self.barf_w, **kw)

    @torch.no_grad()
    def validate(self, rays, rgbs, ts, chunk=32768, shard=False):
        """Mean PSNR of a deterministic render (perturb 0, noise 0; train.py:176-210).  rays: (R, 8) world rays; with
        refine_pose, any other width is the training layout and is rendered through the learned poses.
        shard=True under a process group: every rank renders its parallel.shard_bounds slice, the squared error and the
        element count are summed over the ranks with one fp64 all-reduce, and every rank returns the same PSNR.  Every
        rank must pass the same rays."""
        rank, world = _rank_world()
        if not (shard and world > 1):
            return float(psnr(self._render_eval(rays, ts, chunk), rgbs))
        import torch.distributed as dist
        lo, hi = parallel.shard_bounds(rays.shape[0], rank, world)
        pred = self._render_eval(rays[lo:hi], ts[lo:hi], chunk) if hi > lo else rgbs[:0]
        acc = torch.stack([((pred.double() - rgbs[lo:hi].double()) ** 2).sum(),
                           torch.tensor(float(pred.numel()), dtype=torch.float64, device=pred.device)])
        dist.all_reduce(acc)
        sse, n = acc.tolist()
        return -10.0 * math.log10(sse / n)

    def validate_bank(self, bank, images=None, chunk=32768, shard=False):
        """(mean PSNR, mean SSIM) over the images `images` (default all) of a data.ImageBank, rendered deterministically
        and scored on the device by eval.evaluate_bank (full images, predictions not clipped, as train.py:196-207).
        With refine_pose the images are rendered through the learned poses of their ids.
        shard=True under a process group: every rank renders its parallel.shard_bounds block of the images, the tables are
        summed with one all-reduce, and every rank returns the same means."""
        from .eval import evaluate_bank
        rank, world = _rank_world()
        if not (shard and world > 1):
            rank, world = 0, 1
        idx = list(range(bank.n_images)) if images is None else [int(i) for i in images]
        kw = dict(use_disp=self.hp["use_disp"], white_back=self.hp["white_back"], chunk=chunk)
        poses = None
        if self.refine_pose:
            self._sync_barf()
            ids = torch.as_tensor(bank.host_table["id"][idx].astype("int64"), device=self.dev)
            poses = self.c2w(self.row_of_id[ids])
            kw["barf_weights"] = self.barf_w
        res = evaluate_bank(self.models, self.embeddings, bank, self.hp["N_samples"], self.hp["N_importance"], images=idx,
                            clip=False, rank=rank, world=world, poses=poses, **kw)
        if world == 1:
            return res["mean_psnr"], res["mean_ssim"]
        import torch.distributed as dist
        table = res["table"]
        dist.all_reduce(table)
        host = table.cpu()
        return float(host[:, 5].mean()), float(host[:, 7].mean())

    def _render_eval(self, rays, ts, chunk):
        hp = self.hp
        self._sync_barf()
        outs = []
        for _, _, r, t, _ in _chunks(rays, ts, chunk):
            if self.refine_pose and r.shape[1] != 8:      # the training layout, through the learned poses
                r = posed_rays(self.pose, r, t, self.row_of_id)
            res = render_rays(self.models, self.embeddings, r, t, hp["N_samples"], hp["use_disp"], 0, 0,
                              hp["N_importance"], chunk, hp["white_back"], False, barf_weights=self.barf_w)
            outs.append(res["rgb_fine" if "rgb_fine" in res else "rgb_coarse"])
        return torch.cat(outs)

    # ---- checkpoints with the reference's key prefixes -----------------------------------------
    def state_dict(self):
        return {f"{prefix}.{k}": v for prefix, m in self.modules.items() for k, v in m.state_dict().items()}

    def load_state_dict(self, sd):
        """Accepts this harness' checkpoints and Lightning checkpoints' `state_dict` (prefix-stripped per
        module exactly as utils.extract_model_state_dict does)."""
        sd = sd.get("state_dict", sd)
        for prefix, m in self.modules.items():
            sub = {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}
            m.load_state_dict(sub, strict=True)

    def save(self, path, epoch=0):
        """Write a full-state checkpoint.  `epoch` and `state_dict` are what load() and the reference's utils.load_ckpt
        read.  Lightning 1.2's keys come with them: `global_step`, `optimizer_states` (one element: opt.state_dict(),
        indexed in `params` order) and `lr_schedulers` (the scheduler's state dict, or empty).  `nerf_fl_amd` holds the
        rest resume() needs: current_epoch, the saving rank's generator states and rounding seed, the optimiser and
        schedule names and the world size.  Under a process group only rank 0 writes, and every rank returns once it
        has written (an error on rank 0 is raised on every rank)."""
        from . import rendering
        rank, world = _rank_world()
        err = None
        if rank == 0:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                own = dict(current_epoch=self.current_epoch, global_step=self.global_step, world_size=world,
                           optimizer=self.optimizer_name, lr_scheduler=self._sched_args["name"], seed=self.seed,
                           rng=dict(cpu=torch.get_rng_state(), device=torch.cuda.get_rng_state(self.dev),
                                    perm=self.gen.get_state(), rounding_seed=rendering._rounding_seed))
                torch.save({"epoch": epoch, "state_dict": self.state_dict(), "global_step": self.global_step,
                            "optimizer_states": [self.opt.state_dict()],
                            "lr_schedulers": [] if self.sched is None else [self.sched.state_dict()],
                            "nerf_fl_amd": own}, path)
            except Exception as e:           # noqa: BLE001 -- re-raised below, after the other ranks have heard of it
                err = e
        self._agree(err)

    def load(self, path):
        self.load_state_dict(torch.load(path, map_location=self.dev, weights_only=True))

    # ---- resuming a run -----------------------------------------------------------------------------------------
    def resume(self, path, start_epoch=None, weights_only=True):
        """Continue the run a checkpoint was written by: weights, optimiser state (copied into the existing state
        tensors, device-side step counters reset in place), schedule position, current_epoch (the BARF weights follow
        at the next step), global_step and, at world size 1, the generator states and the rounding seed.  Everything
        is restored in place, so a GraphedTrainStep captured before keeps replaying on live memory.

        Accepts save()'s checkpoints and the reference's Lightning checkpoints (train.py, `--ckpt_path`).  For the
        latter the optimiser state is mapped by name (reference_parameter_names), the schedule is rebuilt by stepping a
        fresh scheduler `start_epoch` times, and `start_epoch` defaults to the checkpoint's `epoch`, read as the next
        epoch to run (unverified).  An explicit `start_epoch` overrides the epoch of either kind.
        weights_only=False: for trusted checkpoints that hold other objects (Lightning's hyper_parameters).

        Under a process group rank 0 reads the file and broadcast() hands everything to the other ranks, which never
        open it; they re-seed their streams with rank_seed(seed, rank, current_epoch).  The captured rounding seed of a
        graph is a kernel argument: a step captured before resume() keeps the seed it was captured with."""
        rank, world = _rank_world()
        if world == 1:
            self._restore(path, start_epoch, weights_only)
            return
        err = None
        if rank == 0:
            try:
                self._restore(path, start_epoch, weights_only)
            except Exception as e:           # noqa: BLE001 -- raised on every rank by _broadcast
                err = e
        self._broadcast(0, err)
        if rank != 0:
            self._seed_streams(rank_seed(self.seed, rank, self.current_epoch))

    def _restore(self, path, start_epoch, weights_only):
        import warnings

        from . import rendering
        ck = torch.load(path, map_location="cpu", weights_only=weights_only)
        own = ck.get("nerf_fl_amd")
        if "optimizer_states" not in ck:
            raise ValueError(f"{path}: no optimizer_states (a weights-only checkpoint: use load())")
        if own is not None:
            for key, mine in (("optimizer", self.optimizer_name), ("lr_scheduler", self._sched_args["name"])):
                if own[key] != mine:
                    raise ValueError(f"{path} was written with {key}={own[key]!r}, this trainer has {mine!r}")
        self.load_state_dict(ck)
        if own is not None:
            self.opt.load_state_dict(ck["optimizer_states"][0])
            epoch = own["current_epoch"] if start_epoch is None else int(start_epoch)
            if self.sched is not None and start_epoch is None and ck["lr_schedulers"]:
                self.sched.load_state_dict(ck["lr_schedulers"][0])
            else:
                self._replay_schedule(epoch)
            self.global_step = int(own["global_step"])
        else:
            self.opt.load_state_dict(self._from_reference_optimizer(ck["optimizer_states"][0]))
            epoch = int(ck["epoch"]) if start_epoch is None else int(start_epoch)
            self._replay_schedule(epoch)
            self.global_step = int(ck.get("global_step", 0))
        self.current_epoch = epoch
        rng = own["rng"] if own is not None else None
        if rng is None:                          # e.g. a Lightning checkpoint: streams re-derived
            self._seed_streams(rank_seed(self.seed, _rank_world()[0], epoch))
        else:
            torch.set_rng_state(rng["cpu"])
            torch.cuda.set_rng_state(rng["device"], self.dev)
            self.gen.set_state(rng["perm"])
            rendering.set_rounding_seed(rng["rounding_seed"])
            if (self._graphed is not None and self._graphed.rounding_seed != rendering._rounding_seed
                    and rendering.get_backward_precision() != "f16x3"):
                warnings.warn("RayTrainer.resume: the captured step keeps the rounding seed it was captured with "
                              f"({self._graphed.rounding_seed}, checkpoint {rendering._rounding_seed})")

    def _replay_schedule(self, epoch):
        """Put the schedule at `epoch` by stepping a fresh one that many times (the schedules are deterministic in the
        epoch count; a scheduler of another implementation, the reference's GradualWarmupScheduler, need not load)."""
        import warnings
        if self.sched is None:
            return
        for g in self.opt.param_groups:
            g["lr"] = g.get("initial_lr", g["lr"])
        self.sched = make_scheduler(self.opt, **self._sched_args)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")       # lr_scheduler.step() before optimizer.step()
            for _ in range(int(epoch)):
                self.sched.step()

    def _from_reference_optimizer(self, osd):
        """The reference's optimizer state dict (one group over get_parameters order, frozen tensors included) as one
        over `params`, matched by name."""
        names = reference_parameter_names(self.modules)
        groups = osd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(names):
            raise ValueError(f"the checkpoint's optimiser has {[len(g['params']) for g in groups]} parameters; this "
                             f"trainer's configuration has {len(names)} in the reference's order")
        ours = {n: i for i, n in enumerate(self.param_names())}
        state = {}
        for name, pid in zip(names, groups[0]["params"]):
            st = osd["state"].get(pid)
            if not st:
                continue
            if name not in ours:
                raise ValueError(f"the checkpoint has optimiser state for {name}, which this trainer does not train")
            p = self.params[ours[name]]
            for k, v in st.items():
                if torch.is_tensor(v) and v.dim() > 0 and v.shape != p.shape:
                    raise ValueError(f"optimiser state {name}.{k}: shape {tuple(v.shape)}, parameter {tuple(p.shape)}")
            state[ours[name]] = st
        missing = [n for n, i in ours.items() if i not in state]
        if state and missing:
            raise ValueError(f"the checkpoint has no optimiser state for {missing[0]} (another configuration?)")
        group = dict(groups[0], params=list(range(len(self.params))))
        return {"state": state, "param_groups": [group]}

    # ---- keeping the ranks identical ------------------------------------------------------------------------------
    def broadcast(self, src=0):
        """Make every rank's trainer rank `src`'s: parameters and buffers of `modules`, optimiser state (the per-parameter
        tensors and steps, the param groups' hyper-parameters, the capturable optimisers' device-side step and
        hyper-parameter tensors), scheduler state, current_epoch and global_step.  Tensors travel through
        parallel.broadcast_tensors_ (one collective per dtype: fp32 and, with a capturable optimiser, int32), the rest
        through one dist.broadcast_object_list.  Every copy is in place, so a step captured before keeps replaying on
        live memory.  Use it after a load() that only one rank performed.  A no-op without a process group."""
        self._broadcast(src, None)

    def _agree(self, err, src=0):
        """Rank `src`'s error, raised on every rank (doubles as the barrier of save())."""
        rank, world = _rank_world()
        if world > 1:
            import torch.distributed as dist
            box = [None if err is None else f"{type(err).__name__}: {err}"]
            dist.broadcast_object_list(box, src=src)
            if box[0] is not None and err is None:
                raise RuntimeError(f"RayTrainer: rank {src} failed: {box[0]}")
        if err is not None:
            raise err

    def _broadcast(self, src, err):
        import torch.distributed as dist
        rank, world = _rank_world()
        if world == 1:
            if err is not None:
                raise err
            return
        opt, pdev = self.opt, self.params[0].device         # the optimiser's device-side state is keyed by p.device
        meta = None
        if rank == src and err is None:
            state = []
            for p in self.params:
                st = opt.state.get(p) or {}
                state.append(dict(scalars={k: v for k, v in st.items() if not torch.is_tensor(v)},
                                  tensors=[(k, tuple(v.shape), str(v.dtype).split(".")[-1])
                                           for k, v in sorted(st.items()) if torch.is_tensor(v)]) if st else None)
            meta = dict(epoch=self.current_epoch, global_step=self.global_step, state=state,
                        groups=[{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups],
                        sched=None if self.sched is None else self.sched.state_dict(),
                        dev_groups=opt.device_state(pdev)[0])
        box = [dict(error=None if err is None else f"{type(err).__name__}: {err}", meta=meta)]
        dist.broadcast_object_list(box, src=src)
        if box[0]["error"] is not None:
            if err is not None:
                raise err
            raise RuntimeError(f"RayTrainer: rank {src} failed: {box[0]['error']}")
        meta = box[0]["meta"]
        if rank != src:
            self.current_epoch, self.global_step = meta["epoch"], meta["global_step"]
            for g, h in zip(opt.param_groups, meta["groups"]):
                g.update(h)
            for p, m in zip(self.params, meta["state"]):
                if m is None:
                    opt.state.pop(p, None)
                    continue
                st = opt.state[p]
                st.update(m["scalars"])
                for k, shape, dtype in m["tensors"]:
                    if not torch.is_tensor(st.get(k)) or tuple(st[k].shape) != shape:
                        st[k] = torch.empty(shape, dtype=getattr(torch, dtype), device=pdev)
            if self.sched is not None and meta["sched"] is not None:
                self.sched.load_state_dict(meta["sched"])
        tensors = self._module_tensors()
        for p, m in zip(self.params, meta["state"]):
            if m is not None:
                tensors += [opt.state[p][k] for k, _, _ in m["tensors"]]
        # the next sync_hyper() re-uploads from the (now common) param groups
        tensors += opt.device_state(pdev, meta["dev_groups"])[1]
        parallel.broadcast_tensors_(tensors, src=src)
