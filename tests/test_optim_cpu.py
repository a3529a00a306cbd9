"""CPU checks of the one-launch optimisers and the schedules: argument validation of nfl_optim_step / nfl_optim_step_dev
(no kernel is launched; nfl_optim_tensors and the NFL_OPT_* constants are held to the header in tests/test_abi_cpu.py), and
make_scheduler against learning-rate sequences recorded from the reference's own warm-up scheduler
(tests/golden/make_sched_golden.py)."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

from abi_probe import L  # noqa: F401  (a fixture)
from nerf_fl_amd import _lib
from nerf_fl_amd.train import SGD, Adam, GradualWarmupLR, RAdam, Ranger, make_optimizer, make_scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g21_lr_schedules.npz")


def _hyper(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, alpha=0.5, k=6.0, thr=5.0):
    return (C.c_float * _lib.NFL_OPT_HYPER)(lr, b1, b2, eps, wd, alpha, k, thr)


def _tensors(n, kind, drop=None):
    """n non-empty tensors with (fake, never dereferenced) pointers for every state `kind` needs, minus field `drop`."""
    t = _lib.OptimTensors()
    for i in range(n):
        t.param[i], t.grad[i], t.numel[i] = 16, 16, 4
        t.state0[i] = 16
        if kind != _lib.NFL_OPT_SGD:
            t.state1[i] = 16
        if kind == _lib.NFL_OPT_RANGER:
            t.state2[i] = 16
    if drop is not None:
        getattr(t, drop)[n - 1] = None
    return t


@pytest.mark.parametrize("kind,drop", [(_lib.NFL_OPT_SGD, "state0"), (_lib.NFL_OPT_ADAM, "state0"),
                                       (_lib.NFL_OPT_ADAM, "state1"), (_lib.NFL_OPT_RADAM, "state1"),
                                       (_lib.NFL_OPT_RANGER, "state2"), (_lib.NFL_OPT_RANGER, "param")])
def test_optim_step_rejects_a_missing_pointer(L, kind, drop):
    t = _tensors(3, kind, drop)
    assert L.nfl_optim_step(C.byref(t), 3, kind, _hyper(), 1, None) == -1                             # NFL_EINVAL
    if drop != "state0" or kind != _lib.NFL_OPT_SGD:          # SGD without a buffer is plain SGD in the device form
        assert L.nfl_optim_step_dev(C.byref(t), 3, kind, C.c_void_p(16), C.c_void_p(16), 1, None) == -1


def test_optim_step_validates_arguments(L):
    t = _tensors(2, _lib.NFL_OPT_RANGER)
    h = _hyper()
    for kind in range(4):
        assert L.nfl_optim_step(None, 1, kind, h, 1, None) == -1                                  # no tensors
        assert L.nfl_optim_step(C.byref(t), 1, kind, None, 1, None) == -1                         # no hyper-parameters
        assert L.nfl_optim_step(C.byref(t), 1, kind, h, 0, None) == -1                            # steps are 1-based
        assert L.nfl_optim_step(C.byref(t), -1, kind, h, 1, None) == -1
        assert L.nfl_optim_step(C.byref(t), _lib.NFL_ADAM_MAX_TENSORS + 1, kind, h, 1, None) == -1
        assert L.nfl_optim_step(C.byref(_lib.OptimTensors()), 0, kind, h, 1, None) == 0          # nothing to do
    for kind in (-1, 4):
        assert L.nfl_optim_step(C.byref(t), 1, kind, h, 1, None) == -1                            # unknown kind
    assert L.nfl_optim_step(C.byref(t), 1, _lib.NFL_OPT_RANGER, _hyper(k=0.0), 1, None) == -1   # lookahead k < 1
    assert L.nfl_optim_step(C.byref(t), 1, _lib.NFL_OPT_SGD, _hyper(b1=-0.5), 1, None) == -1    # negative momentum
    sgd = _tensors(1, _lib.NFL_OPT_SGD, "state0")
    assert L.nfl_optim_step(C.byref(sgd), 1, _lib.NFL_OPT_SGD, _hyper(b1=0.9), 1, None) == -1   # momentum, no buffer
    t.numel[0] = -1
    assert L.nfl_optim_step(C.byref(t), 1, _lib.NFL_OPT_ADAM, h, 1, None) == -1


def test_optim_step_dev_validates_arguments(L):
    t = _tensors(2, _lib.NFL_OPT_RANGER)
    d = C.c_void_p(16)
    for kind in range(4):
        assert L.nfl_optim_step_dev(None, 1, kind, d, d, 1, None) == -1
        assert L.nfl_optim_step_dev(C.byref(t), 1, kind, None, d, 1, None) == -1                  # hyper-parameters
        assert L.nfl_optim_step_dev(C.byref(t), 1, kind, d, None, 1, None) == -1                  # step counter
        assert L.nfl_optim_step_dev(C.byref(t), _lib.NFL_ADAM_MAX_TENSORS + 1, kind, d, d, 1, None) == -1
        assert L.nfl_optim_step_dev(C.byref(_lib.OptimTensors()), 0, kind, d, d, 1, None) == 0
    assert L.nfl_optim_step_dev(C.byref(t), 1, 4, d, d, 1, None) == -1


def test_version_string_names_the_abi(L):
    assert f"abi {_lib.NFL_ABI_VERSION})".encode() in L.nfl_version()


# ---- schedules ---------------------------------------------------------------------------------------------------
def _lrs(opt, sched, epochs):
    out = []
    for _ in range(epochs):
        out.append(opt.param_groups[0]["lr"])
        if sched is not None:
            sched.step()
    return np.array(out)


def _torch_opt(name, lr):
    p = torch.nn.Parameter(torch.zeros(3))
    return torch.optim.SGD([p], lr=lr, momentum=0.9) if name == "sgd" else torch.optim.Adam([p], lr=lr, eps=1e-8)


@pytest.mark.parametrize("opt_name", ["sgd", "adam"])
@pytest.mark.parametrize("sched_name", ["steplr", "cosine"])
@pytest.mark.parametrize("warmup_epochs", [0, 3])
@pytest.mark.parametrize("multiplier", [1, 2])
def test_schedules_match_the_reference(opt_name, sched_name, warmup_epochs, multiplier):
    g = np.load(GOLDEN)
    meta = json.loads(bytes(g["meta"]).decode())
    opt = _torch_opt(opt_name, meta["lr"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # lr_scheduler.step() without optimizer.step()
        sched = make_scheduler(opt, sched_name, num_epochs=meta["num_epochs"], decay_step=meta["decay_step"],
                               decay_gamma=meta["decay_gamma"], warmup_multiplier=multiplier,
                               warmup_epochs=warmup_epochs, optimizer=opt_name)
        got = _lrs(opt, sched, meta["num_epochs"])
    assert isinstance(sched, GradualWarmupLR) == (warmup_epochs > 0)
    np.testing.assert_allclose(got, g[f"{opt_name}_{sched_name}_w{warmup_epochs}_m{multiplier}"], rtol=1e-12, atol=0)


def test_poly_is_the_closed_form():
    opt = _torch_opt("adam", 5e-4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = _lrs(opt, make_scheduler(opt, "poly", num_epochs=20, poly_exp=0.9), 20)
    np.testing.assert_allclose(got, [5e-4 * (1 - e / 20) ** 0.9 for e in range(20)], rtol=1e-12)


def test_poly_with_warmup_hands_over_at_the_scaled_rate():
    opt = _torch_opt("sgd", 1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = _lrs(opt, make_scheduler(opt, "poly", num_epochs=10, poly_exp=2.0, warmup_multiplier=2.0, warmup_epochs=2,
                                       optimizer="sgd"), 10)
    # warm-up 1e-3, 1.5e-3, 2e-3; then LambdaLR from its own epoch 0 on base lrs x 2
    exp = [1e-3, 1.5e-3, 2e-3] + [2e-3 * (1 - e / 10) ** 2.0 for e in range(7)]
    np.testing.assert_allclose(got, exp, rtol=1e-12)


@pytest.mark.parametrize("opt_name", ["radam", "ranger"])
def test_warmup_is_ignored_for_radam_and_ranger(opt_name):
    a, b = _torch_opt("adam", 5e-4), _torch_opt("adam", 5e-4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sa = make_scheduler(a, "cosine", num_epochs=20, warmup_multiplier=2.0, warmup_epochs=3, optimizer=opt_name)
        sb = make_scheduler(b, "cosine", num_epochs=20)
        assert not isinstance(sa, GradualWarmupLR)
        np.testing.assert_array_equal(_lrs(a, sa, 20), _lrs(b, sb, 20))


def test_unknown_names_raise():
    opt = _torch_opt("adam", 5e-4)
    with pytest.raises(ValueError, match="scheduler not recognized"):
        make_scheduler(opt, "exponential")
    with pytest.raises(ValueError, match="optimizer not recognized"):
        make_scheduler(opt, "cosine", optimizer="adagrad")
    with pytest.raises(ValueError, match="optimizer not recognized"):
        make_optimizer("adagrad", [torch.nn.Parameter(torch.zeros(2))])
    with pytest.raises(ValueError):
        GradualWarmupLR(opt, 0.5, 3)
    assert make_scheduler(opt, None) is None


def test_make_optimizer_builds_the_reference_configuration():
    ps = [torch.nn.Parameter(torch.zeros(2))]
    o = make_optimizer("sgd", ps, lr=0.1, momentum=0.9, weight_decay=1e-4)
    assert type(o) is SGD and o.defaults == dict(lr=0.1, momentum=0.9, weight_decay=1e-4, dampening=0, nesterov=False)
    o = make_optimizer("adam", ps, lr=5e-4, weight_decay=1e-4)
    assert type(o) is Adam and o.defaults["eps"] == 1e-8 and o.defaults["weight_decay"] == 1e-4
    o = make_optimizer("radam", ps, lr=5e-4)
    assert type(o) is RAdam and o.defaults["betas"] == (0.9, 0.999) and o.defaults["eps"] == 1e-8
    o = make_optimizer("ranger", ps, lr=5e-4, capturable=True)
    assert type(o) is Ranger and o.capturable and o.defaults["betas"] == (0.95, 0.999)
    assert (o.defaults["alpha"], o.defaults["k"], o.defaults["N_sma_threshhold"]) == (0.5, 6, 5)
