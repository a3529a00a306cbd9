"""Time the individual kernels of one cfg-2 train step (run on the GPU box; not a test)."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nerf_fl_amd
from nerf_fl_amd import NeRF, PosEmbedding, _lib
from nerf_fl_amd import rendering as rnd
from oracle import nerfw_oracle as orc

dev = torch.device("cuda", 0)
R, S, F = 4096, 64, 128
prec = sys.argv[1] if len(sys.argv) > 1 else "f16x3"
nerf_fl_amd.set_precision(prec)
m = NeRF("fine")
m.load_state_dict(orc.make_field_params(orc.FieldSpec("fine"), 12, "sharp"))
m = m.to(dev)
f = rnd._field(m, 10, 4, dev)
BWD = sys.argv[sys.argv.index("--backward") + 1] if "--backward" in sys.argv else "f16"      # f16 | f16x3
nerf_fl_amd.set_precision(backward=BWD)
BP = rnd._BPREC[BWD]
f.ensure_bwd_packed(False, BP)
rays = orc.make_rays(R, 100).to(dev)
z = torch.sort(2 + 4 * torch.rand(R, F, device=dev), dim=1)[0]
noise = torch.randn(R, F, device=dev)


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


print(f"precision {prec}; fine pass {R} rays x {F} samples")
print("fwd  (inference)      %.3f ms" % timeit(lambda: rnd._run_pass(f, rays, F, z=z, noise=noise, noise_std=1.0, white_back=True)))
if prec == "f16x3":
    out = {}
    def fwd_stash():
        out.update(rnd._run_pass(f, rays, F, z=z, noise=noise, noise_std=1.0, white_back=True, stash=True, bprec=BP))
    print("fwd  (training stash) %.3f ms" % timeit(fwd_stash))
    act = out["act_stash"]
    up = [None, None, torch.randn(R, 3, device=dev) * 1e-3] + [None] * 5          # d rgb_fine only
    L = _lib.lib()
    # every buffer a timed call touches exists before it: the wrappers allocate nothing then
    head = torch.empty(R * F, 9, device=dev)
    gmax = torch.zeros(1024, device=dev)
    grad_stash = torch.empty(L.nfl_grad_stash_bytes(C.byref(f.desc), R, F, BP), dtype=torch.uint8, device=dev)
    print("composite backward    %.3f ms" % timeit(lambda: rnd._run_compbwd(
        out["field_raw"], z, R, F, noise=noise, noise_std=1.0, use_t=False, white_back=True, grads=up, go=None,
        g_tsig_const=0.0, head=head, gmax=gmax)))
    print("dgrad                 %.3f ms" % timeit(lambda: rnd._run_dgrad(
        f, act, head, gmax, R, F, use_t=False, bprec=BP, grad_stash=grad_stash)))
    plist = f.param_list()
    arena = torch.zeros(sum(w.numel() + b.numel() for _, w, b in plist), device=dev)
    targets, off = {}, 0
    for i, w, b in plist:
        targets[i] = (arena[off:off + w.numel()], arena[off + w.numel():off + w.numel() + b.numel()])
        off += w.numel() + b.numel()
    scratch = torch.empty(L.nfl_wgrad_scratch_bytes() // 4, device=dev)
    print("wgrad                 %.3f ms" % timeit(lambda: rnd._run_wgrad(
        f, act, grad_stash, gmax, R, F, use_t=False, bprec=BP, targets=targets, scratch=scratch)))
    print("act stash %.2f GB, grad stash %.2f GB" % (act.numel() / 1e9, grad_stash.numel() / 1e9))
