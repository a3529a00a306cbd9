"""Time appearance-code fitting (nerf_fl_amd.appearance) against the render_rays + autograd route (run on the GPU box;
not a test).  Prints one line per measurement: cache build, fit iteration eager / graphed, and the slow route with the
'f16' and the 'f16x3' backward, at 4096 rays and at a 320 000-ray half image, 64 + 64 samples, the routes alternated."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nerf_fl_amd
from nerf_fl_amd import NeRF, PosEmbedding, render_rays
from nerf_fl_amd.appearance import AppearanceFit
from nerf_fl_amd.train import Adam
from oracle import nerfw_oracle as orc

dev = torch.device("cuda", 0)
S = I = 64
sizes = [int(x) for x in sys.argv[1:]] or [4096, 320000]
models = {}
for typ, seed in (("coarse", 11), ("fine", 12)):
    spec = orc.FieldSpec(typ, encode_appearance=typ == "fine")
    m = NeRF(typ, encode_appearance=typ == "fine", in_channels_a=48, encode_transient=False)
    m.load_state_dict(orc.make_field_params(spec, seed, "sharp"))
    models[typ] = m.to(dev)
    for p in m.parameters():
        p.requires_grad_(False)
emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
ev = lambda: torch.cuda.Event(enable_timing=True)


def timed(fn, reps):
    e0, e1 = ev(), ev()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for R in sizes:
    rays = orc.make_rays(R, 100).to(dev)
    target = torch.rand(R, 3, device=dev)
    idx = torch.randint(0, 4, (R,), device=dev)
    init = torch.randn(4, 48, device=dev)
    e0, e1 = ev(), ev()
    torch.cuda.synchronize()
    e0.record()
    fit = AppearanceFit(models, emb, rays, target, idx, S, I, init=init, lr=1e-3)
    e1.record()
    torch.cuda.synchronize()
    print(f"R={R}: cache build {e0.elapsed_time(e1):.2f} ms (first call, includes packing)", flush=True)
    codes = torch.nn.Parameter(init.clone())
    opt = Adam([codes], lr=1e-3)

    def slow():
        opt.zero_grad()
        res = render_rays(models, emb, rays, None, S, False, 0, 0, I, 32768, False, False, output_transient=False,
                          a_embedded=codes[idx], z_fine=fit.z_sorted)
        ((res["rgb_fine"] - target) ** 2).mean().backward()
        opt.step()

    fit.fit(3)                       # warm-up, and the graph
    fit.fit(2, use_graph=True)
    slow_reps = 10
    for rnd_ in range(2):            # the routes alternated
        t_e = timed(fit.step, 50)
        t_g = timed(lambda: fit.fit(1, use_graph=True), 50)
        out = {}
        if R <= 65536:               # the training route stashes ~1.4 MB per ray: a half image does not fit in one call
            for bwd in ("f16", "f16x3"):
                nerf_fl_amd.set_precision("f16x3", backward=bwd)
                slow()
                out[bwd] = f"{timed(slow, slow_reps):.3f} ms"
            nerf_fl_amd.set_precision("f16x3", backward="f16")
        print(f"R={R} round {rnd_}: fit eager {t_e * 1e3:.1f} us, graphed {t_g * 1e3:.1f} us | render_rays+autograd "
              f"f16 {out.get('f16', 'not measured')}, f16x3 {out.get('f16x3', 'not measured')}", flush=True)
    del fit
    torch.cuda.empty_cache()
