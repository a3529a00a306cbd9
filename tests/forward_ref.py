"""References and comparisons for the training forward (nfl_render_kernel in NFL_MODE_STASH / NFL_MODE_STASH2) and the
inference passes (NFL_MODE_RENDER, NFL_MODE_EMBED) on their own.  A plain helper (no pytest hooks) of
tests/test_forward_gpu.py, tests/test_inference_gpu.py and tests/test_forward_refs_cpu.py; everything but the runners
(`run_forward`, `run_render`, `run_embed`) works without a GPU.

* the launch geometry: `ray_split` restates nfl_ray_split (csrc/nfl_launch.cpp), `tiling` / `situation_violations` say what
  a shape makes of it on a device with a given number of CUs;
* Part A: `int_params` / `int_inputs` / `int_reference` / `exactness_violations` -- a field and inputs on which every
  pre-activation is an exact dyadic number, and the conditions under which that is true and proves something;
* the runner: `run_forward` (the stash inside a sentinel-filled arena), `decode`, `unwritten`, `mismatches`;
* Part B: `layer_table`, `check_layers` (three-product prediction from the DECODED operands, hard bound, mask, split and
  discrimination rules) and `emulate_forward`, an fp32 CPU stand-in for the kernel that writes real stash bytes;
* Part C: `composite_ref`, float64 compositing of the pass's own field outputs with the bounds the issue derives;
* the inference passes (tests/test_inference_gpu.py): `run_render` (NFL_MODE_RENDER) and `run_embed` (NFL_MODE_EMBED) with
  every output in a guarded NaN arena, `int_embedded` and `fp16_weight_violations` for Part A on the single-product kernels,
  `bit_differences`, and `x1_forward` / `x1_conditions` / `x1_rule`: the single-product arithmetic in float64, the
  unrounded network, and the rule that holds the kernel between them.

The stash formats come from tests/stash_codec.py, float64 compositing from tests/compbwd_ref.py.
"""
import ctypes as C
import os
import re

import torch

import compbwd_ref as cr
import stash_codec as sc
from oracle import nerfw_oracle as orc

W = 256
U24 = 2.0 ** -24
NSLOT = 4                    # segments of 32 samples per tile of the three-product kernel: one per wave
SENT16 = 0x7E5A              # fp16 NaN with a payload: no pass produces it (the conversions give 0x7e00 or 0xfe00)
SENT32 = 0x7E5A7E5A          # ... and no relu-mask word either: a mask word only has even bits
GUARD = 8192                 # bytes before and behind the activation stash
GRID = 128.0                 # Part A: every input and every value is a multiple of 1 / GRID


# ---- launch geometry -------------------------------------------------------------------------------------------------
def ray_split(n_rays, n_cu, segs_per_tile, spr):
    """nfl_ray_split: (rays per workgroup, workgroups)."""
    rpw = (n_rays + n_cu - 1) // n_cu
    per_tile = segs_per_tile // spr
    if per_tile > 1:
        rpw = (rpw + per_tile - 1) // per_tile * per_tile
    rpw = max(rpw, 1)
    return rpw, (n_rays + rpw - 1) // rpw


def tiling(R, N, n_cu):
    spr = (N + 31) // 32
    rpw, grid = ray_split(R, n_cu, NSLOT, spr)
    segs = [(min(R, (g + 1) * rpw) - g * rpw) * spr for g in range(grid)]
    return dict(spr=spr, rpw=rpw, grid=grid, segs=segs, tiles=[(s + NSLOT - 1) // NSLOT for s in segs],
                last_live=N - 32 * (spr - 1))


def big_shape(n_cu):
    return 2 * n_cu + 1, 33


SMALL_SHAPES = [(1, 1), (3, 40), (2, 160), (3, 300)]


def situation_violations(R, N, n_cu):
    """What the shape is in the suite for; a list of complaints if this device's CU count makes something else of it."""
    t = tiling(R, N, n_cu)
    want = {(1, 1): dict(spr=1, rpw=4, segs=[1], tiles=[1], last_live=1),
            # two rays per workgroup; the second workgroup's only tile has 2 of 4 segments: waves 2 and 3 re-store the last
            (3, 40): dict(spr=2, rpw=2, segs=[4, 2], tiles=[1, 1], last_live=8),
            # one ray per workgroup, two tiles each, the second with one segment: ring and compositing carry cross a tile
            (2, 160): dict(spr=5, rpw=1, segs=[5, 5], tiles=[2, 2], last_live=32),
            (3, 300): dict(spr=10, rpw=1, segs=[10, 10, 10], tiles=[3, 3, 3], last_live=12)}.get((R, N))
    if want is None:       # four rays = two full tiles per workgroup, several rays per tile, one ray in the last workgroup
        if (R, N) != big_shape(n_cu):
            return [f"R={R} N={N} is not the 2 n_cu + 1 rays of 33 samples of a device with {n_cu} CUs"]
        want = dict(spr=2, rpw=4, grid=(R + 3) // 4, last_live=1)
        if t["segs"][:-1] != [8] * (t["grid"] - 1) or t["segs"][-1] != 2 or set(t["tiles"][:-1]) != {2}:
            return [f"R={R} N={N} on {n_cu} CUs: segments per workgroup {t['segs'][:3]} .. {t['segs'][-1]}"]
    return [f"R={R} N={N} on {n_cu} CUs: {k} is {t[k]}, the case needs {v}" for k, v in want.items() if t[k] != v]


def padded_rows(R, N):
    """Row of the (n_seg * 32)-row stash tensors that holds (ray, sample), in (ray, sample) order."""
    spr = (N + 31) // 32
    i = torch.arange(N)
    return ((torch.arange(R)[:, None] * spr + i[None, :] // 32) * 32 + i[None, :] % 32).flatten()


def locate(k, N, n_cu, R):
    """Where live sample k (in (ray, sample) order) runs."""
    ray, sample = divmod(int(k), N)
    t = tiling(R, N, n_cu)
    wg = ray // t["rpw"]
    g = (ray - wg * t["rpw"]) * t["spr"] + sample // 32
    return (f"ray {ray} sample {sample} (workgroup {wg}, tile {g // NSLOT} of its {t['tiles'][wg]}, wave {g % NSLOT}, "
            f"lane {sample % 32})")


def nkp_for(n_emb_xyz):
    """nfl_nkp_for: position-encoding k-steps of the kernel instantiation that runs the field."""
    return (6 * (10 if n_emb_xyz <= 10 else 15) + 3 + 15) // 16


def spec_of(widths, lat, beta_min=0.1):
    nx, nd, na, nt = widths
    if not lat:
        return orc.FieldSpec("coarse", n_emb_xyz=nx, n_emb_dir=nd)
    return orc.FieldSpec("fine", n_emb_xyz=nx, n_emb_dir=nd, encode_appearance=True, n_a=na, encode_transient=True, n_tau=nt,
                         beta_min=beta_min)


def layout_of(widths, lat, use_t):
    nx, nd, na, nt = widths
    return sc.Layout(nx, nd, na, nt, nkp=nkp_for(nx), has_a=lat, has_t=use_t)


# ---- Part A: a field and inputs on which everything is exact ---------------------------------------------------------
# name -> ((n_emb_xyz, n_emb_dir, n_a, n_tau), kind); kinds as in tests/test_dgrad_gpu.py
VARIANTS = {"base": ((10, 4, 48, 16), "coarse"),
            "nerfw": ((10, 4, 48, 16), "nerfw_t"),
            "nerfw_not": ((10, 4, 48, 16), "nerfw_not"),      # t_emb=None: the ring stops before the transient chunks
            "narrow": ((10, 4, 24, 8), "nerfw_t"),            # the scalar-load paths of the latent codes
            "wide": ((15, 4, 48, 16), "nerfw_t")}             # the wide instantiation (nfl_render_x3w.hip), NKP 6


def sparse_ternary(out_f, in_f, gen, fanin):
    """Entries in {-1, 0, 1}, `fanin` non-zeros in every column, then one more in every row that got none (the generator of
    tests/test_dgrad_gpu.py with the count as an argument)."""
    k = min(fanin, out_f)
    rows = torch.rand(out_f, in_f, generator=gen).argsort(0)[:k]
    w = torch.zeros(out_f, in_f)
    w[rows, torch.arange(in_f).expand(k, in_f)] = (2 * torch.randint(0, 2, (k, in_f), generator=gen) - 1).float()
    for i in (w.abs().sum(1) == 0).nonzero().flatten().tolist():
        w[i, int(torch.randint(0, in_f, (1,), generator=gen))] = 1.0
    return w


HEAD_LAYERS = ("static_sigma.0", "static_rgb.0", "transient_sigma.0", "transient_rgb.0", "transient_beta.0")


SEEDS = {(15, 4, 48, 16): 4}      # seed 3 puts a head of the wide field at 11: outside the +-8 the 8 ulp are derived for


def int_params(widths, lat, seed=None):
    """Ternary sparse weights and small-integer biases in every layer, xyz_encoding_final included, so that the fold
    W' = W[:, :256] W_fin, b' = b + W[:, :256] b_fin is an exact integer matrix.  One non-zero per input column in the wide
    layers (values then stay within a few times the inputs' through all thirteen layers), two in the columns that read the
    inputs; the heads have three non-zeros per row, which keeps their pre-activations within +-8."""
    seed = SEEDS.get(widths, 3) if seed is None else seed
    gen = torch.Generator().manual_seed(seed + 100 * list(VARIANTS.values()).index((widths, "nerfw_t" if lat else "coarse")))
    spec = spec_of(widths, lat)
    cx = spec.c_xyz
    P = {}
    for name, shape in orc.field_param_shapes(spec).items():
        layer = name.rsplit(".", 1)[0]
        if name.endswith("bias"):
            P[name] = torch.randint(-1, 2, shape, generator=gen).float()
        elif layer in HEAD_LAYERS:
            w = torch.zeros(shape)
            for r in range(shape[0]):
                cols = torch.randperm(shape[1], generator=gen)[:3]
                w[r, cols] = (2 * torch.randint(0, 2, (3,), generator=gen) - 1).float()
            P[name] = w
        else:
            w = sparse_ternary(*shape, gen, 1)
            # the columns that read an input directly: two non-zeros each, so that the inputs reach more of the layer
            side = {"xyz_encoding_1.0": (0, cx), "xyz_encoding_5.0": (0, cx), "dir_encoding.0": (W, shape[1]),
                    "transient_encoding.0": (W, shape[1])}.get(layer)
            if side:
                w[:, side[0]:side[1]] = sparse_ternary(shape[0], side[1] - side[0], gen, 2)
            P[name] = w
    return P


def int_inputs(R, N, widths, lat):
    """Rays, depths, view directions and codes on dyadic grids: o + d z is a multiple of 1/128 within +-1.5 (d has entries
    in {-1, 0, 1}: the product is exact, so is the sum, with or without fma), the view direction has entries in
    {-1/2, 0, 1/2, 1}, the codes are integers in -2 .. 2.  Every ray differs from its neighbours in origin, direction
    pattern, depth offset, view direction and codes."""
    nx, nd, na, nt = widths
    r = torch.arange(R)
    z = 2.0 + (torch.arange(N)[None, :] + (r % 3)[:, None]).double() / GRID
    pat = torch.tensor([(1, 0, -1), (-1, 1, 0), (0, -1, 1), (1, 1, 0), (0, 1, -1), (-1, 0, -1)], dtype=torch.float64)
    d = pat[r % 6]
    c = round((2.0 + N / 256.0) * GRID) / GRID
    off = torch.stack([(r % 5) - 2, (r // 5 % 5) - 2, (r // 25 % 5) - 2], 1).double() / 8.0
    o = off - d * c
    rays = torch.cat([o, d, torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)], 1)
    view = torch.stack([((r % 3) - 1) / 2.0, ((r // 3 % 3) - 1) / 2.0, torch.ones(R)], 1).double()
    gen = torch.Generator().manual_seed(1000 * R + N)
    a = torch.randint(-2, 3, (R, na), generator=gen).double() if lat else None
    t = torch.randint(-2, 3, (R, nt), generator=gen).double() if lat else None
    xyz = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(R * N, 3)
    return dict(rays=rays, z=z, view=view, a=a, t=t, xyz=xyz)


def int_reference(P, inp, widths, lat, use_t, N):
    """float64 forward of the module as the model defines it (xyz_encoding_final NOT folded): every stash field of every
    live sample in (ray, sample) order, and the (n, 9) head pre-activations in the order of field_raw
    [rgb, sigma, rgb_t, sigma_t, beta] (NaN where the pass has no such head)."""
    nx, nd, na, nt = widths
    cx, cd = 6 * nx + 3, 6 * nd + 3
    P = {k: v.double() for k, v in P.items()}
    lin = lambda name, x: x @ P[name + ".weight"].t() + P[name + ".bias"]
    n = inp["xyz"].shape[0]
    rep = lambda v: v.repeat_interleave(N, 0)
    pe = torch.cat([inp["xyz"], torch.zeros(n, cx - 3, dtype=torch.float64)], 1)         # BARF weights 0: only the raw columns
    out, h = {"pe": pe}, pe
    for l in range(1, 9):
        h = torch.relu(lin(f"xyz_encoding_{l}.0", torch.cat([pe, h], 1) if l == 5 else h))
        out[f"h{l}"] = h
    pre = torch.full((n, 9), float("nan"), dtype=torch.float64)
    pre[:, 3] = lin("static_sigma.0", h)[:, 0]
    feat = lin("xyz_encoding_final", h)
    side = torch.cat([rep(inp["view"]), torch.zeros(n, cd - 3, dtype=torch.float64)] + ([rep(inp["a"])] if lat else []), 1)
    out["dir_side"] = side
    out["dirh"] = torch.relu(lin("dir_encoding.0", torch.cat([feat, side], 1)))
    pre[:, 0:3] = lin("static_rgb.0", out["dirh"])
    if use_t:
        out["tau"] = rep(inp["t"])
        g = torch.cat([feat, out["tau"]], 1)
        for m, j in enumerate((0, 2, 4, 6)):
            g = torch.relu(lin(f"transient_encoding.{j}", g))
            out[f"g{m + 1}"] = g
        pre[:, 4:7] = lin("transient_rgb.0", g)
        pre[:, 7] = lin("transient_sigma.0", g)[:, 0]
        pre[:, 8] = lin("transient_beta.0", g)[:, 0]
    return out, pre


def exactness_violations(P, inp, ref, pre, widths, lat, use_t, N):
    """The conditions under which 'equal in every arithmetic' holds and the case proves something (a list of complaints):
    the inputs are what int_inputs promises and o + d z is exact in fp32; every stashed value is one fp16; every value is a
    multiple of 1/128 and every layer's sum of |terms| -- with the folded matrices -- stays below 2^24 / 128, so every
    partial sum is exact in fp32 in any order; both mask values occur in every 32-feature tile of every masked layer; no
    field is zero everywhere; the head pre-activations are within +-8."""
    bad = []
    rays, z = inp["rays"], inp["z"]
    got = rays.float()[:, None, 0:3] + rays.float()[:, None, 3:6] * z.float()[..., None]          # fp32, products rounded
    if not torch.equal(got.double().reshape(-1, 3), inp["xyz"]) or not torch.equal(rays.float().double(), rays) \
            or not torch.equal(z.float().double(), z) \
            or not torch.equal((rays.float()[:, None, 3:6] * z.float()[..., None]).double(), rays[:, None, 3:6] * z[..., None]):
        bad.append("o + d z is not exact in fp32")
    for name, v in ref.items():
        if not torch.equal(v.half().double(), v):
            bad.append(f"{name}: not representable in one fp16 (max {float(v.abs().max())})")
        if not torch.equal(v * GRID, (v * GRID).round()):
            bad.append(f"{name}: not on the 1/128 grid")
        if not bool(v.any()):
            bad.append(f"{name}: zero everywhere")
    for name in sc.mask_fields(use_t):
        on = (ref[name] > 0).view(ref[name].shape[0], -1, 32)
        both = on.any(0).any(1) & (~on).any(0).any(1)
        if not bool(both.all()):
            bad.append(f"{name}: tiles {(~both).nonzero().flatten().tolist()} hold one mask value only")
    A = {k: v.double().abs() for k, v in P.items()}
    for out_name, _, ins, wname in layer_table(widths, lat, use_t):
        x = torch.cat([ref[i].abs() for i in ins], 1)
        w = A[wname + ".weight"]
        b = A[wname + ".bias"]
        if wname in ("dir_encoding.0", "transient_encoding.0"):       # |W'| <= |W[:, :256]| |W_fin|, |b'| likewise
            w = torch.cat([w[:, :W] @ A["xyz_encoding_final.weight"], w[:, W:]], 1)
            b = b + A[wname + ".weight"][:, :W] @ A["xyz_encoding_final.bias"]
        if float((x @ w.t() + b).max()) * GRID >= 2.0 ** 24:
            bad.append(f"{out_name}: the sum of |terms| reaches 2^24 steps")
    live = pre[:, ~torch.isnan(pre[0])]
    if float(live.abs().max()) > 8.0:
        bad.append(f"head pre-activations reach {float(live.abs().max())}")
    return bad


def fp16_weight_violations(P, fold=None):
    """One more condition, for the single-product kernels (nfl_render_x1.hip): they read the hi image of every weight and
    nothing else, so 'equal in every arithmetic' needs every weight to BE one fp16 -- the two folded matrices included:
    `fold` = name -> (weight, bias) as read back from the field, or None for the fp32 fold of `P`.  The biases go to the
    kernel as fp32.  A list of complaints."""
    F = dict(fold_fp32(P))
    for name, (w, b) in (fold or {}).items():
        F[name + ".weight"] = w.detach().float().cpu()
    bad = []
    for name, w in F.items():
        if name.endswith(".weight") and name != "xyz_encoding_final.weight":
            w = w.detach().float().cpu()
            off = w.half().float() != w
            if bool(off.any()):
                r, c = off.nonzero()[0].tolist()
                bad.append(f"{name}: {int(off.sum())} weights are not one fp16, first [{r}, {c}] = {w[r, c].item()!r}")
    return bad


def int_embedded(inp, widths, lat, use_t, N):
    """The encoded (R N, C) matrix NeRF.forward takes, of a Part A case: with BARF weights 0 only the raw coordinates of both
    encodings are non-zero, so a row is [xyz, 0 ..., view, 0 ..., a, t] (a with an appearance field, t with the transient
    head on), in (ray, sample) order.  float64."""
    nx, nd, na, nt = widths
    n = inp["xyz"].shape[0]
    rep = lambda v: v.double().repeat_interleave(N, 0)
    zeros = lambda c: torch.zeros(n, c, dtype=torch.float64)
    cols = [inp["xyz"].double(), zeros(6 * nx), rep(inp["view"]), zeros(6 * nd)]
    if lat:
        cols.append(rep(inp["a"]))
    if use_t:
        cols.append(rep(inp["t"]))
    return torch.cat(cols, 1)


def head_activation(pre):
    """float64 field_raw of (n, 9) head pre-activations: softplus on sigma, sigma_t and beta, sigmoid on the colours."""
    out = torch.sigmoid(pre)
    for k in (3, 7, 8):
        out[:, k] = torch.clamp(pre[:, k], min=0) + torch.log1p(torch.exp(-pre[:, k].abs()))
    return out


def ulp32(v):
    """Spacing of fp32 at |v| (float64 in, float64 out)."""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126))) - 23)


# ---- the runner --------------------------------------------------------------------------------------------------------
def run_forward(f, rays, z, N, *, split, a_emb=None, t_emb=None, view_dir=None, pe_w=None, noise=None, noise_std=0.0,
                white_back=True):
    """One nfl_render_pass in training mode, its PassArgs built here as rendering._run_pass builds them, with the activation
    stash inside an arena of SENT16 and GUARD bytes of it on either side.  Returns the pass's outputs (device tensors) with
    `stash` (the nfl_act_stash_bytes() bytes, a view of the arena) and `guards_ok`."""
    from nerf_fl_amd import _lib, rendering as rnd
    L = _lib.lib()
    R, dev = rays.shape[0], rays.device
    bprec = _lib.NFL_PREC_F16X3 if split else _lib.NFL_PREC_F16
    rnd._pack_streams([f])
    nb = L.nfl_act_stash_bytes(C.byref(f.desc), R, N, bprec)
    assert nb > 0 and nb % 2 == 0
    arena = torch.full(((2 * GUARD + nb) // 2,), SENT16, dtype=torch.int16, device=dev).view(torch.uint8)
    use_t = t_emb is not None
    new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    out = dict(weights=new(R, N), opacity=new(R), rgb=new(R, 3), depth=new(R), field_raw=new(R * N, 9))
    if use_t:
        out.update(transient_sigmas=new(R, N), beta=new(R), rgb_static=new(R, 3), rgb_transient=new(R, 3))
    stash = arena[GUARD:GUARD + nb]
    a = _pass_args(out, rays, z, N, a_emb, t_emb, view_dir, pe_w, noise, noise_std, white_back)
    a.d_act_stash = rnd._ptr(stash)
    a.stash_split = int(bool(split))
    _launch_pass(f, a)
    g = arena.view(torch.int16)
    out["guards_ok"] = bool((g[:GUARD // 2] == SENT16).all()) and bool((g[(GUARD + nb) // 2:] == SENT16).all())
    out["stash"] = stash
    return out


def _pass_args(out, rays, z, N, a_emb, t_emb, view_dir, pe_w, noise, noise_std, white_back):
    """PassArgs of one pass over given rays and depths, as rendering._run_pass builds them; d_act_stash is left null."""
    from nerf_fl_amd import _lib, rendering as rnd
    p = rnd._ptr
    a = _lib.PassArgs()
    a.d_rays, a.d_view_dir = p(rays), p(view_dir)
    a.n_rays, a.n_samples = rays.shape[0], N
    a.d_z = p(z)
    a.d_noise, a.noise_std = p(noise), float(noise_std)
    a.d_a_emb, a.d_t_emb = p(a_emb), p(t_emb)
    a.white_back = int(bool(white_back))
    a.d_weights, a.d_opacity, a.d_rgb, a.d_depth = p(out["weights"]), p(out["opacity"]), p(out["rgb"]), p(out["depth"])
    a.d_transient_sigmas, a.d_beta = p(out.get("transient_sigmas")), p(out.get("beta"))
    a.d_rgb_static, a.d_rgb_transient = p(out.get("rgb_static")), p(out.get("rgb_transient"))
    a.d_field_raw = p(out["field_raw"])
    if pe_w is not None:
        a.d_pe_w_xyz, a.d_pe_w_dir = p(pe_w[0]), p(pe_w[1])
    a.d_status = p(rnd._status_word(rays.device))
    return a


def _launch_pass(f, a):
    from nerf_fl_amd import _lib, rendering as rnd
    p = rnd._ptr
    _lib.check(_lib.lib().nfl_render_pass(f.h_plan, p(f.d_plan), p(f.packed), C.byref(a), rnd._stream()), "nfl_render_pass")
    torch.cuda.synchronize()


SENTF = 0x7FC5A7E5            # an fp32 NaN with a payload: what the arenas of the inference runners are filled with


class Arena:
    """An fp32 output buffer of `shape` inside an allocation filled with SENTF, GUARD bytes of it on either side."""

    def __init__(self, shape, dev):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.all = torch.full((2 * (GUARD // 4) + n,), SENTF, dtype=torch.int32, device=dev)
        self.t = self.all[GUARD // 4:GUARD // 4 + n].view(torch.float32).view(*shape)

    def guards_ok(self):
        return bool((self.all[:GUARD // 4] == SENTF).all()) and bool((self.all[GUARD // 4 + self.n:] == SENTF).all())


def _finish(out, arenas):
    out["guards"] = {k: v.guards_ok() for k, v in arenas.items()}
    out["guards_ok"] = all(out["guards"].values())
    out["nan_left"] = [k for k, v in arenas.items() if bool(torch.isnan(v.t).any())]
    return out


def run_render(f, rays, z, N, *, a_emb=None, t_emb=None, view_dir=None, pe_w=None, noise=None, noise_std=0.0, white_back=True):
    """One nfl_render_pass at inference: the PassArgs of run_forward with d_act_stash null, so nfl_render_mode picks
    NFL_MODE_RENDER -- of the three-product or the single-product kernel, as `f` was planned.  Every output buffer lies in
    an Arena of its own.  Returns the outputs (device tensors) with `guards` (name -> intact), `guards_ok` and `nan_left`
    (the buffers that still hold a NaN)."""
    from nerf_fl_amd import rendering as rnd
    R, dev = rays.shape[0], rays.device
    rnd._pack_streams([f])
    shapes = dict(weights=(R, N), opacity=(R,), rgb=(R, 3), depth=(R,), field_raw=(R * N, 9))
    if t_emb is not None:
        shapes.update(transient_sigmas=(R, N), beta=(R,), rgb_static=(R, 3), rgb_transient=(R, 3))
    arenas = {k: Arena(s, dev) for k, s in shapes.items()}
    out = {k: v.t for k, v in arenas.items()}
    _launch_pass(f, _pass_args(out, rays, z, N, a_emb, t_emb, view_dir, pe_w, noise, noise_std, white_back))
    return _finish(out, arenas)


def run_embed(f, x, stride=None, sigma_only=False, output_transient=True):
    """nfl_field_forward (NFL_MODE_EMBED) on the encoded (B, C) matrix `x`, laid out with a row stride of `stride` floats
    (default C + 3: rows are then not 16-byte aligned) whose extra columns hold NaN; the (B, 9) output lies in an Arena.
    Returns dict(raw, guards, guards_ok, nan_left)."""
    from nerf_fl_amd import _lib, rendering as rnd
    B, width = x.shape
    stride = width + 3 if stride is None else stride
    assert stride >= width and B > 0
    dev = f.packed.device
    rnd._pack_streams([f])
    rows = torch.full((B, stride), float("nan"), dtype=torch.float32, device=dev)
    rows[:, :width] = x.to(device=dev, dtype=torch.float32)
    arenas = {"raw": Arena((B, 9), dev)}
    p = rnd._ptr
    _lib.check(_lib.lib().nfl_field_forward(f.h_plan, p(f.d_plan), p(f.packed), p(rows), B, stride, int(bool(sigma_only)),
                                            int(bool(output_transient)), p(arenas["raw"].t), rnd._stream()), "nfl_field_forward")
    torch.cuda.synchronize()
    return _finish({"raw": arenas["raw"].t}, arenas)


def bit_differences(a, b, names):
    """The buffers `names` of two passes' outputs that are not bit-identical (name -> where the first difference is)."""
    out = {}
    for k in names:
        x, y = a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)
        if x.shape != y.shape:
            out[k] = f"shapes {tuple(x.shape)} and {tuple(y.shape)}"
        elif not torch.equal(x, y):
            at = (x != y).nonzero()[0].tolist()
            out[k] = (f"{int((x != y).sum())} of {x.numel()} values differ, first at {at}: {a[k][tuple(at)].item()!r} against "
                      f"{b[k][tuple(at)].item()!r}")
    return out


def embed_columns(sigma_only, output_transient):
    """The columns of field_raw NeRF.forward returns (rendering.field_forward)."""
    return [3] if sigma_only else list(range(9 if output_transient else 4))


def decode(stash, lay, n_seg, mult, use_t):
    """Stash bytes (CPU or device) -> dict(hi, lo, masks, words): the named fields of the hi (and lo) records, the relu
    masks, and the mask words as an (n_seg, 84, 64 lanes) int32 tensor."""
    rec = sc.Layout._records(stash, n_seg, lay.act_slots, mult)
    off = sc.mask_offset(n_seg, lay.nkp, mult)
    mbytes = stash[off:off + n_seg * sc.MSK_WORDS * 256]
    words = sc._mask_words(mbytes, n_seg).permute(0, 1, 3, 2).reshape(n_seg, sc.MSK_WORDS, 64)
    return dict(hi=sc.Layout._get(rec[:, 0], lay.act), lo=sc.Layout._get(rec[:, 1], lay.act) if mult == 2 else None,
                masks=sc.decode_masks(mbytes, n_seg, use_t), words=words, rec=rec)


def _bits16(v):
    return v.contiguous().view(torch.int16)


def unwritten(dec, use_t, N):
    """Every position a field names, in every segment (padded lanes included), written and finite; every mask word of a
    layer the pass evaluates written, the words of the others untouched.  A list of complaints."""
    bad = []
    spr = (N + 31) // 32
    for which in ("hi", "lo"):
        if dec[which] is None:
            continue
        for name, v in dec[which].items():
            for what, m in (("never written", _bits16(v) == SENT16), ("not finite", ~torch.isfinite(v))):
                if bool(m.any()):
                    row, col = m.nonzero()[0].tolist()
                    seg, lane = divmod(row, 32)
                    live = (seg % spr) * 32 + lane < N
                    bad.append(f"{name} ({which}): {int(m.sum())} positions {what}; first in segment {seg} (ray {seg // spr}) lane "
                               f"{lane} ({'live' if live else 'padded'}) feature {col}")
                    break
    n_words = 84 if use_t else sc.mask_fields(False)["dirh"][0] + 4
    w = dec["words"]
    if bool((w[:, :n_words] == SENT32).any()):
        seg, word, lane = (w[:, :n_words] == SENT32).nonzero()[0].tolist()
        bad.append(f"mask word {word} of segment {seg} (lane {lane}) never written")
    if bool((w[:, n_words:] != SENT32).any()):
        bad.append("mask words of the transient layers written by a pass without the transient head")
    return bad


def mismatches(dec, ref, R, N, n_cu, use_t):
    """Part A: every live sample's hi record EQUAL to the reference (-0 == 0), its lo record zero, its mask bits value > 0.
    name -> where the first difference is.  Works on the device `dec` lives on."""
    dev = next(iter(dec["hi"].values())).device
    rows = padded_rows(R, N).to(dev)
    out = {}

    def note(what, m, got, exp):
        if bool(m.any()):
            k, col = m.nonzero()[0].tolist()
            rays = sorted(set((m.nonzero()[:, 0] // N).tolist()))[:8]
            out[what] = (f"{int(m.sum())} of {m.numel()} differ; first at {locate(k, N, n_cu, R)} feature {col} (tile {col // 32}): got "
                         f"{got[k, col].item()} expected {exp[k, col].item()}; rays {rays} tiles {sorted(set((m.nonzero()[:, 1] // 32).tolist()))}")

    for name, e in ref.items():
        e = e.to(dev)
        g = dec["hi"][name][rows].double()
        note(name, g != e, g, e)
        if dec["lo"] is not None:
            l = dec["lo"][name][rows].double()
            note(name + " (lo record)", l != 0, l, torch.zeros_like(l))
        if name in dec["masks"]:
            mk = dec["masks"][name][rows]
            note(name + " (mask)", mk != (e > 0), mk.double(), (e > 0).double())
    return out


def same_bits(a, b):
    """STASH against STASH2 of the same case: hi records, mask words (name -> complaint)."""
    out = {}
    for name, v in a["hi"].items():
        if not torch.equal(_bits16(v), _bits16(b["hi"][name])):
            row, col = (_bits16(v) != _bits16(b["hi"][name])).nonzero()[0].tolist()
            out[name] = f"hi record differs between the two modes, first in segment {row // 32} lane {row % 32} feature {col}"
    if not torch.equal(a["words"], b["words"]):
        out["masks"] = f"mask words differ, first (segment, word, lane) {(a['words'] != b['words']).nonzero()[0].tolist()}"
    return out


# ---- Part B: layer by layer from the decoded operands -----------------------------------------------------------------
PRODS_INDEX = dict([(f"h{l}", l - 1) for l in range(1, 9)] + [("sigma", 8), ("dirh", 9), ("rgb", 10)]
                   + [(f"g{m}", 10 + m) for m in range(1, 5)] + [("sigma_t", 15), ("rgb_t", 15), ("beta", 15)])
HEAD_COLS = {"sigma": [3], "rgb": [0, 1, 2], "sigma_t": [7], "rgb_t": [4, 5, 6], "beta": [8]}


def read_prods():
    """The per-layer product plan the library is built with (csrc/nfl_prods.h, the table that is not the sweep override)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nerf_fl_amd", "csrc", "nfl_prods.h")
    text = open(path).read().split("#else", 1)[1]
    vals = re.search(r"NFL_PRODS\[NFL_P_IDX_COUNT\]\s*=\s*\{([^}]*)\}", text).group(1)
    prods = [int(v) for v in vals.split(",")]
    assert len(prods) == 16 and all(0 <= p <= 3 for p in prods), prods
    return prods


def layer_table(widths, lat, use_t):
    """(output, is a head, [input fields in the order of the weight's columns], layer name).  dir_encoding.0 and
    transient_encoding.0 read h8 through the fold."""
    t = []
    for l in range(1, 9):
        t.append((f"h{l}", False, ["pe"] if l == 1 else ["pe", "h4"] if l == 5 else [f"h{l - 1}"], f"xyz_encoding_{l}.0"))
    t.append(("sigma", True, ["h8"], "static_sigma.0"))
    t.append(("dirh", False, ["h8", "dir_side"], "dir_encoding.0"))
    t.append(("rgb", True, ["dirh"], "static_rgb.0"))
    if use_t:
        t.append(("g1", False, ["h8", "tau"], "transient_encoding.0"))
        for m, j in ((2, 2), (3, 4), (4, 6)):
            t.append((f"g{m}", False, [f"g{m - 1}"], f"transient_encoding.{j}"))
        t += [("sigma_t", True, ["g4"], "transient_sigma.0"), ("rgb_t", True, ["g4"], "transient_rgb.0"),
              ("beta", True, ["g4"], "transient_beta.0")]
    return t


def split16(w):
    """fp32 -> (hi, lo) fp16 images, round to nearest even, as nfl_pack.hip splits a forward stream (float64 out)."""
    hi = w.float().half()
    return hi.double(), (w.float() - hi.float()).half().double()


def predict(xh, xl, w, b, prods=3):
    """float64 value of the products the kernel issues, b + w_hi x_hi (+ w_lo x_hi) (+ w_hi x_lo), the same without either
    correction, and the sum of the absolute values of all terms."""
    wh, wl = split16(w)
    b = b.double()
    base = b + xh @ wh.t()
    c_w = xh @ wl.t() if prods & 1 else torch.zeros_like(base)
    c_x = xl @ wh.t() if prods & 2 else torch.zeros_like(base)
    mag = b.abs() + xh.abs() @ wh.abs().t() + (xh.abs() @ wl.abs().t() if prods & 1 else 0.0) + (xl.abs() @ wh.abs().t() if prods & 2 else 0.0)
    return base + c_w + c_x, {"w_lo x_hi": base + c_x, "w_hi x_lo": base + c_w}, mag


def rms(v):
    return float(v.double().pow(2).mean().sqrt()) if v.numel() else 0.0


def check_layers(dec, field_raw, P, widths, lat, use_t, R, N, n_cu, prods=None):
    """Part B on one decoded split stash.  `P`: the fp32 parameters the packer read, dir_encoding.0 / transient_encoding.0
    being the FOLDED ones.  Returns (complaints, report): report[layer] = (largest error / hard bound,
    rms(h^ - full) / rms(full - mutant) for the mutant without w_lo x_hi, the same without w_hi x_lo)."""
    prods = read_prods() if prods is None else prods
    rows = padded_rows(R, N)
    hi = {k: v[rows].double() for k, v in dec["hi"].items()}
    lo = {k: v[rows].double() for k, v in dec["lo"].items()}
    bad, report = [], {}
    fr = None if field_raw is None else field_raw.double()

    def where(m):
        k, col = m.nonzero()[0].tolist()
        return f"{locate(k, N, n_cu, R)} feature {col} (tile {col // 32})"

    for name, head, ins, layer in layer_table(widths, lat, use_t):
        xh, xl = torch.cat([hi[i] for i in ins], 1), torch.cat([lo[i] for i in ins], 1)
        w, b = P[layer + ".weight"], P[layer + ".bias"]
        K = w.shape[1]
        assert xh.shape[1] == K, (name, xh.shape, w.shape)
        pp = prods[PRODS_INDEX[name]]
        full, mutants, mag = predict(xh, xl, w, b, pp)
        acc_bound = (3 * K + 1) * U24 * mag
        if head:
            if fr is None:
                continue
            cols = HEAD_COLS[name]
            soft = name in ("sigma", "sigma_t", "beta")
            pre9 = torch.zeros(full.shape[0], 9, dtype=torch.float64)
            pre9[:, cols] = full
            exp = head_activation(pre9)[:, cols]
            bound = (1.0 if soft else 0.25) * acc_bound + 8 * ulp32(exp)
            ratio = (fr[:, cols] - exp).abs() / bound
            report[name] = (float(ratio.max()), None, None)
            if not float(ratio.max()) <= 1.0:
                bad.append(f"{name}: field_raw is {float(ratio.max()):.3f} of its bound from the layer-local float64 head at {where(ratio == ratio.max())}")
            continue
        hh, hl = hi[name], lo[name]
        hhat = hh + hl
        target = torch.relu(full)
        bound = acc_bound + 2.0 ** -22 * target + U24
        ratio = (hhat - target).abs() / bound
        if not float(ratio.max()) <= 1.0:
            bad.append(f"{name}: |h^ - relu(pre)| reaches {float(ratio.max()):.3f} of the hard bound at {where(ratio == ratio.max())}")
        mk = dec["masks"][name][rows]
        if not torch.equal(mk, hh != 0):
            bad.append(f"{name}: {int((mk != (hh != 0)).sum())} mask bits are not (hi != 0), first at {where(mk != (hh != 0))}")
        # a nearest one: when x - hi rounds up to exactly half a step of hi, hi + lo is a tie and round-to-even may name
        # the other neighbour, which is then exactly as far
        resplit = hhat.float().half().double()
        farther = (resplit != hh) & ((hhat - resplit).abs() != (hhat - hh).abs())
        if bool(farther.any()):
            bad.append(f"{name}: hi is not an fp16 nearest to hi + lo, first at {where(farther)}")
        err = rms((hhat - target)[mk])
        rep = [float(ratio.max())]
        for bit, (what, mut) in zip((1, 2), mutants.items()):
            if not pp & bit:
                rep.append(None)
                continue
            gap = rms((target - torch.relu(mut))[mk])
            rep.append(err / gap if gap > 0 else float("inf"))
            if not gap > 0:
                bad.append(f"{name}: the product {what} changes nothing here: the case cannot see its loss")
            elif not err <= gap / 8:
                bad.append(f"{name}: rms(h^ - full) = {err:.3e} is {err / gap:.3f} of rms(full - [without {what}]) = {gap:.3e}; allowed 1/8")
        report[name] = tuple(rep)
    return bad, report


def check_sides(dec, inp, widths, lat, use_t, R, N, pe_w):
    """Part B: the side records.  Codes bit-exact (hi = code.half(), lo = (code - hi).half(), zero beyond a narrower code's
    width); encodings within 1e-6 + 2^-22 |v| of the float64 encoding of the exact point (raw columns exact)."""
    nx, nd, na, nt = widths
    cx, cd = 6 * nx + 3, 6 * nd + 3
    rows = padded_rows(R, N)
    bad = []
    val = lambda name: dec["hi"][name][rows].double() + dec["lo"][name][rows].double()
    xyz = inp["rays"][:, None, 0:3].double() + inp["rays"][:, None, 3:6].double() * inp["z"][..., None].double()
    for name, x, nf, w in (("pe", xyz.reshape(-1, 3), nx, None if pe_w is None else pe_w[0]),
                           ("dir_side", inp["rays"][:, 3:6].double().repeat_interleave(N, 0), nd, None if pe_w is None else pe_w[1])):
        exp = orc.posenc(x, nf, None if w is None else w.double())
        got = val(name)[:, :exp.shape[1]]
        ratio = (got - exp).abs() / (1e-6 + 2.0 ** -22 * exp.abs())
        if not float(ratio.max()) <= 1.0:
            bad.append(f"{name}: encoding off by {float(ratio.max()):.3f} of its tolerance")
        if not torch.equal(got[:, :3], x):
            bad.append(f"{name}: raw columns are not the exact point")
    for name, code, c0 in (("dir_side", inp["a"], cd), ("tau", inp["t"], 0)) if lat else ():
        if code is None or name not in dec["hi"]:
            continue
        c = code.float().repeat_interleave(N, 0)
        h = c.half()
        l = (c - h.float()).half()
        gh, gl = dec["hi"][name][rows][:, c0:c0 + c.shape[1]], dec["lo"][name][rows][:, c0:c0 + c.shape[1]]
        if not (torch.equal(_bits16(gh), _bits16(h)) and torch.equal(_bits16(gl), _bits16(l))):
            bad.append(f"{name}: the stashed code is not (code.half(), (code - hi).half())")
    return bad


def beyond_width(dec_rec, lay, widths):
    """Positions of the appearance / transient k-steps beyond a narrower code's width: zero in every record."""
    full = sc.Layout(widths[0], widths[1], 48, 16, nkp=lay.nkp, has_a=True, has_t="tau" in lay.act)
    bad = []
    for part in range(dec_rec.shape[1]):
        got = sc.Layout._get(dec_rec[:, part], {k: full.act[k] for k in ("dir_side", "tau") if k in full.act})
        for name, n_used, c0 in (("dir_side", lay.n_a, lay.cd), ("tau", lay.n_tau, 0)):
            if name in got and bool(_bits16(got[name][:, c0 + n_used:]).any()):
                bad.append(f"{name} (record {part}): not zero beyond the code's {n_used} columns")
    return bad


def emulate_forward(P, inp, widths, lat, use_t, R, N, pe_w=None, drop=None):
    """The kernel's arithmetic in fp32 torch on the CPU: operands split hi + lo, three products per layer, relu, split
    again; padded lanes repeat the ray's last sample.  `P`: fp32 parameters, the two folded layers folded.
    `drop` = (layer output, "w_lo x_hi" | "w_hi x_lo"): that layer loses the product.  Returns (stash bytes in a sentinel
    arena as the runner leaves them, field_raw fp32)."""
    nx, nd, na, nt = widths
    lay = layout_of(widths, lat, use_t)
    xyz = (inp["rays"][:, None, 0:3] + inp["rays"][:, None, 3:6] * inp["z"][..., None]).reshape(-1, 3).float()
    rep = lambda v: v.float().repeat_interleave(N, 0)
    val = {"pe": orc.posenc(xyz, nx, pe_w and pe_w[0]).float()}
    side = [orc.posenc(inp["rays"][:, 3:6].float(), nd, pe_w and pe_w[1]).float()] + ([inp["a"].float()] if lat else [])
    val["dir_side"] = rep(torch.cat(side, 1))
    if use_t:
        val["tau"] = rep(inp["t"])
    sp = lambda v: (v.half(), (v - v.half().float()).half())
    raw = torch.zeros(R * N, 9)
    for name, head, ins, layer in layer_table(widths, lat, use_t):
        parts = [sp(val[i]) for i in ins]
        xh, xl = torch.cat([p[0] for p in parts], 1).float(), torch.cat([p[1] for p in parts], 1).float()
        wh, wl = sp(P[layer + ".weight"].float())
        acc = P[layer + ".bias"].float() + xh @ wh.float().t()
        if drop != (name, "w_lo x_hi"):
            acc = acc + xh @ wl.float().t()
        if drop != (name, "w_hi x_lo"):
            acc = acc + xl @ wh.float().t()
        if head:
            raw[:, HEAD_COLS[name]] = acc
        else:
            val[name] = torch.relu(acc)
    act = head_activation(raw.double()).float()
    if not use_t:
        act[:, 4:] = 0
    # the stash: rows of padded lanes hold the ray's last sample
    spr = (N + 31) // 32
    n_seg = R * spr
    i = torch.arange(spr * 32).clamp(max=N - 1)
    src = (torch.arange(R)[:, None] * N + i[None, :]).flatten()
    hi = {k: sp(v)[0][src] for k, v in val.items()}
    lo = {k: sp(v)[1][src] for k, v in val.items()}
    off = sc.mask_offset(n_seg, lay.nkp, 2)
    nb = off + n_seg * sc.MSK_WORDS * 256
    stash = torch.full((nb // 2,), SENT16, dtype=torch.int16).view(torch.uint8)
    rec = sc.Layout._records(stash, n_seg, lay.act_slots, 2)
    sc.Layout._put(rec[:, 0], lay.act, hi)
    sc.Layout._put(rec[:, 1], lay.act, lo)
    n_words = 84 if use_t else 68
    mw = sc.encode_masks({k: hi[k] != 0 for k in sc.mask_fields(use_t)}, use_t)
    stash[off:off + n_seg * sc.MSK_WORDS * 256].view(n_seg, sc.MSK_WORDS // 4, 1024)[:, :n_words // 4] = \
        mw.view(n_seg, sc.MSK_WORDS // 4, 1024)[:, :n_words // 4]
    return stash, act


# ---- Part C: compositing of the pass's own field outputs ------------------------------------------------------------
def composite_ref(field_raw, z, *, noise, noise_std, use_t, white_back, beta_min):
    """name -> (float64 value, bound) of the pass's composited outputs from the field_raw the same pass wrote.
    tests/test_compbwd_gpu.py grants alpha 3 u and each factor 1 - alpha 5 u absolute (u = 2^-24), so a weight of sample i --
    alpha_i times a product of i such factors, all at most 1 -- gets (5 i + 3) u; a per-ray sum of N terms gets
    N u sum|terms| for its additions on top of its terms' own errors; every further addition (the white background, beta_min,
    static + transient) rounds once: u of its result."""
    p = cr._pieces(field_raw, z, noise, noise_std, use_t, white_back, [None] * 8, None, 0.0)
    R, N = p["R"], p["N"]
    z = z.double().cpu()
    T = p["T"]
    wb = ((5 * torch.arange(N) + 3) * U24).double()[None, :].expand(R, N)
    w = (1 - p["e"]) * T
    out = {"weights": (w, wb)}

    def ray_sum(wgt, v):
        v = v if v.dim() == 3 else v[..., None]
        t = wgt[..., None] * v
        return t.sum(1).squeeze(-1), ((wb[..., None] * v.abs()).sum(1) + N * U24 * t.abs().sum(1)).squeeze(-1)

    out["opacity"] = ray_sum(w, torch.ones(R, N, dtype=torch.float64))
    out["depth"] = ray_sum(w, z)
    wsum, wsum_b = out["opacity"]
    white = (1 - wsum, wsum_b + U24 * (1 - wsum).abs()) if white_back else (torch.zeros(R, dtype=torch.float64),) * 2

    def plus(a, b):        # value and bound of a rounded sum of two (value, bound) pairs
        v = a[0] + b[0]
        return v, a[1] + b[1] + U24 * v.abs()

    if use_t:
        ws, wt = (1 - torch.exp(-p["delta"] * p["sig"])) * T, (1 - torch.exp(-p["delta"] * p["sig_t"])) * T
        out["rgb_static"] = plus(ray_sum(ws, p["rgb"]), (white[0][:, None], white[1][:, None]))
        out["rgb_transient"] = ray_sum(wt, p["rgb_t"])
        out["rgb"] = plus(out["rgb_static"], out["rgb_transient"])
        bsum = ray_sum(wt, p["beta"])
        out["beta"] = plus(bsum, (torch.full((R,), beta_min, dtype=torch.float64), torch.zeros(R, dtype=torch.float64)))
    else:
        out["rgb"] = plus(ray_sum(w, p["rgb"]), (white[0][:, None], white[1][:, None]))
    return out


def composite_violations(out, ref):
    """A pass's composited outputs against composite_ref of its own field_raw: (complaints, name -> largest error / bound)."""
    bad, report = [], {}
    for name, (v, b) in ref.items():
        got = out[name].cpu().double().view_as(v)
        ratio = (got - v).abs() / b
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        report[name] = float(ratio.max())
        if not float(v.abs().max()) > 0:
            bad.append(f"{name}: the reference is zero everywhere")
        if not float(ratio.max()) <= 1.0:
            k = (ratio == ratio.max()).nonzero()[0].tolist()
            bad.append(f"{name}: {float(ratio.max()):.3f} of its bound at {k} (ray first; a weight's second index is its sample): "
                       f"got {got[tuple(k)].item()!r} float64 {v[tuple(k)].item()!r}")
    return bad, report


def sorted_depths(R, N, seed):
    """Sorted distinct depths on a 1/64 grid in [2, 10) (tests/test_wgrad_gpu.py::exact_rays has only 256 of them)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([torch.sort(128 + torch.randperm(512, generator=gen)[:N])[0] for _ in range(R)]).float() / 64.0


# ---- the cases ---------------------------------------------------------------------------------------------------------
# Part A: (variant, R, N); the fifth shape (2 n_cu + 1, 33) is added by the GPU test from the device's CU count
A_CASES = [(v, R, N) for v in ("base", "nerfw") for R, N in SMALL_SHAPES]
A_CASES += [(v, R, N) for v in ("nerfw_not", "narrow", "wide") for R, N in ((3, 40), (2, 160))]
B_SHAPES = [(3, 40), (2, 160)]
BARF = (torch.linspace(1.0, 0.25, 10), torch.linspace(0.9, 0.3, 4))      # BARF weights != 1, as tests/test_dgrad_gpu.py draws them


def real_inputs(R, N, lat):
    """Part B: the oracle's `sharp` weights as tests/test_dgrad_gpu.py::real_case uses them, exact_rays, random fp32 codes."""
    from test_wgrad_gpu import exact_rays
    widths = (10, 4, 48, 16)
    spec = spec_of(widths, lat)
    P = orc.make_field_params(spec, 81 + lat, "sharp")
    rays, z = exact_rays(R, N, 5 * R + N)
    gen = torch.Generator().manual_seed(R + N)
    a = torch.randn(R, 48, generator=gen) if lat else None
    t = torch.randn(R, 16, generator=gen) if lat else None
    return widths, spec, P, dict(rays=rays, z=z, a=a, t=t)


def fold_fp32(P):
    """The fold of nfl_compose_forward in fp32 torch (the CPU emulation's stand-in; the GPU test reads the kernel's back)."""
    out = dict(P)
    for n in ("dir_encoding.0", "transient_encoding.0"):
        if n + ".weight" in P:
            w = P[n + ".weight"].float()
            out[n + ".weight"] = torch.cat([w[:, :W] @ P["xyz_encoding_final.weight"].float(), w[:, W:]], 1)
            out[n + ".bias"] = P[n + ".bias"].float() + w[:, :W] @ P["xyz_encoding_final.bias"].float()
    return out


# ---- the single-product kernel on real weights ---------------------------------------------------------------------------
def encoded_inputs(inp, widths, lat, use_t, N, pe_w=None):
    """float64 side inputs of every live sample as a pass over rays encodes them (the view direction is the ray's): pe,
    dir_side [direction encoding, a], tau."""
    nx, nd, na, nt = widths
    rays, z = inp["rays"].double(), inp["z"].double()
    xyz = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    rep = lambda v: v.double().repeat_interleave(N, 0)
    w = (None, None) if pe_w is None else tuple(v.double() for v in pe_w)
    val = {"pe": orc.posenc(xyz, nx, w[0])}
    val["dir_side"] = rep(torch.cat([orc.posenc(rays[:, 3:6], nd, w[1])] + ([inp["a"].double()] if lat else []), 1))
    if use_t:
        val["tau"] = rep(inp["t"])
    return val


def x1_forward(F, val, widths, lat, use_t, *, acc=torch.float64, rounded=True, zero_bias=None):
    """field_raw (n, 9), float64, of the network on the encoded inputs `val`; `F`: fp32 parameters, the two folded layers
    folded.  rounded, acc = float64: the single-product kernel's arithmetic restated -- every layer b + half(W) half(x)
    accumulated in float64, activations fp32 between layers (`x1_64`).  rounded, acc = float32: torch's fp32 matmul in the
    accumulator's place, a CPU stand-in for the kernel.  not rounded: the same network on unrounded operands (`truth`).
    `zero_bias`: the output name of a layer that loses its bias (a deliberate defect)."""
    op = (lambda v: v.float().half().to(acc)) if rounded else (lambda v: v.to(acc))
    val = dict(val)
    n = val["pe"].shape[0]
    pre = torch.zeros(n, 9, dtype=torch.float64)
    for name, head, ins, layer in layer_table(widths, lat, use_t):
        x = torch.cat([op(val[i]) for i in ins], 1)
        b = F[layer + ".bias"].to(acc)
        y = (torch.zeros_like(b) if zero_bias == name else b) + x @ op(F[layer + ".weight"]).t()
        if head:
            pre[:, HEAD_COLS[name]] = y.double()
        else:
            val[name] = torch.relu(y).float() if rounded else torch.relu(y)
    out = head_activation(pre)
    if not use_t:
        out[:, 4:] = 0
    return out


COLUMN_NAMES = ("rgb.r", "rgb.g", "rgb.b", "sigma", "rgb_t.r", "rgb_t.g", "rgb_t.b", "sigma_t", "beta")


def x1_conditions(x1, truth, use_t):
    """Before the launch: in every head column the gap between the kernel's arithmetic and the truth is well above fp32
    rounding of the column, rms(x1_64 - truth) >= 8 * 2^-24 * max|truth|.  A list of complaints."""
    bad = []
    for c in range(9 if use_t else 4):
        gap, floor = rms(x1[:, c] - truth[:, c]), 8 * U24 * float(truth[:, c].abs().max())
        if not gap >= floor:
            bad.append(f"{COLUMN_NAMES[c]}: rms(x1_64 - truth) = {gap:.3e} is below 8 * 2^-24 * max|truth| = {floor:.3e}")
    return bad


def x1_rule(raw, x1, truth, use_t):
    """The kernel is nearer to its own arithmetic than that arithmetic is to the truth, per head column over the live samples:
    rms(kernel - x1_64) <= rms(x1_64 - truth).  Returns (complaints, column name -> ratio)."""
    raw = raw.double()
    bad, report = [], {}
    for c in range(9 if use_t else 4):
        err, gap = rms(raw[:, c] - x1[:, c]), rms(x1[:, c] - truth[:, c])
        ratio = err / gap if gap > 0 else float("inf")
        report[COLUMN_NAMES[c]] = ratio
        if not ratio <= 1.0:
            bad.append(f"{COLUMN_NAMES[c]}: rms(kernel - x1_64) = {err:.3e} is {ratio:.3f} of rms(x1_64 - truth) = {gap:.3e}")
    if not use_t and bool(raw[:, 4:].any()):
        bad.append("field_raw is not zero in the columns of a head the pass does not have")
    return bad, report
