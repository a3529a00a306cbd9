"""nfl_mlp_wgrad on its own: bit-exact against an integer reference on synthetic stashes, and against a float64 sum on the
stashes the real forward and dgrad write.  The stash formats and the operand -> gradient map come from tests/stash_codec.py,
which is written from the documentation of the formats and the model, not from the kernels' tile tables."""
import ctypes as C
import functools
import itertools
import math
import struct

import pytest
import torch

import stash_codec as sc
from oracle import nerfw_oracle as orc

pytestmark = pytest.mark.gpu

SENT = -12345.5          # sentinel of the gradient arena: whatever the call does not own must still hold it afterwards
GUARD = 8                # floats between two tensors of the arena
GMAX_SLOT = 777          # where the tests leave the pass's gradient maximum (any of the 1024 words will do)

# (n_emb_xyz, n_emb_dir, n_a, n_tau)
WIDTHS = [(10, 4, 48, 16),       # the default
          (12, 4, 40, 5),        # row (6, 6, 4) of WG_INST; partial tiles of 11, 8 and 5 features
          (3, 1, 48, 16),        # a single partial tile on both encoders
          (15, 4, 1, 1)]         # one-feature side tiles
KINDS = ["coarse", "nerfw_t", "nerfw_not"]      # plain field; appearance + transient with use_transient on / off
N_SEGS = [1, 2, 5, 37, 601]
N_MAX = max(N_SEGS)
D_MAX = 8                # most segments any instantiation keeps in flight (WG_INST)


def loss_scale(gmax):
    """nfl_loss_scale_from_bits (csrc/nfl_plan.h) of a positive normal fp32."""
    bits = struct.unpack("<I", struct.pack("<f", gmax))[0]
    e = ((bits >> 23) & 0xff) - 127
    return 1.0 if bits == 0 or e < -100 else 2.0 ** (5 - min(e, 100))


def deal_workgroups(cost, budget, n_seg):
    """Workgroups per job as nfl_wgrad_schedule deals them: proportional shares rounded down, the rest one at a time to the
    job whose workgroups carry the most each."""
    n = [min(max(budget * c // sum(cost), 1), n_seg) for c in cost]
    while sum(n) < budget:
        best = -1
        for j in range(len(cost)):
            if n[j] < n_seg and (best < 0 or cost[j] * n[best] > cost[best] * n[j]):
                best = j
        if best < 0:
            break
        n[best] += 1
    return n


def make_model(widths, kind, seed):
    """A field of these widths whose master weights read by the composition (W_dir, W_t0, W_fin, b_fin) are in {-1, 0, 1}."""
    import gpu_util
    from nerf_fl_amd import NeRF
    nx, nd, na, nt = widths
    lat = kind != "coarse"
    torch.manual_seed(seed)
    m = NeRF("fine" if lat else "coarse", in_channels_xyz=6 * nx + 3, in_channels_dir=6 * nd + 3, encode_appearance=lat,
             in_channels_a=na, encode_transient=lat, in_channels_t=nt)
    gen = torch.Generator().manual_seed(seed)
    table = torch.tensor([-1.0, 0.0, 0.0, 1.0])
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.startswith(("xyz_encoding_final", "dir_encoding.0.weight", "transient_encoding.0.weight")):
                p.copy_(table[torch.randint(0, 4, p.shape, generator=gen)])
    return m.to(gpu_util.DEV)


def draw(layout, n, gen, residual):
    """Small integers: deltas and the natural-order inputs signed, hidden activations non-negative like a relu output (half
    of them zero); residual (lo) records signed throughout."""
    out = {}
    for name, w in layout.widths().items():
        signed = residual or name.startswith(("delta", "heads")) or name in ("pe", "dir_side", "tau")
        x = torch.randint(-2, 3 if signed else 4, (n, w), generator=gen, dtype=torch.int8)
        out[name] = x if signed else x.clamp_(min=0)
    return out


def stash_buffers(f, n_rays, n_samples, BP, act_rec, grd_rec, junk=7.0):
    """Buffers of the library's sizes with the records at their heads; the tail pad, the scratch record and (unread here)
    the relu masks hold `junk`."""
    import gpu_util
    from nerf_fl_amd import _lib
    L = _lib.lib()
    out = []
    for nbytes, rec in ((L.nfl_act_stash_bytes(C.byref(f.desc), n_rays, n_samples, BP), act_rec),
                        (L.nfl_grad_stash_bytes(C.byref(f.desc), n_rays, n_samples, BP), grd_rec)):
        assert nbytes >= rec.numel() and nbytes % 2 == 0
        buf = torch.full((nbytes // 2,), junk, dtype=torch.float16, device=gpu_util.DEV).view(torch.uint8)
        buf[:rec.numel()] = rec
        out.append(buf)
    return out


@functools.lru_cache(maxsize=1)
def case_data(widths, lat, mult):
    """Operands of N_MAX segments (int8, CPU) and their stashes on the device.  A run over n_seg < N_MAX segments uses the
    first n_seg records: a stash of fewer segments is a prefix of a longer one."""
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    f = field_of(widths, "nerfw_t" if lat else "coarse")[1]
    lay = sc.Layout(*widths, nkp=sc.nkp_of_plan(f.wgrad_plan(lat)[0]), has_a=lat, has_t=lat)
    gen = torch.Generator().manual_seed(1000 * WIDTHS.index(widths) + 10 * lat + mult)
    hi = draw(lay, N_MAX * 32, gen, False)
    lo = draw(lay, N_MAX * 32, gen, True) if mult == 2 else None
    on = lambda d: None if d is None else {k: v.to(gpu_util.DEV) for k, v in d.items()}
    # unnamed positions of the records (padding features) hold 7: a tile that took them for real would show
    act_rec, grd_rec = lay.encode(on(hi), on(lo), fill=7.0)
    BP = rnd._BPREC["f16x3" if mult == 2 else "f16"]
    act, grd = stash_buffers(f, N_MAX, 32, BP, act_rec, grd_rec)
    return lay, hi, lo, act, grd


@functools.lru_cache(maxsize=1)
def largest_magnitude(widths, kind, mult):
    """Largest sum of |terms| over every element of every gradient of the N_MAX-segment case, composed ones and G included."""
    lay, hi, lo, _, _ = case_data(widths, kind != "coarse", mult)
    params = {k: v.detach().cpu() for k, v in field_of(widths, kind)[0].named_parameters()}
    mag = sc.reference_grads(lay, hi, lo, params, kind == "nerfw_t", absolute=True)
    return max(float(v.max()) for v in mag.values())


@functools.lru_cache(maxsize=4)
def field_of(widths, kind):
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    model = make_model(widths, kind, 17 + WIDTHS.index(widths))
    return model, rnd._field(model, widths[0], widths[1], torch.device(gpu_util.DEV), pack=False)


def run_wgrad(f, use_t, act, grd, gmax_value, n_rays, n_samples, backward, leave_out=()):
    """nfl_mlp_wgrad into a sentinel-filled arena with guards between the tensors.  Returns name -> gradient on the CPU (the
    tensors of the layers in `leave_out` get NULL pointers; their places in the arena are returned like the others), after
    checking that nothing outside the tensors the call was given has been written."""
    import gpu_util
    from nerf_fl_amd import _lib, rendering as rnd
    L, dev = _lib.lib(), gpu_util.DEV
    plist = f.param_list()
    where, off = {}, GUARD
    for i, w, b in plist:
        for suffix, p in ((".weight", w), (".bias", b)):
            where[_lib.LAYER_NAMES[i] + suffix] = (off, p.numel(), tuple(p.shape), i)
            off += (p.numel() + 3) // 4 * 4 + GUARD
    arena = torch.full((off,), SENT, dtype=torch.float32, device=dev)
    place = lambda name: arena[where[name][0]:where[name][0] + where[name][1]]
    targets = {i: (place(_lib.LAYER_NAMES[i] + ".weight"), place(_lib.LAYER_NAMES[i] + ".bias"))
               for i, _, _ in plist if _lib.LAYER_NAMES[i] not in leave_out}
    gmax = torch.zeros(_lib.NFL_GMAX_SLOTS, dtype=torch.float32, device=dev)
    gmax[GMAX_SLOT] = gmax_value
    scratch = torch.empty(L.nfl_wgrad_scratch_bytes() // 4, dtype=torch.float32, device=dev)
    rnd._run_wgrad(f, act, grd, gmax, n_rays, n_samples, use_t=use_t, bprec=rnd._BPREC[backward], targets=targets,
                   scratch=scratch)
    torch.cuda.synchronize()
    host = arena.cpu()
    got = {name: host[o:o + n].view(shape).clone() for name, (o, n, shape, _) in where.items()}
    owned = torch.zeros(off, dtype=torch.bool)
    for name, (o, n, _, i) in where.items():
        if _lib.LAYER_NAMES[i] not in leave_out:
            owned[o:o + n] = True
    stray = (host[~owned] != SENT).nonzero().flatten()
    assert stray.numel() == 0, f"{stray.numel()} floats outside the gradient tensors were written"
    return got


def describe(got, exp):
    bad = (got != exp).nonzero()
    rows, cols = sorted(set(bad[:, 0].tolist())), sorted(set(bad[:, -1].tolist()))
    d = (got.double() - exp.double())[got != exp]
    return (f"{bad.shape[0]} of {got.numel()} elements differ; rows {rows[:12]}{'...' if len(rows) > 12 else ''} "
            f"cols {cols[:12]}{'...' if len(cols) > 12 else ''}; first {bad[0].tolist()} got {got[tuple(bad[0])].item()} "
            f"expected {exp[tuple(bad[0])].item()}; differences {d.min().item()} .. {d.max().item()}")


# every width set x field kind x arithmetic x segment count at loss scale 1, then: f16w (shares f16's kernel), a pass whose
# loss scale is 2^12, and a call that leaves the rgb head out
CASES = [(w, k, b, n, "") for w, b, k, n in itertools.product(WIDTHS, ["f16", "f16x3"], KINDS, N_SEGS)]
CASES += [(WIDTHS[0], "nerfw_t", "f16w", 37, ""), (WIDTHS[0], "nerfw_t", "f16x3", 37, "scale12"),
          (WIDTHS[0], "nerfw_t", "f16x3", 37, "no_rgb"), (WIDTHS[1], "coarse", "f16", 37, "no_rgb")]


@pytest.mark.parametrize("widths,kind,backward,n_seg,variant", CASES,
                         ids=["-".join(["x".join(map(str, c[0])), c[1], c[2], f"n{c[3]}"] + ([c[4]] if c[4] else []))
                              for c in CASES])
def test_wgrad_exact_on_integer_stashes(widths, kind, backward, n_seg, variant):
    """fp16 operands, fp32 accumulators: with small integers in the stashes every product and every partial sum is exact,
    whatever the order, so every element of every weight and bias gradient -- the composed ones through xyz_encoding_final
    included -- must EQUAL the integer reference: one segment lost, read twice or credited to the wrong element shows.

    Segment counts: 1, 2, 5 are fewer than any job has workgroups (the `live` clamp of the reduction, the early return of
    the stream kernel); at 37 some jobs have idle workgroups and some do not; 601 is the steady state of every pipeline: the
    schedule deals min(CUs, 256) workgroups to the jobs in proportion to their cost classes (4..8 of a total of 82..107
    per field), so no job has more than about 26 of 256 and every workgroup takes at least 601 // 26 = 23 segments
    round-robin -- more than 2 D for the deepest pipeline (D = 8), and 601 = 23 * 26 + 3 leaves remainders that are no
    multiple of any D in 2..8 for most workgroup counts.  (Asserted below from the plan's cost classes when the device has
    at least 64 CUs; with fewer the run still happens, the claim is not made.)"""
    import gpu_util
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    mult = 2 if backward == "f16x3" else 1
    model, f = field_of(widths, kind)
    lay, hi_all, lo_all, act, grd = case_data(widths, lat, mult)
    n = n_seg * 32
    hi = {k: v[:n] for k, v in hi_all.items()}
    lo = None if lo_all is None else {k: v[:n] for k, v in lo_all.items()}
    params = {k: v.detach().cpu() for k, v in model.named_parameters()}
    gmax_value = 2.0 ** -7 if variant == "scale12" else 32.0
    scale = loss_scale(gmax_value)
    assert scale == (4096.0 if variant == "scale12" else 1.0)

    # the condition that makes "exact in any order" true, then the reference (float64 matmuls of integers: exact) -- both
    # on the CPU, before the GPU runs.  The magnitudes of the first n_seg segments are at most those of all N_MAX (sums of
    # non-negative terms), which are computed once per stash
    worst = largest_magnitude(widths, kind, mult)
    assert worst < 2.0 ** 24, f"sum of |terms| reaches {worst}: the value ranges are too wide for an exact test"
    ref = sc.reference_grads(lay, hi, lo, params, use_t)
    assert all(torch.equal(v, v.round()) and float(v.abs().max()) <= worst for v in ref.values())

    if n_seg == N_MAX and torch.cuda.get_device_properties(0).multi_processor_count >= 64:
        ncu = min(torch.cuda.get_device_properties(0).multi_processor_count, 256)
        from nerf_fl_amd import _lib
        h_wp = f.wgrad_plan(use_t)[0]
        n_jobs = (C.c_int32 * 2).from_buffer(h_wp)[1]
        c0 = 4 + 2 * _lib.NFL_NUM_LAYERS          # WgPlan: magic, n_jobs, act_slots, grd_slots, w_numel[], b_numel[], cost[]
        cost = list((C.c_int32 * (c0 + n_jobs)).from_buffer(h_wp)[c0:])
        assert 8 <= n_jobs <= 20 and all(4 <= c <= 8 for c in cost), cost
        n_wg = deal_workgroups(cost, ncu, n_seg)
        assert n_seg // max(n_wg) > 2 * D_MAX, (cost, n_wg)

    leave_out = ("static_rgb.0",) if variant == "no_rgb" else ()
    got = run_wgrad(f, use_t, act, grd, gmax_value, n_seg, 32, backward, leave_out)
    bad = {}
    for name, g in got.items():
        layer = name.rsplit(".", 1)[0]
        if layer in leave_out:
            exp = torch.full_like(g, SENT)                   # neither tensor of a head left out is touched
        elif name in ref:
            exp64 = (ref[name] / scale).view_as(g)           # a power of two: exact
            exp = exp64.float()
            assert torch.equal(exp.double(), exp64)
        else:
            exp = torch.zeros_like(g)                        # transient layers of a pass that does not use them
        if not torch.equal(g, exp):
            bad[name] = describe(g, exp)
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())


# ---- the stashes the real producers write ----------------------------------------------------------------------------
def exact_rays(R, N, seed):
    """Rays and sorted depths on a 1/64 grid: o + d z is exact in fp32 (with or without fma), so the float64 position
    encoding sees the very points the kernel encodes."""
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.0, 4.0]) + torch.randint(-8, 9, (R, 3), generator=gen) / 64.0
    d = torch.randint(-24, 25, (R, 3), generator=gen) / 64.0
    d[:, 2] = -torch.randint(52, 65, (R,), generator=gen) / 64.0
    z = torch.stack([torch.sort(128 + torch.randperm(256, generator=gen)[:N])[0] for _ in range(R)]) / 64.0
    rays = torch.cat([o, d, torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)], 1)
    return rays.float(), z.float()


REAL_FWD_ATOL = 2e-5      # what test_parity_gpu.py::test_field_raw_vs_oracle grants the forward of these fields


@pytest.mark.parametrize("backward", ["f16", "f16x3"])
@pytest.mark.parametrize("kind", ["coarse", "nerfw"])
@pytest.mark.parametrize("R,N", [(3, 40), (40, 64)])
def test_wgrad_on_real_stashes(R, N, kind, backward):
    """Training forward -> composite backward -> dgrad write the stashes; the codec decodes them.
    1. The decoded h_1..h_8 of every live sample are the trunk evaluated in float64 from the same weights, to fp16
       rounding (2^-10 relative; 2^-20 for hi + lo) plus the forward's own 2e-5.
    2. nfl_mlp_wgrad on these stashes equals the float64 sum over the LIVE samples only of the decoded operands, every
       element within N_live * 2^-24 * sum|terms| (fp32 summation's worst case, a ceiling): the padded lanes of a ray's
       last segment (R = 3, 40 samples: 8 live lanes of 32) contribute nothing to any dW or db.
    Largest |error| / bound over all elements of all tensors, as measured on the MI355X (printed per case):
        R = 3,  N = 40:  coarse f16 3.0e-2, f16x3 4.1e-2;  nerfw f16 5.0e-2, f16x3 5.1e-2
        R = 40, N = 64:  coarse f16 1.6e-3, f16x3 1.8e-3;  nerfw f16 1.6e-3, f16x3 2.1e-3
    (the bound grows with N, the error with about sqrt(N)); the decoded h_l reach 0.49 of their tolerance with fp16
    stashes (fp16 rounding to nearest is 2^-11) and 0.04 with hi + lo."""
    import gpu_util
    import nerf_fl_amd
    from nerf_fl_amd import _lib, rendering as rnd
    dev = gpu_util.DEV
    lat = kind == "nerfw"
    BP = rnd._BPREC[backward]
    mult = 2 if backward == "f16x3" else 1
    spec = orc.FieldSpec("fine", encode_appearance=True, encode_transient=True, beta_min=0.1) if lat else orc.FieldSpec("coarse")
    P = orc.make_field_params(spec, 81 + lat, "sharp")
    model = gpu_util.module_from(spec, P)
    f = rnd._field(model, 10, 4, torch.device(dev), prec=rnd._PREC["f16x3"])
    f.ensure_bwd_packed(False, BP)
    rays, z = exact_rays(R, N, 5 * R + N)
    gen = torch.Generator().manual_seed(R + N)
    a_emb = torch.randn(R, 48, generator=gen).to(dev) if lat else None
    t_emb = torch.randn(R, 16, generator=gen).to(dev) if lat else None
    rays_d, z_d = rays.to(dev), z.to(dev)
    out = rnd._run_pass(f, rays_d, N, z=z_d, noise=None, noise_std=0.0, white_back=True, a_emb=a_emb, t_emb=t_emb,
                        stash=True, bprec=BP)
    # composite backward with a generic upstream gradient on every output the pass has
    g = {k: (torch.randn(*s, generator=gen) * 1e-2).to(dev) for k, s in
         dict(weights=(R, N), opacity=(R,), rgb=(R, 3), depth=(R,), tsig=(R, N), beta=(R,), rgb_s=(R, 3), rgb_t=(R, 3)).items()}
    up = [g[k] for k in ("weights", "opacity", "rgb", "depth")] + ([g[k] for k in ("tsig", "beta", "rgb_s", "rgb_t")] if lat else [None] * 4)
    gmax = torch.zeros(_lib.NFL_GMAX_SLOTS, dtype=torch.float32, device=dev)
    head, gmax = rnd._run_compbwd(out["field_raw"], z_d, R, N, noise=None, noise_std=0.0, use_t=lat, white_back=True, grads=up,
                                  go=None, g_tsig_const=0.0, gmax=gmax)
    grad_stash = rnd._run_dgrad(f, out["act_stash"], head, gmax, R, N, use_t=lat, bprec=BP)
    torch.cuda.synchronize()
    gmax_value = float(gmax.max())
    assert gmax_value > 0
    scale = loss_scale(gmax_value)
    got = run_wgrad(f, lat, out["act_stash"], grad_stash, gmax_value, R, N, backward)

    spr = (N + 31) // 32
    n_seg = R * spr
    lay = sc.Layout(10, 4, 48, 16, nkp=sc.nkp_of_plan(f.wgrad_plan(lat)[0]), has_a=lat, has_t=lat)
    hi, lo = lay.decode(out["act_stash"].cpu(), grad_stash.cpu(), n_seg, mult)
    i = torch.arange(N)
    rows = ((torch.arange(R)[:, None] * spr + i[None, :] // 32) * 32 + i[None, :] % 32).flatten()      # (ray, sample) order

    # 1. the stashed activations are the trunk's
    P64 = {k: v.double() for k, v in P.items()}
    xyz = rays[:, None, 0:3].double() + rays[:, None, 3:6].double() * z[..., None].double()
    pe = orc.posenc(xyz.reshape(-1, 3), 10)
    rel = 2.0 ** -20 if mult == 2 else 2.0 ** -10
    h, worst_h = pe, 0.0
    for l in range(1, 9):
        x = torch.cat([pe, h], 1) if l == 5 else h
        h = torch.relu(x @ P64[f"xyz_encoding_{l}.0.weight"].t() + P64[f"xyz_encoding_{l}.0.bias"])
        dec = hi[f"h{l}"][rows].double() + (lo[f"h{l}"][rows].double() if lo is not None else 0.0)
        ratio = ((dec - h).abs() / (rel * h.abs() + REAL_FWD_ATOL)).max().item()
        worst_h = max(worst_h, ratio)
        assert ratio <= 1.0, f"h{l}: |decoded - float64 trunk| reaches {ratio:.3f} of its tolerance"

    # 2. the weight gradients are the sum over the live samples of the decoded operands
    ref = sc.reference_grads(lay, hi, lo, P64, lat, rows=rows)
    mag = sc.reference_grads(lay, hi, lo, P64, lat, rows=rows, absolute=True)
    n_live = R * N
    worst, bad = 0.0, {}
    for name, gt in got.items():
        exp = ref[name].view_as(gt) / scale
        bound = n_live * 2.0 ** -24 * mag[name].view_as(gt) / scale
        err = (gt.double() - exp).abs()
        assert float(exp.abs().max()) > 0, name
        ratio = float(torch.where(bound > 0, err / bound.clamp(min=1e-300), (err > 0).double() * float("inf")).nan_to_num(nan=0.0, posinf=float("inf")).max())
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            bad[name] = ratio
    print(f"real stashes R={R} N={N} {kind} {backward}: loss scale 2^{int(math.log2(scale))}, "
          f"h within {worst_h:.3f} of its tolerance, largest |dW error| / (N 2^-24 sum|terms|) = {worst:.3e}")
    assert not bad, bad
