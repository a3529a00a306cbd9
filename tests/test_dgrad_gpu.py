"""nfl_mlp_dgrad on its own: every delta of every layer EQUAL to a float64 integer reference on synthetic inputs, in all three
arithmetics.  The stash formats and the mask records come from tests/stash_codec.py (written from the documentation of the
formats); the reference chain below is the model's, delta_{l-1} = mask (.) W_l^T delta_l, written from models/nerf.py.
Then on the real forward's masks with dense weights, layer by layer from the decoded deltas, within bounds that follow from
the number formats; and the ray gradient against the float64 chain through the encodings.

Which axes meet.  The default widths meet every field kind, ray shape and arithmetic (36 cases): the tiling depends on the
shape and the arithmetic (NCB, TPC), the stream on the kind.  The wide encoder (15 frequencies: the kernels' second
translation unit, with one-feature latent tiles) meets the two kinds that change its stream and the two shapes with partial
workgroups and several tiles; (12, 4, 40, 5) -- a partial second appearance tile -- runs once per arithmetic, as do the
2^12 loss scale and the table form of the latent gradients, which do not interact with the tiling."""
import ctypes as C
import functools
import itertools

import pytest
import torch

import stash_codec as sc
from oracle import nerfw_oracle as orc
from test_wgrad_gpu import REAL_FWD_ATOL, exact_rays, loss_scale

pytestmark = pytest.mark.gpu

SENT_BYTE = 0xA5         # sentinel of the gradient stash's surroundings
GUARD = 8192             # bytes before and behind the gradient stash
GMAX_SLOT = 777
W = 256

# (n_emb_xyz, n_emb_dir, n_a, n_tau): the second appearance tile of n_a - 32 rows full, empty, partial
WIDTHS = [(10, 4, 48, 16), (15, 4, 1, 1), (12, 4, 40, 5)]
KINDS = ["coarse", "nerfw_t", "nerfw_not"]      # plain field; appearance + transient with use_transient on / off
# (R, N).  A workgroup takes 4 NCB segments per tile (NCB 2 for f16, 1 otherwise; nfl_ray_split in nfl_launch.cpp):
SHAPES = [(1, 1),        # one live lane
          (9, 40),       # several rays per workgroup, a partial last workgroup, 8 live lanes in each ray's second segment
          (3, 300),      # 10 segments per ray: two or three tiles per workgroup -- the ring's wrap to c_start, the clamped
                         # seg_issue, a partly idle last tile
          (2, 1024)]     # four / eight full tiles
ARITH = ["f16", "f16w", "f16x3"]
FANIN = 2                # non-zeros per input column of every weight


def sparse_ternary(out_f, in_f, gen):
    """Entries in {-1, 0, 1}: FANIN non-zeros in every column (all of them where the layer has fewer rows), then one more in
    every row that got none: every row and every column is used."""
    k = min(FANIN, out_f)
    rows = torch.rand(out_f, in_f, generator=gen).argsort(0)[:k]
    w = torch.zeros(out_f, in_f)
    w[rows, torch.arange(in_f).expand(k, in_f)] = (2 * torch.randint(0, 2, (k, in_f), generator=gen) - 1).float()
    for i in (w.abs().sum(1) == 0).nonzero().flatten().tolist():
        w[i, int(torch.randint(0, in_f, (1,), generator=gen))] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def make_model(widths, kind):
    """A field of these widths (on the CPU) whose every weight is ternary and sparse; biases zero (dgrad reads none)."""
    from nerf_fl_amd import NeRF
    nx, nd, na, nt = widths
    lat = kind != "coarse"
    torch.manual_seed(5)
    m = NeRF("fine" if lat else "coarse", in_channels_xyz=6 * nx + 3, in_channels_dir=6 * nd + 3, encode_appearance=lat,
             in_channels_a=na, encode_transient=lat, in_channels_t=nt)
    gen = torch.Generator().manual_seed(31 + WIDTHS.index(widths))
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(sparse_ternary(*p.shape, gen) if n.endswith("weight") else torch.zeros_like(p))
    return m


def padded_rows(R, N):
    """Row of the (n_seg * 32)-row stash tensors that holds (ray, sample), in (ray, sample) order."""
    spr = (N + 31) // 32
    i = torch.arange(N)
    return ((torch.arange(R)[:, None] * spr + i[None, :] // 32) * 32 + i[None, :] % 32).flatten()


def draw_masks(has_t, n_rows, gen):
    """Random bits; rows 3, 14, 25, .. have an all-zero h3 and dirh (the chain below dies there), rows 5, 16, .. an all-one h6
    and g2."""
    masks = {n: torch.randint(0, 2, (n_rows, 32 * tiles), generator=gen).bool() for n, (_, tiles) in sc.mask_fields(has_t).items()}
    r = torch.arange(n_rows)
    masks["h3"][r % 11 == 3] = False
    masks["dirh"][r % 11 == 3] = False
    masks["h6"][r % 11 == 5] = True
    if has_t:
        masks["g2"][r % 11 == 5] = True
    return masks


def reference_chain(params, widths, masks, head, use_t, has_a):
    """float64 deltas (name -> (rows, width)) and the per-row latent gradient terms from the head gradients `head`
    ((rows, 9) in the kernel's order [rgb, sigma, rgb_t, sigma_t, beta], already multiplied by the loss scale), the masks and
    the weights.  d(feat) goes straight through xyz_encoding_final: W' = W[:, :256] W_fin, as the packed streams hold it."""
    nx, nd, na, nt = widths
    cx, cd = 6 * nx + 3, 6 * nd + 3
    P = lambda n: params[n + ".weight"].double()
    m = lambda n: masks[n].double()
    head = head.double()
    d = {"heads0": head[:, 3:4], "heads1": head[:, 0:3]}
    d["delta_dirh"] = m("dirh") * (d["heads1"] @ P("static_rgb.0"))
    wfin = P("xyz_encoding_final")
    pre8 = d["delta_dirh"] @ (P("dir_encoding.0")[:, :W] @ wfin) + d["heads0"] @ P("static_sigma.0")
    lat = {}
    if has_a:
        lat["a"] = d["delta_dirh"] @ P("dir_encoding.0")[:, W + cd:W + cd + na]
    if use_t:
        d.update(heads2=head[:, 7:8], heads3=head[:, 4:7], heads4=head[:, 8:9])
        g = m("g4") * (d["heads2"] @ P("transient_sigma.0") + d["heads3"] @ P("transient_rgb.0") + d["heads4"] @ P("transient_beta.0"))
        d["delta_g4"] = g
        for k, j in ((3, 6), (2, 4), (1, 2)):
            g = m(f"g{k}") * (g @ P(f"transient_encoding.{j}"))
            d[f"delta_g{k}"] = g
        pre8 = pre8 + g @ (P("transient_encoding.0")[:, :W] @ wfin)
        lat["t"] = g @ P("transient_encoding.0")[:, W:W + nt]
    x = m("h8") * pre8
    d["delta8"] = x
    for l in range(8, 1, -1):
        x = x @ P(f"xyz_encoding_{l}.0")
        x = m(f"h{l - 1}") * (x[:, cx:] if l == 5 else x)
        d[f"delta{l - 1}"] = x
    return d, lat


def latent_sums(lat_rows, R, N, scale, latent_row=None, n_vocab=None):
    """g_a / g_t: the rows' terms summed over the ray's live samples, divided by the loss scale; with `latent_row` summed
    further into the table's rows (duplicates add)."""
    rows = padded_rows(R, N)
    out = {}
    for k, v in lat_rows.items():
        per_ray = v[rows].view(R, N, -1).sum(1) / scale
        if latent_row is not None:
            per_ray = torch.zeros(n_vocab, per_ray.shape[1], dtype=torch.float64).index_add_(0, latent_row, per_ray)
        out[k] = per_ray
    return out


def exactness_violations(deltas, R, N):
    """The conditions under which 'equal in every arithmetic' holds, and under which the case proves something: every
    scaled delta an integer of magnitude <= 2048 (fp16 holds it exactly, so nearest, stochastic and split rounding all leave
    it alone; every partial sum is an integer below 2^24, exact in fp32 in any order), and non-zero values in every 32-feature
    tile of every layer.  Returns a list of complaints."""
    bad = []
    live = padded_rows(R, N)
    for name, v in deltas.items():
        if not torch.equal(v, v.round()) or float(v.abs().max()) > 2048:
            bad.append(f"{name}: not integers within 2048 (max {float(v.abs().max())})")
        if name.startswith("delta"):
            tiles = v[live].abs().sum(0).view(-1, 32).sum(1)
            if bool((tiles == 0).any()):
                bad.append(f"{name}: feature tiles {(tiles == 0).nonzero().flatten().tolist()} are zero everywhere")
        if not v[live].any():
            bad.append(f"{name}: zero everywhere")
    return bad


def mismatches(got, exp, R, N, lo=None):
    """name -> description of where got != exp (both name -> (rows, width)), with the layer, ray, sample and tile of the
    first difference; every row that is not a live sample must be zero; `lo`: records that must be zero altogether."""
    spr = (N + 31) // 32
    live = torch.zeros(R * spr * 32, dtype=torch.bool)
    live[padded_rows(R, N)] = True
    out = {}
    for name, e in exp.items():
        g = got[name].double()
        e = torch.where(live[:, None], e, torch.zeros_like(e))            # the padded tail of a ray: exactly zero
        for what, x, y in ((name, g, e),) + (((name + " (lo record)", lo[name].double(), torch.zeros_like(e)),) if lo is not None else ()):
            bad = (x != y).nonzero()
            if bad.numel():
                row, col = bad[0].tolist()
                seg, lane = divmod(row, 32)
                rays = sorted(set((bad[:, 0] // 32 // spr).tolist()))
                out[what] = (f"{bad.shape[0]} of {x.numel()} differ; first at ray {seg // spr} sample {(seg % spr) * 32 + lane} "
                             f"({'live' if live[row] else 'padded'}; segment {seg} lane {lane}) feature {col} (tile {col // 32}): got "
                             f"{x[row, col].item()} expected {y[row, col].item()}; rays {rays[:8]} tiles "
                             f"{sorted(set((bad[:, 1] // 32).tolist()))}")
    return out


def latent_mismatches(got, exp):
    out = {}
    for k, e in exp.items():
        g = got[k].double()
        if not torch.equal(g, e):
            bad = (g != e).nonzero()
            out["g_" + k] = f"{bad.shape[0]} of {e.numel()} differ; first at row {bad[0, 0].item()} column {bad[0, 1].item()}: got {g[tuple(bad[0])].item()} expected {e[tuple(bad[0])].item()}"
    return out


@functools.lru_cache(maxsize=None)
def host_case(widths, kind, R, N, gmax_value):
    """Masks, head gradients and the reference of one case, on the CPU (shared by the arithmetics and by
    tests/test_backward_refs_cpu.py)."""
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    spr = (N + 31) // 32
    n_rows = R * spr * 32
    gen = torch.Generator().manual_seed(100 * R + N + 7 * KINDS.index(kind) + WIDTHS.index(widths))
    masks = draw_masks(lat, n_rows, gen)
    scale = loss_scale(gmax_value)
    ints = torch.zeros(n_rows, 9)
    live = torch.randint(-2, 3, (R, N, 9), generator=gen).float()
    live[:, 0] = torch.where(live[:, 0] == 0, torch.ones(R, 9), live[:, 0])      # a ray's first sample: no head gradient is zero
    ints[padded_rows(R, N)] = live.view(R * N, 9)
    if not use_t:
        ints[:, 4:] = 0
    params = dict(make_model(widths, kind).named_parameters())
    deltas, lat_rows = reference_chain({k: v.detach() for k, v in params.items()}, widths, masks, ints, use_t, lat)
    return masks, ints, scale, deltas, lat_rows


@functools.lru_cache(maxsize=4)
def field_of(widths, kind):
    import copy
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    model = copy.deepcopy(make_model(widths, kind)).to(gpu_util.DEV)
    return model, rnd._field(model, widths[0], widths[1], torch.device(gpu_util.DEV), pack=False)


def run_dgrad(f, lay, masks, head, gmax_value, R, N, use_t, backward, lat, latent_row=None, n_vocab=None, act_stash=None,
              **ray_kw):
    """nfl_mlp_dgrad with the gradient stash inside a sentinel-filled buffer.  The activation RECORDS hold fp16 NaN: the
    kernel must read only the masks behind them.  Returns (hi, lo, g_a, g_t) on the CPU after checking that nothing beyond
    the n_seg + 1 records (the scratch record of padded segments included) was written."""
    import gpu_util
    from nerf_fl_amd import _lib, rendering as rnd
    L, dev = _lib.lib(), gpu_util.DEV
    BP = rnd._BPREC[backward]
    mult = 2 if backward == "f16x3" else 1
    n_seg = R * ((N + 31) // 32)
    f.ensure_bwd_packed(bool(ray_kw), BP)
    if act_stash is None:
        nb = L.nfl_act_stash_bytes(C.byref(f.desc), R, N, BP)
        off = sc.mask_offset(n_seg, lay.nkp, mult)
        assert nb == off + n_seg * sc.MSK_WORDS * 256
        act_stash = torch.full((nb // 2,), float("nan"), dtype=torch.float16).view(torch.uint8)
        act_stash[off:] = sc.encode_masks(masks, lay.has_t)
        act_stash = act_stash.to(dev)
    ng = L.nfl_grad_stash_bytes(C.byref(f.desc), R, N, BP)
    owned = (n_seg + 1) * sc.GRD_SLOTS * mult * 1024
    assert ng >= owned
    arena = torch.full((GUARD + ng + GUARD,), SENT_BYTE, dtype=torch.uint8, device=dev)
    gmax = torch.zeros(_lib.NFL_GMAX_SLOTS, dtype=torch.float32, device=dev)
    gmax[GMAX_SLOT] = gmax_value
    rows_out = n_vocab if latent_row is not None else R
    g_a = torch.zeros(rows_out, f.desc.n_a, dtype=torch.float32, device=dev) if lat else None
    g_t = torch.zeros(rows_out, f.desc.n_tau, dtype=torch.float32, device=dev) if (lat and use_t) else None
    rnd._run_dgrad(f, act_stash, head.to(dev), gmax, R, N, use_t=use_t, bprec=BP, grad_stash=arena[GUARD:GUARD + ng], g_a=g_a,
                   g_t=g_t, latent_row=None if latent_row is None else latent_row.to(dev), rays_grad=bool(ray_kw), **ray_kw)
    torch.cuda.synchronize()
    host = arena.cpu()
    stray = (host[:GUARD] != SENT_BYTE).sum() + (host[GUARD + owned:] != SENT_BYTE).sum()
    assert int(stray) == 0, f"{int(stray)} bytes outside the {n_seg} + 1 gradient records were written"
    rec = sc.Layout._records(host[GUARD:GUARD + ng], n_seg, sc.GRD_SLOTS, mult)
    hi = sc.Layout._get(rec[:, 0], lay.grd)
    lo = sc.Layout._get(rec[:, 1], lay.grd) if mult == 2 else None
    return hi, lo, None if g_a is None else g_a.cpu(), None if g_t is None else g_t.cpu()


def live_head(ints, scale, R, N):
    """The (R N, 9) fp32 head gradient whose scaled values are the integers `ints` (padded rows layout)."""
    head = ints[padded_rows(R, N)] / scale
    assert torch.equal(head.float().double() * scale, ints[padded_rows(R, N)].double())
    return head.float().contiguous()


CASES = [(WIDTHS[0], k, s, b, "") for k, s, b in itertools.product(KINDS, SHAPES, ARITH)]
CASES += [(WIDTHS[1], k, s, b, "") for k, s, b in itertools.product(["coarse", "nerfw_t"], SHAPES[1:3], ARITH)]
CASES += [(WIDTHS[2], "nerfw_t", SHAPES[1], b, "") for b in ARITH]
CASES += [(WIDTHS[0], "nerfw_t", SHAPES[1], b, "scale12") for b in ("f16", "f16x3")]
CASES += [(w, "nerfw_t", SHAPES[1], b, "table") for w in WIDTHS for b in ("f16", "f16x3")]
HOST_CASES = sorted({(c[0], c[1], c[2][0], c[2][1], 2.0 ** -7 if c[4] == "scale12" else 32.0) for c in CASES})


@pytest.mark.parametrize("widths,kind,shape,backward,variant", CASES,
                         ids=["-".join(["x".join(map(str, c[0])), c[1], f"R{c[2][0]}N{c[2][1]}", c[3]] + ([c[4]] if c[4] else []))
                              for c in CASES])
def test_dgrad_exact_on_integers(widths, kind, shape, backward, variant):
    """Ternary sparse weights in every layer, small-integer head gradients, random relu masks and a chosen loss scale: the fold
    W' = W[:, :256] W_fin that nfl_compose_forward computes in fp32 is exact, so is every product and every sum, and a value
    fp16 represents is unchanged by nearest, stochastic and split rounding alike.  So every delta of every layer -- the heads'
    records included -- must EQUAL the float64 integer reference in all three arithmetics, every residual (lo) record must
    be zero, every lane of a ray's padded tail must be zero, and the latent gradients (sums of integers times a power of two:
    exact under any atomic order) must equal their sums, per ray or through latent_row with duplicate rows.  The conditions
    (integers within 2048, something non-zero in every tile of every layer) are asserted on the CPU before the GPU runs.
    With use_transient off on a field that has the head (nerfw_not) the transient records are not written and delta8 must
    carry no transient term."""
    R, N = shape
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    gmax_value = 2.0 ** -7 if variant == "scale12" else 32.0
    masks, ints, scale, deltas, lat_rows = host_case(widths, kind, R, N, gmax_value)
    assert scale == (4096.0 if variant == "scale12" else 1.0)
    bad = exactness_violations(deltas, R, N)
    assert not bad, bad

    model, f = field_of(widths, kind)
    lay = sc.Layout(*widths, nkp=sc.nkp_of_plan(f.wgrad_plan(lat)[0]), has_a=lat, has_t=lat)
    latent_row = n_vocab = None
    if variant == "table":
        n_vocab = 5
        latent_row = torch.tensor([3, 0, 3, 3, 1, 0, 4, 3, 1][:R], dtype=torch.int64)            # row 2 is never named
    hi, lo, g_a, g_t = run_dgrad(f, lay, masks, live_head(ints, scale, R, N), gmax_value, R, N, use_t, backward, lat,
                                 latent_row, n_vocab)
    wrong = mismatches(hi, deltas, R, N, lo)
    exp_lat = latent_sums(lat_rows, R, N, scale, latent_row, n_vocab)
    wrong.update(latent_mismatches({"a": g_a, "t": g_t}, exp_lat))
    if kind == "nerfw_not":         # the transient head's records are not written: they still hold the arena's sentinel bytes
        untouched = torch.tensor([SENT_BYTE, SENT_BYTE], dtype=torch.uint8).view(torch.int16)
        for name in [f"delta_g{m}" for m in range(1, 5)] + ["heads2", "heads3", "heads4"]:
            for rec in (hi, lo) if lo is not None else (hi,):
                if not bool((rec[name].contiguous().view(torch.int16) == untouched).all()):
                    wrong[name + " (use_transient off)"] = "written although the pass does not use the transient head"
    assert not wrong, "\n".join(f"{k}: {v}" for k, v in wrong.items())


# ---- the real forward's masks, dense weights, layer by layer ---------------------------------------------------------------
U24 = 2.0 ** -24
# per arithmetic: (eps_w: what the packed transposed weights lose, eps_out: what a stored delta loses)
#   f16    weights and deltas are single fp16 images rounded stochastically: up to a full ulp, 2^-10 of the value
#   f16w   weights hi + lo (2^-21: lo is the fp16 image of a residual of at most 2^-11 of the value), deltas as f16
#   f16x3  weights and deltas hi + lo (2^-21 each); of the four products the kernel omits lo * lo, at most 2^-22 of the term
EPS = {"f16": (2.0 ** -10, 2.0 ** -10), "f16w": (2.0 ** -21, 2.0 ** -10), "f16x3": (2.0 ** -21 + 2.0 ** -22, 2.0 ** -21)}
# The relative figures hold for normal fp16 images only.  The lo image of a weight |w| < 2^-3 is a SUBNORMAL fp16 (the
# residual of hi is below 2^-14; nfl_pack.hip stores it unscaled), so hi + lo holds such a weight to half the subnormal step,
# 2^-25 absolute, whatever its size: of the `sharp` weights (median |w| = 0.03) half are held worse than 2^-21, static_rgb's
# smallest to 800 * 2^-21.  Each weight's fp16 subnormal step therefore enters the bound times the operand it multiplies:
# 2^-25 sum_k |delta^_k| for hi + lo (rounded to nearest), 2^-24 for the single stochastically rounded image of f16.
W_STEP = {"f16": 2.0 ** -24, "f16w": 2.0 ** -25, "f16x3": 2.0 ** -25}


def layer_inputs(P, cx, use_t):
    """output field -> (mask name or None, [(input field, W (out x in) float64, |W| as the kernel's arithmetic sees it,
    extra relative error of that matrix)]).  The folded matrices W' = W[:, :256] W_fin are formed in fp32 by
    nfl_compose_forward: 256 products and sums, so up to 256 * 2^-24 of |W[:, :256]| |W_fin|."""
    w = lambda n: P[n + ".weight"]
    fold = lambda n: (w(n)[:, :W] @ w("xyz_encoding_final"), w(n)[:, :W].abs() @ w("xyz_encoding_final").abs(), 256 * U24)
    plain = lambda m: (m, m.abs(), 0.0)
    out = {"delta_dirh": ("dirh", [("heads1",) + plain(w("static_rgb.0"))])}
    d8 = [("delta_dirh",) + fold("dir_encoding.0"), ("heads0",) + plain(w("static_sigma.0"))]
    if use_t:
        out["delta_g4"] = ("g4", [("heads2",) + plain(w("transient_sigma.0")), ("heads3",) + plain(w("transient_rgb.0")),
                                  ("heads4",) + plain(w("transient_beta.0"))])
        for k, j in ((3, 6), (2, 4), (1, 2)):
            out[f"delta_g{k}"] = (f"g{k}", [(f"delta_g{k + 1}",) + plain(w(f"transient_encoding.{j}"))])
        d8.append(("delta_g1",) + fold("transient_encoding.0"))
    out["delta8"] = ("h8", d8)
    for l in range(8, 1, -1):
        m = w(f"xyz_encoding_{l}.0")
        out[f"delta{l - 1}"] = (f"h{l - 1}", [(f"delta{l}",) + plain(m[:, cx:] if l == 5 else m)])
    return out


def fp16_spacing(v):
    """Distance between the two fp16 neighbours of a value that is not one itself (subnormal step 2^-24 at the bottom)."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -14)))
    return torch.maximum(2.0 ** (e - 10), torch.full_like(v, U24))


def real_case(R, N, kind, backward, nfx=10, pe_w=None):
    """Training forward -> composite backward -> dgrad on the oracle's `sharp` weights, as test_wgrad_on_real_stashes sets
    them up, and everything decoded.  `pe_w`: (xyz, dir) BARF weights; the ray gradient is then asked for as well."""
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    dev = gpu_util.DEV
    lat = kind == "nerfw"
    BP = rnd._BPREC[backward]
    mult = 2 if backward == "f16x3" else 1
    kw = dict(n_emb_xyz=nfx) if nfx != 10 else {}
    spec = orc.FieldSpec("fine", encode_appearance=True, encode_transient=True, beta_min=0.1, **kw) if lat else orc.FieldSpec("coarse", **kw)
    P = orc.make_field_params(spec, 81 + lat, "sharp")
    model = gpu_util.module_from(spec, P)
    f = rnd._field(model, nfx, 4, torch.device(dev), prec=rnd._PREC["f16x3"])
    rays, z = exact_rays(R, N, 5 * R + N)
    gen = torch.Generator().manual_seed(R + N)
    a_emb = torch.randn(R, 48, generator=gen).to(dev) if lat else None
    t_emb = torch.randn(R, 16, generator=gen).to(dev) if lat else None
    rays_d, z_d = rays.to(dev), z.to(dev)
    pw = {} if pe_w is None else dict(pe_w_xyz=pe_w[0].to(dev), pe_w_dir=pe_w[1].to(dev))
    f.ensure_bwd_packed(pe_w is not None, BP)
    out = rnd._run_pass(f, rays_d, N, z=z_d, noise=None, noise_std=0.0, white_back=True, a_emb=a_emb, t_emb=t_emb,
                        stash=True, bprec=BP, **pw)
    g = {k: (torch.randn(*s, generator=gen) * 1e-2).to(dev) for k, s in
         dict(weights=(R, N), opacity=(R,), rgb=(R, 3), depth=(R,), tsig=(R, N), beta=(R,), rgb_s=(R, 3), rgb_t=(R, 3)).items()}
    up = [g[k] for k in ("weights", "opacity", "rgb", "depth")] + ([g[k] for k in ("tsig", "beta", "rgb_s", "rgb_t")] if lat else [None] * 4)
    head, gmax = rnd._run_compbwd(out["field_raw"], z_d, R, N, noise=None, noise_std=0.0, use_t=lat, white_back=True, grads=up,
                                  go=None, g_tsig_const=0.0)
    torch.cuda.synchronize()
    gmax_value = float(gmax.max())
    assert gmax_value > 0
    lay = sc.Layout(nfx, 4, 48, 16, nkp=sc.nkp_of_plan(f.wgrad_plan(lat)[0]), has_a=lat, has_t=lat)
    g_rays = None
    ray_kw = {}
    if pe_w is not None:
        g_rays = torch.zeros(R, 8, dtype=torch.float32, device=dev)
        ray_kw = dict(g_rays=g_rays, rays=rays_d, z=z_d, **pw)
    hi, lo, g_a, g_t = run_dgrad(f, lay, None, head, gmax_value, R, N, lat, backward, lat, act_stash=out["act_stash"], **ray_kw)
    n_seg = R * ((N + 31) // 32)
    rows = padded_rows(R, N)
    act = out["act_stash"].cpu()
    return dict(lat=lat, mult=mult, rays=rays, z=z, scale=loss_scale(gmax_value), head=head, lay=lay, hi=hi, lo=lo, g_a=g_a, g_t=g_t,
                g_rays=None if g_rays is None else g_rays.cpu(), rows=rows, P64={k: v.double() for k, v in P.items()},
                masks=sc.decode_masks(act[sc.mask_offset(n_seg, lay.nkp, mult):], n_seg, lat),
                ahi=sc.Layout._get(sc.Layout._records(act, n_seg, lay.act_slots, mult)[:, 0], lay.act),
                val=lambda name: (hi[name].double() + (lo[name].double() if lo is not None else 0.0))[rows])


@pytest.mark.parametrize("backward", ARITH)
@pytest.mark.parametrize("kind", ["coarse", "nerfw"])
@pytest.mark.parametrize("R,N", [(3, 40), (9, 64)])
def test_dgrad_on_real_masks_layer_by_layer(R, N, kind, backward):
    """Training forward -> composite backward -> dgrad on the oracle's `sharp` weights; the codec decodes masks and deltas.
    (a) Every live sample's decoded mask agrees with the float64 trunk: a set bit implies a pre-activation > -tol, a clear
        bit one < +tol, tol = rel |pre| + 2e-5 as test_wgrad_on_real_stashes grants h_l; and for every masked layer (dir and
        transient ones included) a stashed activation > 0 has its bit set.
    (b) The heads' records are head * scale: to 2^-21 (hi + lo) in f16x3, otherwise one of its two fp16 neighbours.
    (c) Layer by layer, with the DECODED delta^ of the layer above as the input, so that no error compounds:
            |delta^_{l-1} - mask (.) (W^T delta^_l)| <= mask (.) ((eps_w + K 2^-24) |W|^T |delta^_l| + eps_out |value| + 2^-24)
        and exactly 0 where the mask is clear.  W: the float64 weights (the folded W_dir', W_t0', layer 5's skip columns and
        the three transient heads into g4 included); K: the terms of the fp32 accumulation (the inputs' total width); eps_w,
        eps_out: EPS above, from the formats; 2^-24: the fp16 subnormal step of the stored delta.  The weights' own subnormal
        step enters as W_STEP sum_k |delta^_k| (see W_STEP: without it f16x3's delta_dirh measured 1.57 of the bound at a
        feature whose three static_rgb weights, 0.035, 0.012 and 0.0045, are held to 0.2, 4.2 and 12.7 * 2^-21 by hi + lo).
        The folded matrices add 256 * 2^-24 of |W| |W_fin| (layer_inputs).
    (d) g_a, g_t equal the float64 sums over a ray's live samples of the decoded operands within (N + K) 2^-24 sum|terms|
        plus the weight terms eps_w sum|terms| + W_STEP sum|delta^|.
    Largest |error| / bound over all layers as measured on the MI355X (printed per case and per layer), then the latents':
        R = 3, N = 40:  coarse f16 0.64, f16w 0.95, f16x3 0.51;  nerfw f16 0.71 (0.13), f16w 0.94 (0.026), f16x3 0.53 (0.023)
        R = 9, N = 64:  coarse f16 0.93, f16w 0.98, f16x3 0.54;  nerfw f16 0.79 (0.13), f16w 0.98 (0.018), f16x3 0.52 (0.017)
    f16w sits just below 1 in every layer because its bound is almost only eps_out: a stochastic rounding moves a value by up
    to (not including) one ulp, and an ulp is 2^-10 of a value just above a power of two."""
    c = real_case(R, N, kind, backward)
    lat, mult, masks, rows, val, P64, hi, lo = c["lat"], c["mult"], c["masks"], c["rows"], c["val"], c["P64"], c["hi"], c["lo"]
    rays, z, scale, head, lay, ahi, g_a, g_t = c["rays"], c["z"], c["scale"], c["head"], c["lay"], c["ahi"], c["g_a"], c["g_t"]
    eps_w, eps_out = EPS[backward]
    report, bad = [], []

    # (a) the masks
    xyz = rays[:, None, 0:3].double() + rays[:, None, 3:6].double() * z[..., None].double()
    pe = orc.posenc(xyz.reshape(-1, 3), 10)
    rel = 2.0 ** -20 if mult == 2 else 2.0 ** -10
    h = pe
    for l in range(1, 9):
        x = torch.cat([pe, h], 1) if l == 5 else h
        pre = x @ P64[f"xyz_encoding_{l}.0.weight"].t() + P64[f"xyz_encoding_{l}.0.bias"]
        h = torch.relu(pre)
        tol = rel * pre.abs() + REAL_FWD_ATOL
        m = masks[f"h{l}"][rows]
        wrong = (m & (pre <= -tol)) | (~m & (pre >= tol))
        if wrong.any():
            bad.append(f"mask h{l}: {int(wrong.sum())} bits contradict the float64 trunk, first (sample, feature) {wrong.nonzero()[0].tolist()}")
    for name in masks:
        wrong = (ahi[name][rows] > 0) & ~masks[name][rows]
        if wrong.any():
            bad.append(f"mask {name}: {int(wrong.sum())} stashed activations > 0 have a clear bit")
        assert bool(masks[name][rows].any()) and not bool(masks[name][rows].all())

    # (b) the heads' records
    hd = head.cpu().double() * scale
    for k, cols in enumerate([[3], [0, 1, 2], [7], [4, 5, 6], [8]][:5 if lat else 2]):
        v, got = hd[:, cols], val(f"heads{k}")
        if mult == 2:
            ok = (got - v).abs() <= 2.0 ** -21 * v.abs() + U24
        else:
            ok = ((got - v).abs() < fp16_spacing(v)) | (got == v)
        if not ok.all():
            bad.append(f"heads{k}: {int((~ok).sum())} records are not head * scale, first {(~ok).nonzero()[0].tolist()}")

    # (c) layer by layer
    worst_c = 0.0
    for name, (mask_name, ins) in layer_inputs(P64, lay.cx, lat).items():
        K = sum(m.shape[0] for _, m, _, _ in ins)
        pred = sum(val(src) @ m for src, m, _, _ in ins)
        bound = sum((eps_w + K * U24 + extra) * (val(src).abs() @ am) + W_STEP[backward] * val(src).abs().sum(1, keepdim=True)
                    for src, _, am, extra in ins) + eps_out * pred.abs() + U24
        mk = masks[mask_name][rows]
        got = val(name)
        if got[~mk].any():
            bad.append(f"{name}: non-zero where the relu mask is clear")
        assert bool(got[mk].any()), name
        ratio = torch.where(mk, (got - pred).abs() / bound, torch.zeros_like(pred))
        k = int(ratio.argmax())
        report.append(f"{name} {float(ratio.max()):.3f}")
        worst_c = max(worst_c, float(ratio.max()))
        if not float(ratio.max()) <= 1.0:
            bad.append(f"{name}: |delta^ - mask W^T delta^| reaches {float(ratio.max()):.3f} of its bound at ray {k // pred.shape[1] // N} "
                       f"sample {k // pred.shape[1] % N} feature {k % pred.shape[1]} (tile {k % pred.shape[1] // 32})")

    # (d) the latent gradients
    worst_d = 0.0
    if lat:
        cd = lay.cd
        for got, src, m in ((g_a, "delta_dirh", P64["dir_encoding.0.weight"][:, W + cd:W + cd + 48]),
                            (g_t, "delta_g1", P64["transient_encoding.0.weight"][:, W:W + 16])):
            exp = (val(src) @ m).view(R, N, -1).sum(1) / scale
            mag = (val(src).abs() @ m.abs()).view(R, N, -1).sum(1) / scale
            step = W_STEP[backward] * val(src).abs().sum(1, keepdim=True).view(R, N, 1).sum(1) / scale
            ratio = (got.double() - exp).abs() / (((N + m.shape[0]) * U24 + eps_w) * mag + step)
            worst_d = max(worst_d, float(ratio.max()))
            assert float(exp.abs().max()) > 0
            if not float(ratio.max()) <= 1.0:
                bad.append(f"latent gradient from {src}: {float(ratio.max()):.3f} of its bound")
    print(f"real masks R={R} N={N} {kind} {backward}: loss scale 2^{int(torch.log2(torch.tensor(scale)))}, layer-local worst {worst_c:.3f} "
          f"({', '.join(report)}); latent worst {worst_d:.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("nfx,kind,backward", [(10, "nerfw", "f16"), (15, "coarse", "f16x3")])
def test_dgrad_ray_gradients(nfx, kind, backward):
    """(e) d/d rays with BARF weights != 1, for both encoder instantiations: g_rays against the float64 chain through the
    position and direction encodings (autograd through the oracle's posenc) of the DECODED delta1, delta5 and delta_dirh.  The
    kernel's sine is not derivable, so the thresholds are the ones tests/test_grad_gpu.py holds `grad.rays` to in that
    arithmetic: its `max` (of the largest element) and `elem` (relative, elements >= 0.1 max) measures.  Measured on the
    MI355X: 10 frequencies, nerfw, f16: max 2.4e-4, elem 5.8e-4 (limits 8e-3, 4.5e-2); 15 frequencies, coarse, f16x3: max 5.1e-7,
    elem 1.1e-6 (limits 1.5e-3, 1e-2)."""
    import test_grad_gpu as tg
    R, N = 3, 40
    pe_w = (torch.linspace(1.0, 0.25, nfx), torch.linspace(0.9, 0.3, 4))
    c = real_case(R, N, kind, backward, nfx=nfx, pe_w=pe_w)
    val, P64, lay = c["val"], c["P64"], c["lay"]
    cx, cd = lay.cx, lay.cd
    G_pe = val("delta1") @ P64["xyz_encoding_1.0.weight"] + val("delta5") @ P64["xyz_encoding_5.0.weight"][:, :cx]
    G_dir = val("delta_dirh") @ P64["dir_encoding.0.weight"][:, W:W + cd]
    o = c["rays"][:, 0:3].double().requires_grad_(True)
    d = c["rays"][:, 3:6].double().requires_grad_(True)
    xyz = o[:, None, :] + d[:, None, :] * c["z"][..., None].double()
    loss = (orc.posenc(xyz.reshape(-1, 3), nfx, pe_w[0]) * G_pe).sum()
    loss = loss + (orc.posenc(d, 4, pe_w[1]).repeat_interleave(N, 0) * G_dir).sum()
    loss.backward()
    exp = torch.cat([o.grad, d.grad], 1) / c["scale"]
    got = c["g_rays"].double()
    assert not got[:, 6:].any() and float(exp.abs().max()) > 0
    table = {"f16": tg.THRESH, "f16w": tg.THRESH_F16W, "f16x3": tg.THRESH_X3}[backward]
    worst_max = float((got[:, :6] - exp).abs().max() / exp.abs().max())
    worst_elem = tg._elem_rel(got[:, :6], exp)
    print(f"ray gradients nfx={nfx} {kind} {backward}: max {worst_max:.3e} (limit {tg._limit('max', 'grad.rays', table)}), "
          f"elem {worst_elem:.3e} (limit {tg._limit('elem', 'grad.rays', table)})")
    assert worst_max <= tg._limit("max", "grad.rays", table) and worst_elem <= tg._limit("elem", "grad.rays", table)
