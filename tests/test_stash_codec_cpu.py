"""tests/stash_codec.py on the CPU: encode and decode are inverses, and a record's named bytes are written exactly once."""
import ctypes as C

import pytest
import torch

import stash_codec as sc

# (n_emb_xyz, n_emb_dir, n_a, n_tau): the width sets of tests/test_wgrad_gpu.py
WIDTHS = [(10, 4, 48, 16), (12, 4, 40, 5), (3, 1, 48, 16), (15, 4, 1, 1)]


def plan_nkp(widths, latents):
    """nkp as the tests take it: from a weight-gradient plan the library's host planner builds for the field."""
    from nerf_fl_amd import _lib
    L = _lib.lib()
    desc = _lib.FieldDesc(n_emb_xyz=widths[0], n_emb_dir=widths[1], encode_appearance=int(latents), n_a=widths[2],
                          encode_transient=int(latents), n_tau=widths[3], beta_min=0.03, reserved=0)
    n = L.nfl_wgrad_plan_bytes()
    h = C.create_string_buffer(n)
    _lib.check(L.nfl_wgrad_plan_build(C.byref(desc), int(latents), h, n), "nfl_wgrad_plan_build")
    return sc.nkp_of_plan(h)


def random_fields(layout, n_seg, gen):
    # fp16-exact values, all distinct enough that a misplaced element shows
    return {n: (torch.randint(-2048, 2049, (n_seg * 32, w), generator=gen).to(torch.float16) / 64)
            for n, w in layout.widths().items()}


@pytest.mark.parametrize("latents", [False, True])
@pytest.mark.parametrize("widths", WIDTHS)
def test_nkp_from_plan(widths, latents):
    assert plan_nkp(widths, latents) == (4 if widths[0] <= 10 else 6)


@pytest.mark.parametrize("mult", [1, 2])
@pytest.mark.parametrize("latents", [False, True])
@pytest.mark.parametrize("widths", WIDTHS)
def test_encode_decode_roundtrip(widths, latents, mult):
    lay = sc.Layout(*widths, nkp=plan_nkp(widths, latents), has_a=latents, has_t=latents)
    gen = torch.Generator().manual_seed(7)
    n_seg = 3
    hi = random_fields(lay, n_seg, gen)
    lo = random_fields(lay, n_seg, gen) if mult == 2 else None
    act, grd = lay.encode(hi, lo, fill=-7.0)
    assert act.dtype == torch.uint8 and act.numel() == n_seg * mult * lay.act_slots * 1024
    assert grd.numel() == n_seg * mult * lay.grd_slots * 1024
    dhi, dlo = lay.decode(act, grd, n_seg, mult)
    assert set(dhi) == set(hi)
    for n in hi:
        assert torch.equal(dhi[n], hi[n]), n
        if mult == 2:
            assert torch.equal(dlo[n], lo[n]), n
    # and the other way round: decode followed by encode reproduces the named bytes and leaves the rest at the fill value
    act2, grd2 = lay.encode(dhi, dlo, fill=-7.0)
    assert torch.equal(act2, act) and torch.equal(grd2, grd)
    # a longer buffer (tail pad, relu masks) decodes the same
    dhi3, _ = lay.decode(torch.cat([act, torch.zeros(4096, dtype=torch.uint8)]), grd, n_seg, mult)
    assert all(torch.equal(dhi3[n], hi[n]) for n in lay.act)


@pytest.mark.parametrize("latents", [False, True])
@pytest.mark.parametrize("widths", WIDTHS)
def test_named_bytes_written_exactly_once(widths, latents):
    lay = sc.Layout(*widths, nkp=plan_nkp(widths, latents), has_a=latents, has_t=latents)
    for count, fields, slots in zip(lay.coverage(), (lay.act, lay.grd), (lay.act_slots, lay.grd_slots)):
        assert count.shape == (slots, 32, 16)
        assert int(count.max()) == 1                                    # no two fields (or pieces) share a position
        assert int(count.sum()) == 32 * sum(p[4] for ps in fields.values() for p in ps)      # every named value has one
    # what encode leaves at the fill value is exactly what the map does not name
    n_seg = 2
    ones = {n: torch.ones(n_seg * 32, w) for n, w in lay.widths().items()}
    for buf, count in zip(lay.encode(ones, fill=-7.0), lay.coverage()):
        v = buf.view(torch.float16).view(n_seg, *count.shape)
        for s in range(n_seg):
            assert torch.equal(v[s] == 1.0, count == 1) and torch.equal(v[s] == -7.0, count == 0)


def random_masks(has_t, n_seg, gen):
    return {n: torch.randint(0, 2, (n_seg * 32, 32 * tiles), generator=gen).bool() for n, (_, tiles) in sc.mask_fields(has_t).items()}


@pytest.mark.parametrize("has_t", [False, True])
def test_mask_roundtrip(has_t):
    gen = torch.Generator().manual_seed(11)
    n_seg = 3
    masks = random_masks(has_t, n_seg, gen)
    buf = sc.encode_masks(masks, has_t)
    assert buf.dtype == torch.uint8 and buf.numel() == n_seg * sc.MSK_WORDS * 256
    back = sc.decode_masks(buf, n_seg, has_t)
    assert set(back) == set(masks) and all(torch.equal(back[n], masks[n]) for n in masks)
    assert torch.equal(sc.encode_masks(back, has_t), buf)
    # a longer buffer decodes the same, and without the transient head its words stay zero
    assert all(torch.equal(v, masks[n]) for n, v in sc.decode_masks(torch.cat([buf, buf[:512]]), n_seg, has_t).items())
    if not has_t:
        assert not sc.decode_masks(buf, n_seg, True)["g3"].any()


def test_mask_words_owned_exactly_once():
    """Every one of the 84 * 64 words of a record belongs to exactly one (field, tile, lane); of its 32 bits the 16 the bit
    rule names carry one feature each, the other 16 none."""
    count = torch.zeros(sc.MSK_WORDS, 64, 32, dtype=torch.int32)
    masks = {n: torch.ones(32, 32 * tiles, dtype=torch.bool) for n, (_, tiles) in sc.mask_fields(True).items()}
    buf = sc.encode_masks(masks, True, count)
    assert int(count.max()) == 1
    named = [2 * p for p in range(8)] + [16 + 2 * p for p in range(8)]
    assert torch.equal(count.sum(-1), torch.full((sc.MSK_WORDS, 64), 16, dtype=torch.int32))
    assert int(count[:, :, named].sum()) == int(count.sum()) == sc.MSK_WORDS * 64 * 16 == 32 * sum(32 * t for _, t in sc.mask_fields(True).values())
    words = buf.view(torch.int32)
    assert words.numel() == sc.MSK_WORDS * 64 and bool((words == sum(1 << b for b in named)).all())
    # the words of two fields never meet, and together they are 0 .. 83
    owner = sorted(w0 + t for w0, tiles in sc.mask_fields(True).values() for t in range(tiles))
    assert owner == list(range(sc.MSK_WORDS))


def test_mask_bit_and_word_placement():
    """One set bit at a time, against the rules of nfl_plan.h spelled out here: word w of a segment lies at byte
    (w >> 2) * 1024 + lane * 16 + (w & 3) * 4 of its 84 * 256-byte record, lane = 32 * half + sample, and the feature in row
    (r & 3) + 8 (r >> 2) + 4 half of tile t is bit r (r even) or 16 + r - 1 (r odd)."""
    n_seg = 2
    for name, seg, sample, feature in [("h1", 0, 0, 0), ("h3", 1, 31, 255), ("h8", 1, 7, 100), ("dirh", 0, 5, 37), ("g1", 1, 9, 4),
                                       ("g4", 0, 30, 127), ("h5", 0, 17, 45)]:
        masks = {n: torch.zeros(n_seg * 32, 32 * tiles, dtype=torch.bool) for n, (_, tiles) in sc.mask_fields(True).items()}
        masks[name][seg * 32 + sample, feature] = True
        words = sc.encode_masks(masks, True).view(torch.int32)
        tile, row = feature // 32, feature % 32
        half = (row // 4) % 2
        r = (row % 4) + 4 * (row // 8)
        assert (r & 3) + 8 * (r >> 2) + 4 * half == row
        w = (64 if name == "dirh" else 68 + 4 * (int(name[1]) - 1) if name[0] == "g" else 8 * (int(name[1]) - 1)) + tile
        at = (seg * sc.MSK_WORDS * 256 + (w >> 2) * 1024 + (32 * half + sample) * 16 + (w & 3) * 4) // 4
        bit = r if r % 2 == 0 else 16 + r - 1
        nz = words.nonzero().flatten().tolist()
        assert nz == [at] and int(words[at]) == 1 << bit, (name, nz, at, int(words[at]), bit)


@pytest.mark.parametrize("mult", [1, 2])
@pytest.mark.parametrize("widths", WIDTHS)
def test_mask_offset_is_the_librarys(widths, mult):
    """nfl_msk_offset through the one exported function built on it: nfl_act_stash_bytes = nfl_msk_offset + n_seg * 84 * 256."""
    from nerf_fl_amd import _lib
    L = _lib.lib()
    desc = _lib.FieldDesc(n_emb_xyz=widths[0], n_emb_dir=widths[1], encode_appearance=1, n_a=widths[2], encode_transient=1,
                          n_tau=widths[3], beta_min=0.03, reserved=0)
    prec = _lib.NFL_PREC_F16X3 if mult == 2 else _lib.NFL_PREC_F16
    for n_rays, n_samples in [(1, 1), (9, 40), (3, 300)]:
        n_seg = n_rays * ((n_samples + 31) // 32)
        total = L.nfl_act_stash_bytes(C.byref(desc), n_rays, n_samples, prec)
        assert total - n_seg * sc.MSK_WORDS * 256 == sc.mask_offset(n_seg, plan_nkp(widths, True), mult)


def test_feature_orders():
    """The two k-slot -> column maps of nfl_plan.h, spelled out on a few positions."""
    act = sc.feature_of_position(sc.ACT, 64)
    # k-step 0, half 0, values 0..7 -> columns 0..3, 8..11; half 1 -> 4..7, 12..15; k-step 1 starts at column 16
    assert act[:8].tolist() == [0, 1, 2, 3, 8, 9, 10, 11]
    assert act[8:16].tolist() == [4, 5, 6, 7, 12, 13, 14, 15]
    assert act[16] == 16 and act[32] == 32 and act[63] == 63
    assert sorted(act.tolist()) == list(range(64))
    assert sc.feature_of_position(sc.NAT, 32).tolist() == list(range(32))


def test_reference_grads_matches_autograd():
    """The operand -> gradient map against autograd on the model itself (float64, a few samples): deltas are autograd's
    gradients of the pre-activations, the map must rebuild every parameter gradient from them and the activations."""
    from oracle import nerfw_oracle as orc
    torch.manual_seed(3)
    spec = orc.FieldSpec("fine", n_emb_xyz=3, n_emb_dir=1, encode_appearance=True, n_a=5, encode_transient=True, n_tau=4)
    P = {k: v.double().requires_grad_(True) for k, v in orc.make_field_params(spec, 5).items()}
    lay = sc.Layout(3, 1, 5, 4, nkp=4)
    n = 32
    pe, side, tau = torch.randn(n, lay.cx).double(), torch.randn(n, lay.cd + 5).double(), torch.randn(n, 4).double()
    acts, pre = {"pe": pe, "dir_side": side, "tau": tau}, {}

    def lin(name, x, key):
        y = torch.nn.functional.linear(x, P[name + ".weight"], P[name + ".bias"])
        y.retain_grad()
        pre[key] = y
        return y

    h = pe
    for l in range(1, 9):
        h = torch.relu(lin(f"xyz_encoding_{l}.0", torch.cat([pe, h], 1) if l == 5 else h, f"delta{l}"))
        acts[f"h{l}"] = h
    sigma = lin("static_sigma.0", h, "heads0")
    feat = torch.nn.functional.linear(h, P["xyz_encoding_final.weight"], P["xyz_encoding_final.bias"])
    acts["dirh"] = torch.relu(lin("dir_encoding.0", torch.cat([feat, side], 1), "delta_dirh"))
    outs = [sigma, lin("static_rgb.0", acts["dirh"], "heads1")]
    g = torch.cat([feat, tau], 1)
    for m, j in enumerate((0, 2, 4, 6)):
        g = torch.relu(lin(f"transient_encoding.{j}", g, f"delta_g{m + 1}"))
        acts[f"g{m + 1}"] = g
    outs += [lin("transient_sigma.0", g, "heads2"), lin("transient_rgb.0", g, "heads3"), lin("transient_beta.0", g, "heads4")]
    sum((o * torch.randn_like(o)).sum() for o in outs).backward()
    hi = {k: v.detach() for k, v in acts.items()}
    hi.update({k: v.grad for k, v in pre.items()})
    ref = sc.reference_grads(lay, hi, None, P, True)
    for name, p in P.items():
        assert torch.allclose(ref[name], p.grad, rtol=1e-10, atol=1e-12), name
