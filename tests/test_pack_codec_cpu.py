"""tests/pack_codec.py on the CPU: every weight has exactly one place in a stream, the tile order written down from
nfl_plan.h is the one the library's plan builders emit, and nfl_pack_fields refuses on the host what it must.  No kernel is
launched; tests/test_pack_gpu.py compares the pack kernel's bytes with the codec, so a mistake in the codec fails here."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_codec as pc
from pack_codec import F16, F16W, F16X3, WIDTHS

KINDS = list(pc.KINDS)                  # with WIDTHS: the layouts tests/test_pack_gpu.py runs


def occurrences(idx, shapes):
    """layer -> (out, in) int tensor: how often each weight element is named by the index tensor."""
    flat = idx.reshape(-1, 3).long()
    flat = flat[flat[:, 0] != pc.PAD]
    out = {}
    for l, (o, i) in shapes.items():
        e = flat[flat[:, 0] == l]
        assert e.numel() == 0 or (int(e[:, 1].max()) < o and int(e[:, 2].max()) < i and int(e[:, 1:].min()) >= 0), l
        out[l] = torch.bincount(e[:, 1] * i + e[:, 2], minlength=o * i).view(o, i)
    assert set(flat[:, 0].unique().tolist()) <= set(shapes)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("widths", WIDTHS)
def test_every_weight_has_exactly_one_place(widths, kind):
    has_a, has_t = pc.KINDS[kind]
    shapes = pc.layer_shapes(widths, has_a, has_t)
    cx, cd = 6 * widths[0] + 3, 6 * widths[1] + 3
    for name, tiles in (("forward", pc.forward_tiles(widths, has_a, has_t)), ("dgrad+rays", pc.dgrad_tiles(widths, has_a, has_t, True)),
                        ("dgrad", pc.dgrad_tiles(widths, has_a, has_t, False))):
        idx, bidx, tile = pc.index(tiles)
        occ = occurrences(idx, shapes)
        expect = {l: torch.ones(s, dtype=torch.long) for l, s in shapes.items()}
        expect[pc.P_FINAL].zero_()                                   # xyz_encoding_final has no tiles
        if name == "dgrad":                                          # without the ray gradient nothing reads these
            expect[pc.P_XYZ1].zero_()
            expect[pc.P_XYZ1 + 4][:, :cx] = 0
            expect[pc.P_DIR][:, pc.W:pc.W + cd] = 0
        for l in shapes:
            assert torch.equal(occ[l], expect[l]), (name, l)
        # every other position is padding: named positions = weights named
        assert int((idx[..., 0] != pc.PAD).sum()) == sum(int(e.sum()) for e in expect.values()), name
        assert idx.shape[0] == tile.numel() == pc.frag_offsets(tiles)[1]
        # bias table: a forward stream names every bias (except xyz_encoding_final's) once, a dgrad stream none
        named = bidx[bidx[..., 0] != pc.PAD].long()
        if name == "forward":
            want = sorted((l, r) for l, (o, _) in shapes.items() if l != pc.P_FINAL for r in range(o))
            assert sorted(map(tuple, named.tolist())) == want
            assert named.shape[0] == sum(o for l, (o, _) in shapes.items() if l != pc.P_FINAL)
        else:
            assert named.numel() == 0


def test_plan_record_size():
    from nerf_fl_amd import _lib
    assert pc.PLAN_DTYPE.fields["beta_min"][1] == 24 * 4 and pc.PLAN_DTYPE.fields["rt"][1] == pc.PLAN_HEADER_INTS * 4
    assert pc.TILE_DTYPE.itemsize == 96 and pc.BLK_DTYPE.itemsize == 8 and pc.SEG_DTYPE.itemsize == 16
    assert pc.PLAN_DTYPE.itemsize == pc.PLAN_HEADER_INTS * 4 + 112 * 96
    d = pc.desc_of(WIDTHS[0], "nerfw")
    assert _lib.lib().nfl_plan_bytes(C.byref(d)) == pc.PLAN_DTYPE.itemsize


def check_plan(plan, tiles, widths, kind, split, what):
    has_a, has_t = pc.KINDS[kind]
    off, total = pc.frag_offsets(tiles)
    assert int(plan["magic"]) == pc.PLAN_MAGIC and int(plan["elem"]) == 0, what
    assert int(plan["n_rt"]) == len(tiles), (what, int(plan["n_rt"]), len(tiles))
    got = pc.plan_tiles(plan)
    for n, (g, e) in enumerate(zip(got, tiles)):
        assert g == e, (what, "tile", n, g, e)
        rt = plan["rt"][n]
        assert int(rt["frag_off"]) == off[n] and int(rt["nks"]) == sum(s[0] for s in e[4]), (what, "tile", n)
        assert int(rt["nblk"]) == len(e[3]) and int(rt["nseg"]) == len(e[4]), (what, "tile", n)
    assert int(plan["total_ks"]) == total, what
    assert int(plan["ks_bytes"]) == (2048 if split else 1024) and int(plan["nsplit"]) == (3 if split else 1), what
    assert int(plan["stream_bytes"]) == int(plan["bias_off"]) == total * int(plan["ks_bytes"]), what
    assert int(plan["packed_bytes"]) == int(plan["bias_off"]) + len(tiles) * 128, what
    assert int(plan["nkp"]) == pc.nkp_for(widths[0]), what
    for l, (_, n_in) in pc.layer_shapes(widths, has_a, has_t).items():        # row stride of every layer the field has
        assert int(plan["ld"][l]) == n_in, (what, "ld", l)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("widths", WIDTHS)
def test_codec_order_is_the_built_plans(widths, kind):
    from nerf_fl_amd import _lib
    L = _lib.lib()
    has_a, has_t = pc.KINDS[kind]
    d = pc.desc_of(widths, kind)
    for prec in (F16, F16X3):
        _, plan = pc.build_plan(widths, kind, prec)
        check_plan(plan, pc.forward_tiles(widths, has_a, has_t), widths, kind, prec == F16X3, ("forward", prec))
        assert int(plan["is_bwd"]) == 0 and int(plan["prec"]) == prec
        assert L.nfl_packed_bytes(C.byref(d), prec) == int(plan["packed_bytes"])
    for rays_grad in (0, 1):
        for prec in (F16, F16W, F16X3):
            _, plan = pc.build_plan(widths, kind, prec, rays_grad)
            check_plan(plan, pc.dgrad_tiles(widths, has_a, has_t, bool(rays_grad)), widths, kind, prec != F16, ("dgrad", rays_grad, prec))
            assert int(plan["is_bwd"]) == 1 and int(plan["prec"]) == prec
            assert int(plan["reserved_flags"]) == (rays_grad | widths[1] << 8)
            assert L.nfl_bwd_packed_bytes(C.byref(d), rays_grad, prec) == int(plan["packed_bytes"])


def test_pack_refuses_on_the_host():
    """NFL_ESMALL for a valid plan and a destination one byte short, NFL_EINVAL for a plan whose magic is wrong: both before
    any launch.  Without a device the device pointers are made up: they are never dereferenced only because nfl_pack_fields
    validates every job of a batch before its single launch.  Where the suite runs on a GPU the same calls get real buffers
    (device copies of the plans, a destination of the full size, zero parameters of the largest layer's size), so that a
    regression of that order fails these assertions instead of launching the kernel on pointers that point nowhere."""
    from nerf_fl_amd import _lib
    L = _lib.lib()
    h, plan = pc.build_plan(WIDTHS[0], "nerfw", F16X3)
    h2, plan2 = pc.build_plan(WIDTHS[0], "coarse", F16, 0)
    nbytes, nbytes2 = int(plan["packed_bytes"]), int(plan2["packed_bytes"])
    fp = _lib.FieldParams()
    d_plan = d_plan2 = d_out = 4096
    if torch.cuda.is_available():
        keep = [torch.frombuffer(bytearray(x.raw), dtype=torch.uint8).cuda() for x in (h, h2)]
        keep += [torch.empty(max(nbytes, nbytes2), dtype=torch.uint8, device="cuda"), torch.zeros(256 * 352, device="cuda")]
        d_plan, d_plan2, d_out, zeros = (t.data_ptr() for t in keep)
        for i in range(len(fp.weight)):               # every layer is at most 256 x 349
            fp.weight[i] = fp.bias[i] = zeros

    def job(n):
        return _lib.PackJob(C.cast(h, C.c_void_p), d_plan, C.pointer(fp), d_out, n, None)

    assert L.nfl_pack_fields(1, (_lib.PackJob * 1)(job(nbytes - 1)), None) == -4
    assert L.nfl_pack_field(h, d_plan, C.byref(fp), d_out, nbytes - 1, None, None) == -4
    # in a batch too, whichever job it is
    ok = _lib.PackJob(C.cast(h2, C.c_void_p), d_plan2, C.pointer(fp), d_out, nbytes2, None)
    assert L.nfl_pack_fields(2, (_lib.PackJob * 2)(ok, job(nbytes - 1)), None) == -4
    np.frombuffer(h, dtype=np.uint32, count=1)[0] ^= 1               # the magic, in the host plan the validation reads
    assert L.nfl_pack_fields(1, (_lib.PackJob * 1)(job(nbytes)), None) == -1
    assert L.nfl_pack_fields(2, (_lib.PackJob * 2)(ok, job(nbytes)), None) == -1
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def test_slot_maps():
    """The two k-slot maps spelled out on a few positions (nfl_plan.h), and as permutations of a segment's columns."""
    act = pc.slot_columns(pc.ACT, 4)
    assert act[0, 0].tolist() == [0, 1, 2, 3, 8, 9, 10, 11] and act[0, 32].tolist() == [4, 5, 6, 7, 12, 13, 14, 15]
    assert act[1, 0, 0] == 16 and act[2, 0, 0] == 32 and act[3, 63, 7] == 63
    assert torch.equal(act[:, 0], act[:, 31]) and torch.equal(act[:, 32], act[:, 63])
    nat = pc.slot_columns(pc.NAT, 2)
    assert nat[0, 0].tolist() == list(range(8)) and nat[1, 32].tolist() == list(range(24, 32))
    for kind in (pc.ACT, pc.NAT):
        m = pc.slot_columns(kind, 4)
        assert sorted(torch.cat([m[:, 0], m[:, 32]], 1).flatten().tolist()) == list(range(64))


def test_encode_places_single_weights():
    """One non-zero weight at a time: the byte offset the documentation gives, computed here by hand."""
    widths, kind = (10, 4, 48, 16), "nerfw"
    shapes = pc.layer_shapes(widths, True, True)
    zero = lambda: {l: (torch.zeros(s), torch.zeros(s[0])) for l, s in shapes.items()}
    fwd, bwd = pc.forward_tiles(widths, True, True), pc.dgrad_tiles(widths, True, True, False)
    # forward, L2 (tiles 8..15, 16 k-steps each, behind L1's 8 x 4): W[40][21] -> tile 9 row 8; column 21 = 16 + 4 h + (j & 3):
    # k-step 1, h 1, j 1 -> lane 40
    P = zero()
    P[1][0][40, 21] = 1.5
    P[1][1][40] = -2.0
    hi, lo, bias, _ = pc.encode(fwd, P, True)
    at = (32 + 16 + 1) * 512 + 40 * 8 + 1
    assert hi.view(torch.float16).flatten().nonzero().flatten().tolist() == [at] and float(hi.view(torch.float16).flatten()[at]) == 1.5
    assert not lo.any() and bias.flatten().nonzero().flatten().tolist() == [9 * 32 + 8] and float(bias[9, 8]) == -2.0
    # the three-block head tile: beta's bias in row 8, rgb_t's in rows 1..3, sigma_t's in row 0 of the last tile
    P = zero()
    P[pc.P_TBETA][1][0], P[pc.P_TSIGMA][1][0] = 3.0, 4.0
    P[pc.P_TRGB][1][:] = torch.tensor([5.0, 6.0, 7.0])
    bias = pc.encode(fwd, P, False)[2]
    assert bias[-1, :9].tolist() == [4.0, 5.0, 6.0, 7.0, 0, 0, 0, 0, 3.0] and int((bias != 0).sum()) == 5
    # dgrad, first tile (heads into g4): beta's weight of input column 5 is k-step 2 (third segment), k-slot 0 of row 5
    P = zero()
    P[pc.P_TBETA][0][0, 5] = 0.25
    hi = pc.encode(bwd, P, False)[0].view(torch.float16).flatten()
    assert hi.nonzero().flatten().tolist() == [2 * 512 + 5 * 8 + 0]
    # lo image of a weight fp16 cannot hold
    P = zero()
    P[0][0][0, 0] = 1.0 + 2.0 ** -12
    hi, lo, _, _ = pc.encode(fwd, P, True)
    assert float(hi.view(torch.float16).flatten()[0]) == 1.0 and float(lo.view(torch.float16).flatten()[0]) == 2.0 ** -12
    buf = pc.assemble(hi, lo, torch.zeros(len(fwd), 32))
    assert buf.numel() == hi.numel() * 2 + len(fwd) * 128 and buf[:2].tolist() == [0x00, 0x3C] and buf[1024:1026].tolist() == [0x00, 0x0C]


def test_torch_rounds_like_numpy():
    """The codec's rounding is torch's fp32 -> fp16 conversion; held to numpy's, hi and lo, on bit patterns that include
    fp16-subnormal magnitudes, ties between fp16 neighbours, fp32 denormals, +-0 and +-65504."""
    rng = np.random.default_rng(5)
    h = rng.integers(0, 0x7BFF, 1 << 16, dtype=np.int64)                       # fp16 patterns below the largest
    lo16, hi16 = h.astype(np.uint16).view(np.float16).astype(np.float32), (h + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    ties = (lo16 + hi16) / 2                                                   # exact in fp32
    bits = rng.integers(0, 1 << 32, 1 << 17, dtype=np.uint64).astype(np.uint32)
    bits = (bits & np.uint32(0x807FFFFF)) | (rng.integers(127 - 30, 127 + 16, bits.size).astype(np.uint32) << np.uint32(23))
    w = np.concatenate([bits.view(np.float32), ties, -ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1e9)),
                        rng.integers(1, 1 << 23, 4096).astype(np.uint32).view(np.float32),
                        np.array([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25], np.float32)])
    w = w[np.abs(w) <= 65504]
    n_hi = w.astype(np.float16)
    n_lo = (w - n_hi.astype(np.float32)).astype(np.float16)
    t_hi, t_lo = pc.round_hi_lo(torch.from_numpy(w))
    assert np.array_equal(t_hi.numpy().view(np.uint16), n_hi.view(np.uint16))
    assert np.array_equal(t_lo.numpy().view(np.uint16), n_lo.view(np.uint16))
    assert w.size > 3e5 and int((np.abs(w) < 2.0 ** -14).sum()) > 5e4


def test_fp16_neighbours():
    """pack_codec.fp16_neighbours: the neighbour toward zero, the discarded fraction and the ulp, against fp16 arithmetic."""
    g = torch.Generator().manual_seed(9)
    w = torch.randn(1 << 16, generator=g) * 10.0 ** torch.randint(-8, 3, (1 << 16,), generator=g)
    w = torch.cat([w, torch.tensor([0.0, -0.0, 1.0, -65504.0, 2.0 ** -24, 2.0 ** -25, -3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -30, 1e-42])])
    toward, f, ulp = pc.fp16_neighbours(w)
    t = toward.view(torch.float16).double()
    a = w.double().abs()
    assert bool((t.abs() <= a).all()) and bool((a - t.abs() < ulp).all()) and bool(((0 <= f) & (f < 1)).all())
    assert torch.equal(t.abs() + f * ulp, a)                                   # exact in float64
    assert torch.equal(torch.signbit(t), torch.signbit(w))
    nxt = (toward + 1).view(torch.float16).double()                            # the next pattern is the neighbour away from zero
    below_max = t.abs() < 65504
    assert torch.equal(nxt.abs()[below_max], (t.abs() + ulp)[below_max]) and int((~below_max).sum()) == 1
    rn = w.half().view(torch.int16)
    assert bool(((rn == toward) | (rn == toward + 1)).all()) and bool((rn[f == 0] == toward[f == 0]).all())
    assert bool((ulp[a < 2.0 ** -14] == 2.0 ** -24).all()) and float(ulp[w == 1.0][0]) == 2.0 ** -10
