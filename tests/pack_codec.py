"""The packed weight streams as ordinary tensors: which weight every fp16 position of a stream holds, and its bytes.

A plain helper for the packer's tests (no pytest hooks).  Everything here is written from the documentation of the
format in csrc/nfl_plan.h, not from the plan builder (csrc/nfl_plan.cpp) or the pack kernel (csrc/nfl_pack.hip):

* the forward stream's tile order ("Stream order" at the head of the header) and the dgrad stream's ("Dgrad stream
  order", the comment block behind it), with nfl_nkp_for for the position encoding's k-steps;
* the two k-slot -> column maps, NFL_SEG_ACT and NFL_SEG_NAT;
* the k-step image: 1 KiB = 64 lanes x 8 fp16, lane l holds tile row l & 31 and k-slots 8 (l >> 5) + j; in a hi + lo
  stream a k-step is 2 KiB, the hi image and the lo image 1024 bytes behind it (NflPlan.ks_bytes);
* the element rules of NflRowTile (forward: element(i, m) = W[blk.layer][blk.src_row0 + i - blk.dst_row][seg.col0 + m];
  transposed: W[seg.layer][seg.col0 + m][tcol0 + i] for i < tncols) and the bias table [n_rt][32] fp32 behind the stream
  (a forward tile's rows carry their layer's biases, every other row is 0).

test_pack_codec_cpu.py checks, without a GPU, that the order written down here is the one the library's plan builders
emit; test_pack_gpu.py then compares the kernel's bytes with `encode`.

A tile is a tuple (trans, tcol0, tncols, blocks, segs): blocks = ((layer, nrows, src_row0, dst_row), ...) and
segs = ((nks, kind, col0, ncols, layer), ...); `layer` is an NFL_P_* index, -1 in the segments of a forward tile (whose
blocks name the layers).  `widths` = (n_emb_xyz, n_emb_dir, n_a, n_tau).  `params` = {NFL_P_* index: (weight, bias)} fp32
CPU tensors, exactly what the packer is handed: the codec does not fold xyz_encoding_final into dir_encoding.0 /
transient_encoding.0, those two are whatever matrices the caller passes.
"""
import ctypes as C
import functools

import numpy as np
import torch

ACT, NAT = 0, 1                        # NFL_SEG_ACT, NFL_SEG_NAT
W, H = 256, 128
# NFL_P_*
P_XYZ1, P_FINAL, P_DIR, P_SIGMA, P_RGB, P_T0, P_TSIGMA, P_TRGB, P_TBETA = 0, 8, 9, 10, 11, 12, 16, 17, 18
PAD = -1                               # `layer` of a position no weight lands on
F16X3, F16, F16W = 0, 1, 2             # NFL_PREC_*

# The layouts both test files run, so that the CPU check of the codec's order covers what the GPU tests rely on.
# (n_emb_xyz, n_emb_dir, n_a, n_tau): the wide instantiation; a second appearance tile that is empty (and n_tau 1); a partial
# one; n_a exactly 32 with a narrow encoder whose second position tile is empty
WIDTHS = [(10, 4, 48, 16), (15, 4, 1, 1), (12, 4, 40, 5), (3, 1, 32, 16)]
KINDS = {"coarse": (False, False), "nerfw": (True, True)}                  # kind -> (has_a, has_t)


def nkp_for(n_emb_xyz):
    """nfl_nkp_for: position-encoding k-steps of the kernel instantiation (10 or 15 frequencies) that runs the field."""
    return (6 * (10 if n_emb_xyz <= 10 else 15) + 3 + 15) // 16


def layer_shapes(widths, has_a, has_t):
    """NFL_P_* index -> (out_features, in_features) of every layer the field has (xyz_encoding_final included)."""
    nx, nd, n_a, n_tau = widths
    cx, cd = 6 * nx + 3, 6 * nd + 3
    s = {P_XYZ1 + i: (W, cx if i == 0 else W + cx if i == 4 else W) for i in range(8)}
    s[P_FINAL], s[P_DIR], s[P_SIGMA], s[P_RGB] = (W, W), (H, W + cd + (n_a if has_a else 0)), (1, W), (3, H)
    if has_t:
        s[P_T0] = (H, W + n_tau)
        s.update({P_T0 + j: (H, H) for j in (1, 2, 3)})
        s[P_TSIGMA], s[P_TRGB], s[P_TBETA] = (1, H), (3, H), (1, H)
    return s


def _fwd(blocks, segs):
    return (0, 0, 0, tuple(blocks), tuple(s + (-1,) for s in segs))


def _dense(layer, rows, segs):
    return [_fwd([(layer, min(32, rows - 32 * i), 32 * i, 0)], segs) for i in range((rows + 31) // 32)]


def forward_tiles(widths, has_a, has_t):
    nx, nd, n_a, n_tau = widths
    cx, cd, nkp = 6 * nx + 3, 6 * nd + 3, nkp_for(nx)
    t = _dense(P_XYZ1, W, [(nkp, NAT, 0, cx)])                                               # L1
    for i in range(1, 8):
        t += _dense(P_XYZ1 + i, W, [(nkp, NAT, 0, cx), (16, ACT, cx, W)] if i == 4 else [(16, ACT, 0, W)])
    t += _dense(P_SIGMA, 1, [(16, ACT, 0, W)])                                               # SIG
    t += _dense(P_DIR, H, [(16, ACT, 0, W), (2, NAT, W, cd)] + ([(3, NAT, W + cd, n_a)] if has_a else []))
    t += _dense(P_RGB, 3, [(8, ACT, 0, H)])
    if has_t:
        t += _dense(P_T0, H, [(16, ACT, 0, W), (1, NAT, W, n_tau)])                          # T1 = h8 | tau
        for j in (1, 2, 3):
            t += _dense(P_T0 + j, H, [(8, ACT, 0, H)])
        t.append(_fwd([(P_TSIGMA, 1, 0, 0), (P_TRGB, 3, 0, 1), (P_TBETA, 1, 0, 8)], [(8, ACT, 0, H)]))      # THEAD
    return tuple(t)


def dgrad_tiles(widths, has_a, has_t, rays_grad):
    nx, nd, n_a, n_tau = widths
    cx, cd, nkp = 6 * nx + 3, 6 * nd + 3, nkp_for(nx)
    tt = lambda tcol0, tncols, segs: (1, tcol0, tncols, (), tuple(segs))
    pos = lambda layer: [tt(32 * t, max(0, min(32, cx - 32 * t)), [(16, ACT, 0, W, layer)]) for t in range((nkp + 1) // 2)]
    out = []
    if has_t:
        out += [tt(32 * t, 32, [(1, NAT, 0, 1, P_TSIGMA), (1, NAT, 0, 3, P_TRGB), (1, NAT, 0, 1, P_TBETA)]) for t in range(4)]
        for j in (3, 2, 1):
            out += [tt(32 * t, 32, [(8, ACT, 0, H, P_T0 + j)]) for t in range(4)]
        out.append(tt(W, n_tau, [(8, ACT, 0, H, P_T0)]))
    out += [tt(32 * t, 32, [(1, NAT, 0, 3, P_RGB)]) for t in range(4)]
    if has_a:
        out += [tt(W + cd, min(n_a, 32), [(8, ACT, 0, H, P_DIR)]), tt(W + cd + 32, max(n_a - 32, 0), [(8, ACT, 0, H, P_DIR)])]
    if rays_grad:
        out.append(tt(W, cd, [(8, ACT, 0, H, P_DIR)]))
    for t in range(8):
        out.append(tt(32 * t, 32, [(8, ACT, 0, H, P_DIR)] + ([(8, ACT, 0, H, P_T0)] if has_t else []) + [(1, NAT, 0, 1, P_SIGMA)]))
    for l in range(8, 1, -1):                          # layer l, 1-based
        out += [tt((cx if l == 5 else 0) + 32 * t, 32, [(16, ACT, 0, W, P_XYZ1 + l - 1)]) for t in range(8)]
        if l == 5 and rays_grad:
            out += pos(P_XYZ1 + 4)
    if rays_grad:
        out += pos(P_XYZ1)
    return tuple(out)


def slot_columns(kind, nks):
    """(nks, 64 lanes, 8) column offset `map(k-slot)` of a segment of `nks` k-steps: the two maps of nfl_plan.h, lane half
    h = lane >> 5."""
    ks = torch.arange(nks).view(nks, 1, 1)
    h = (torch.arange(64) >> 5).view(1, 64, 1)
    j = torch.arange(8).view(1, 1, 8)
    if kind == NAT:
        return 16 * ks + 8 * h + j
    return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3)


def frag_offsets(tiles):
    """First k-step of every tile, and the stream's k-step total."""
    off, n = [], 0
    for t in tiles:
        off.append(n)
        n += sum(s[0] for s in t[4])
    return off, n


@functools.lru_cache(maxsize=None)
def index(tiles):
    """(idx, bidx, tile): idx (total_ks, 64, 8, 3) int32 names the (layer, row, col) of the weight at fp16 position
    (k-step, lane, j) of the hi image (and of the lo image), layer PAD where nothing lands; bidx (n_rt, 32, 2) the
    (layer, row) of the bias in every row of the bias table; tile (total_ks,) the tile each k-step belongs to.  Cached
    per layout: do not write to the result."""
    off, total = frag_offsets(tiles)
    idx = torch.full((total, 64, 8, 3), PAD, dtype=torch.int32)
    bidx = torch.full((len(tiles), 32, 2), PAD, dtype=torch.int32)
    tile = torch.zeros(total, dtype=torch.int32)
    row = (torch.arange(64) & 31).view(1, 64, 1)
    for n, (trans, tcol0, tncols, blocks, segs) in enumerate(tiles):
        # forward tiles: layer and source row of every tile row
        lay_r, src_r = torch.full((32,), PAD), torch.zeros(32, dtype=torch.long)
        for layer, nrows, src_row0, dst_row in blocks:
            lay_r[dst_row:dst_row + nrows] = layer
            src_r[dst_row:dst_row + nrows] = torch.arange(src_row0, src_row0 + nrows)
        if not trans:
            bidx[n, :, 0], bidx[n, :, 1] = lay_r, torch.where(lay_r >= 0, src_r, torch.full_like(src_r, PAD))
        ks0 = off[n]
        for nks, kind, col0, ncols, layer in segs:
            m = slot_columns(kind, nks).expand(nks, 64, 8)
            r = row.expand(nks, 64, 8)
            if trans:
                ok = (m < ncols) & (r < tncols)
                ent = torch.stack([torch.full_like(m, layer), col0 + m, tcol0 + r], -1)
            else:
                ok = (m < ncols) & (lay_r[r] >= 0)
                ent = torch.stack([lay_r[r], src_r[r], col0 + m], -1)
            ent = torch.where(ok.unsqueeze(-1), ent, torch.full_like(ent, PAD))
            idx[ks0:ks0 + nks] = ent.to(torch.int32)
            tile[ks0:ks0 + nks] = n
            ks0 += nks
    return idx, bidx, tile


def round_hi_lo(w):
    """The packer's round-to-nearest split: hi = fp16(w), lo = fp16(w - hi) (the subtraction is exact in fp32)."""
    hi = w.half()
    return hi, (w - hi.float()).half()


def fp16_neighbours(w):
    """Where fp32 `w` (|w| <= 65504) lies between two fp16 values: (toward, f, ulp).  toward = int16 bit pattern of the
    neighbour toward zero, with w's sign (the neighbour away from zero is the next pattern, toward + 1, across the
    subnormal range and the binades alike); f = the fraction of the interval that a truncation discards, in [0, 1), and
    ulp = the interval's width, both float64 and exact: |w| = |toward| + f ulp.  In the normal range f is the low 13
    mantissa bits / 8192, below 2^-14 the interval is 2^-24 wide."""
    a = w.double().abs()
    e = torch.frexp(a)[1]                                                      # a in [2^(e-1), 2^e)
    ulp = torch.where(a >= 2.0 ** -14, torch.ldexp(torch.ones_like(a), e - 11), torch.full_like(a, 2.0 ** -24))
    q = a / ulp
    k = q.floor()
    toward = (k * ulp).half().view(torch.int16)
    return torch.where(torch.signbit(w), toward | -32768, toward), q - k, ulp


def _gather(ix, tensors, col):
    """Values of `tensors[layer]` (2-D, or 1-D with col None) at the (layer, row[, col]) entries of ix; 0 at PAD."""
    layers = sorted(tensors)
    base, n = {}, 0
    for l in layers:
        base[l] = n
        n += tensors[l].numel()
    flat = torch.cat([tensors[l].reshape(-1) for l in layers] + [torch.zeros(1)])
    lay = ix[..., 0].long()
    present = [l for l in lay.unique().tolist() if l != PAD]
    assert all(l in tensors for l in present), "the stream names a layer the caller did not pass"
    b = torch.full((max(layers) + 2,), 0, dtype=torch.long)
    ld = torch.ones(max(layers) + 2, dtype=torch.long)
    for l in layers:
        b[l] = base[l]
        ld[l] = tensors[l].shape[1] if col else 1
    pos = b[lay] + ix[..., 1].long() * ld[lay] + (ix[..., 2].long() if col else 0)
    return flat[torch.where(lay == PAD, torch.full_like(pos, n), pos)]


def gather_weights(tiles, params):
    """fp32 (total_ks, 64, 8): the weight at every position of the stream, +0 at padding."""
    return _gather(index(tiles)[0], {l: p[0] for l, p in params.items()}, True)


def encode(tiles, params, split):
    """(hi, lo, bias, idx): hi / lo = uint8 (total_ks, 1024) images of the round-to-nearest stream (lo None unless `split`),
    bias = fp32 (n_rt, 32) table, idx = index(tiles)[0]."""
    idx, bidx, _ = index(tiles)
    hi, lo = round_hi_lo(gather_weights(tiles, params))
    bias = _gather(bidx, {l: p[1] for l, p in params.items()}, False)
    as_bytes = lambda x: x.reshape(x.shape[0], 512).view(torch.uint8)
    return as_bytes(hi), (as_bytes(lo) if split else None), bias, idx


def assemble(hi, lo, bias):
    """The packed buffer as the library lays it out: per k-step the hi image (then the lo image), then the bias table."""
    img = hi if lo is None else torch.stack([hi, lo], 1)
    return torch.cat([img.reshape(-1), bias.contiguous().view(torch.uint8).reshape(-1)])


def locate(tiles, ks, lane, j):
    """Human-readable place of one fp16 position, for failure messages."""
    idx, _, tile = index(tiles)
    t = int(tile[ks])
    off, _ = frag_offsets(tiles)
    return f"tile {t} k-step {ks - off[t]} (stream k-step {ks}) lane {lane} j {j} -> (layer, row, col) = {tuple(idx[ks, lane, j].tolist())}"


# ---- the library's side: NflPlan as a numpy record, and the plans its builders write ----------------------------------
# The struct as nfl_plan.h declares it (NflBlk, NflSeg, NflRowTile, NflPlan; NFL_MAX_RT 112, NFL_MAX_CHUNKS 104).
BLK_DTYPE = np.dtype([("layer", "<i2"), ("nrows", "<i2"), ("src_row0", "<i2"), ("dst_row", "<i2")])
SEG_DTYPE = np.dtype([("nks", "<i2"), ("kind", "<i2"), ("col0", "<i2"), ("ncols", "<i2"), ("layer", "<i2"), ("pad", "<i2", 3)])
TILE_DTYPE = np.dtype([("frag_off", "<i4"), ("nks", "<i4"), ("nblk", "<i4"), ("nseg", "<i4"), ("trans", "<i2"), ("tcol0", "<i2"),
                       ("tncols", "<i2"), ("pad", "<i2"), ("blk", BLK_DTYPE, 3), ("seg", SEG_DTYPE, 3)])
_HEAD = ["magic", "prec", "nsplit", "elem", "is_bwd", "reserved_flags", "n_emb_xyz", "nkp", "has_a", "has_t", "n_a", "n_tau", "n_rt",
         "n_rt_sigma", "n_rt_static", "n_chunks", "n_chunks_sigma", "n_chunks_static", "total_ks", "ks_bytes", "max_chunk_ks",
         "stream_bytes", "bias_off", "packed_bytes"]
PLAN_DTYPE = np.dtype([(n, "<u4" if n == "magic" else "<i4") for n in _HEAD]
                      + [("beta_min", "<f4"), ("ld", "<i4", 19), ("chunk_off", "<i4", 105), ("chunk_aux", "<i4", 105),
                         ("rt", TILE_DTYPE, 112)])
PLAN_HEADER_INTS = 254
PLAN_MAGIC = 0x4E464C31


def desc_of(widths, kind):
    from nerf_fl_amd import _lib
    has_a, has_t = KINDS[kind]
    return _lib.FieldDesc(n_emb_xyz=widths[0], n_emb_dir=widths[1], encode_appearance=int(has_a), n_a=widths[2],
                          encode_transient=int(has_t), n_tau=widths[3], beta_min=0.03, reserved=0)


def build_plan(widths, kind, prec, rays_grad=None):
    """(host plan blob, record view of it) from nfl_plan_build (rays_grad None) or nfl_bwd_plan_build."""
    from nerf_fl_amd import _lib
    L = _lib.lib()
    d = desc_of(widths, kind)
    n = L.nfl_plan_bytes(C.byref(d))
    h = C.create_string_buffer(n)
    rc = L.nfl_plan_build(C.byref(d), prec, h, n) if rays_grad is None else L.nfl_bwd_plan_build(C.byref(d), int(rays_grad), prec, h, n)
    assert rc == 0, rc
    return h, np.frombuffer(h, dtype=PLAN_DTYPE, count=1)[0]


def plan_tiles(plan):
    """The tiles of a built plan in this module's tuple form."""
    out = []
    for t in plan["rt"][:int(plan["n_rt"])]:
        blocks = tuple((int(b["layer"]), int(b["nrows"]), int(b["src_row0"]), int(b["dst_row"])) for b in t["blk"][:int(t["nblk"])])
        segs = tuple((int(s["nks"]), int(s["kind"]), int(s["col0"]), int(s["ncols"]), int(s["layer"])) for s in t["seg"][:int(t["nseg"])])
        out.append((int(t["trans"]), int(t["tcol0"]), int(t["tncols"]), blocks, segs))
    return tuple(out)
