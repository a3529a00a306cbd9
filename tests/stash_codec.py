"""The two training stashes as ordinary tensors, and back; plus the map from stash operands to weight gradients.

A plain helper for the weight-gradient tests (no pytest hooks).  Everything here is written from the documentation of the
formats, not from the kernels' tile tables:

* the record maps of csrc/nfl_plan.h (nfl_act_h / _d / _dirh / _tau / _g / _slots, NFL_GRD_D / DIRH / G / HEADS / SLOTS);
* the two feature orders of a k-step (NFL_SEG_ACT, NFL_SEG_NAT, same header);
* the k-step image of csrc/nfl_wgrad.hip: 1 KiB = [32 samples][2 lane halves][8 fp16], a sample's 16 values contiguous;
* split stashes: a segment's record is [hi record | lo record] of the same layout;
* the model, dW_l = sum_s delta_l (x) h_{l-1}, and the composition formulas in the header comment of csrc/nfl_wgrad.hip.

The only thing taken from a built plan is the number of position-encoding k-steps (`nkp_of_plan`).

Field names.  Activation stash: `pe`, `h1`..`h8`, `dir_side` ([dir PE | appearance code], as dir_encoding.0 reads it behind
its 256 feature columns), `dirh`, `tau`, `g1`..`g4`.  Gradient stash: `delta1`..`delta8`, `delta_dirh`, `delta_g1`..`delta_g4`,
`heads0`..`heads4` (d sigma, d rgb, d sigma_t, d rgb_t, d beta).  Every tensor is (n_seg * 32, width), sample-major.
"""
import ctypes as C

import torch

NAT, ACT = "nat", "act"
W, H = 256, 128
HEAD_WIDTHS = (1, 3, 1, 3, 1)
GRD_SLOTS = 173


def nkp_of_plan(h_wplan):
    """Position-encoding k-steps of the kernel instantiation that runs the field: WgPlan.act_slots - 174, read through a
    view of the struct's first four int32 (magic, n_jobs, act_slots, grd_slots)."""
    return (C.c_int32 * 4).from_buffer(h_wplan)[2] - 174


def feature_of_position(order, n):
    """Feature held at position i = 16 * ks + 8 * h + j of a field of n / 16 k-steps (nfl_plan.h, k-slot -> column maps)."""
    i = torch.arange(n)
    if order == NAT:
        return i
    ks, h, j = i // 16, (i // 8) % 2, i % 8
    return 32 * (ks // 2) + 16 * (ks % 2) + 8 * (j // 4) + 4 * h + (j % 4)


class Layout:
    """Where every named tensor lives in a segment's record.  A field is a list of pieces (slot0, k-steps, order, col0,
    width): columns [col0, col0 + width) of the tensor occupy the k-steps from slot0 on, feature f at the position the
    order gives it; positions of features beyond `width` are padding that no gradient reads."""

    def __init__(self, n_emb_xyz, n_emb_dir, n_a, n_tau, nkp, has_a=True, has_t=True):
        self.cx, self.cd = 6 * n_emb_xyz + 3, 6 * n_emb_dir + 3
        self.n_a, self.n_tau = (n_a if has_a else 0), (n_tau if has_t else 0)
        self.has_a, self.has_t, self.nkp = has_a, has_t, nkp
        assert self.cx <= 16 * nkp and self.cd <= 32 and self.n_a <= 48 and self.n_tau <= 16
        a = {"pe": [(0, nkp, NAT, 0, self.cx)]}
        for l in range(1, 9):
            a[f"h{l}"] = [(nkp + 16 * (l - 1), 16, ACT, 0, W)]
        a["dir_side"] = [(nkp + 128, 2, NAT, 0, self.cd)] + ([(nkp + 130, 3, NAT, self.cd, self.n_a)] if has_a else [])
        a["dirh"] = [(nkp + 133, 8, ACT, 0, H)]
        g = {f"delta{l}": [(16 * (l - 1), 16, ACT, 0, W)] for l in range(1, 9)}
        g["delta_dirh"] = [(128, 8, ACT, 0, H)]
        heads = 5 if has_t else 2
        if has_t:
            a["tau"] = [(nkp + 141, 1, NAT, 0, self.n_tau)]
            for m in range(1, 5):
                a[f"g{m}"] = [(nkp + 142 + 8 * (m - 1), 8, ACT, 0, H)]
                g[f"delta_g{m}"] = [(136 + 8 * (m - 1), 8, ACT, 0, H)]
        for k in range(heads):
            g[f"heads{k}"] = [(168 + k, 1, NAT, 0, HEAD_WIDTHS[k])]
        self.act, self.grd = a, g
        self.act_slots, self.grd_slots = nkp + 174, GRD_SLOTS

    def width(self, name):
        return sum(p[4] for p in (self.act.get(name) or self.grd[name]))

    def widths(self):
        return {n: self.width(n) for n in list(self.act) + list(self.grd)}

    # ---- one stash
    @staticmethod
    def _records(stash, n_seg, slots, mult):
        """(n_seg, mult, slots, 32 samples, 16 values) fp16 view of the records at the head of a stash buffer."""
        nb = n_seg * mult * slots * 1024
        return stash[:nb].view(torch.float16).view(n_seg, mult, slots, 32, 16)

    @staticmethod
    def _put(rec, fields, tensors, count=None):
        for name, pieces in fields.items():
            x = tensors[name]
            n_seg = rec.shape[0]
            assert x.shape == (n_seg * 32, sum(p[4] for p in pieces)), (name, tuple(x.shape))
            for slot0, nks, order, col0, width in pieces:
                pos = feature_of_position(order, 16 * nks).to(x.device)
                ok = pos < width
                img = torch.zeros(n_seg, 32, 16 * nks, dtype=rec.dtype, device=x.device)
                img[:, :, ok] = x[:, col0:col0 + width].reshape(n_seg, 32, width)[:, :, pos[ok]].to(rec.dtype)
                dst = rec[:, slot0:slot0 + nks]                                  # (n_seg, nks, 32, 16)
                okk = ok.view(nks, 1, 16).expand(nks, 32, 16)
                dst[:, okk] = img.view(n_seg, 32, nks, 16).permute(0, 2, 1, 3)[:, okk]
                if count is not None:
                    count[slot0:slot0 + nks][okk] += 1

    @staticmethod
    def _get(rec, fields):
        out = {}
        for name, pieces in fields.items():
            cols = []
            for slot0, nks, order, col0, width in pieces:
                pos = feature_of_position(order, 16 * nks).to(rec.device)
                img = rec[:, slot0:slot0 + nks].permute(0, 2, 1, 3).reshape(rec.shape[0] * 32, 16 * nks)
                inv = torch.empty(width, dtype=torch.long, device=rec.device)
                ok = pos < width
                inv[pos[ok]] = torch.arange(16 * nks, device=rec.device)[ok]
                cols.append(img[:, inv])
            out[name] = torch.cat(cols, 1)
        return out

    def encode(self, hi, lo=None, fill=0.0):
        """Named tensors -> (activation stash, gradient stash) record bytes (uint8, on the tensors' device).  `lo`: a second
        set for split stashes, placed behind every hi record.  Positions that no field names hold `fill`."""
        mult = 1 if lo is None else 2
        first = hi["pe"]
        n_seg = first.shape[0] // 32
        out = []
        for fields, slots in ((self.act, self.act_slots), (self.grd, self.grd_slots)):
            buf = torch.full((n_seg * mult * slots * 512,), fill, dtype=torch.float16, device=first.device).view(torch.uint8)
            rec = self._records(buf, n_seg, slots, mult)
            self._put(rec[:, 0], fields, hi)
            if lo is not None:
                self._put(rec[:, 1], fields, lo)
            out.append(buf)
        return tuple(out)

    def decode(self, act, grd, n_seg, mult=1):
        """Stash bytes -> (hi, lo) dicts of fp16 tensors (lo is None for mult 1).  The buffers may be longer than the records
        (the library pads them and keeps the relu masks behind the activation records)."""
        ra, rg = self._records(act, n_seg, self.act_slots, mult), self._records(grd, n_seg, self.grd_slots, mult)
        hi = dict(self._get(ra[:, 0], self.act), **self._get(rg[:, 0], self.grd))
        lo = dict(self._get(ra[:, 1], self.act), **self._get(rg[:, 1], self.grd)) if mult == 2 else None
        return hi, lo

    def coverage(self):
        """How many fields write each fp16 position of one activation / gradient record: (slots, 32, 16) int tensors."""
        out = []
        for fields, slots in ((self.act, self.act_slots), (self.grd, self.grd_slots)):
            count = torch.zeros(slots, 32, 16, dtype=torch.int32)
            rec = torch.zeros(1, slots, 32, 16, dtype=torch.float16)
            self._put(rec, fields, {n: torch.zeros(32, sum(p[4] for p in ps)) for n, ps in fields.items()}, count)
            out.append(count)
        return tuple(out)


# ---- the relu-mask records behind the activation records ---------------------------------------------------------------
# Written from the documentation: nfl_plan.h (nfl_msk_h / _dirh / _g, NFL_MSK_WORDS, nfl_msk_offset, the record layout
# [group of 4 tiles][lane][4 words] and the bit rule: bit 2p = accumulator 2p, bit 16 + 2p = accumulator 2p + 1) and the
# 32x32 MFMA accumulator layout (lane = 32 * half + sample; accumulator r holds row (r & 3) + 8 * (r >> 2) + 4 * half of the
# tile).  A mask is a boolean (n_seg * 32, width) tensor, sample-major like every other field; tile t covers features
# 32 t .. 32 t + 31.  The records are the same for one-image and split activation records; only their offset differs.
MSK_WORDS = 84


def mask_fields(has_t=True):
    """name -> (first word, row tiles), nfl_msk_h / nfl_msk_dirh / nfl_msk_g."""
    m = {f"h{l}": (8 * (l - 1), 8) for l in range(1, 9)}
    m["dirh"] = (64, 4)
    if has_t:
        m.update({f"g{k}": (68 + 4 * (k - 1), 4) for k in range(1, 5)})
    return m


def mask_offset(n_seg, nkp, mult=1):
    """nfl_msk_offset: the records, their 4 KiB tail pad, then the masks."""
    return n_seg * (nkp + 174) * mult * 1024 + 4096


def mask_bit_of_row():
    """(half, bit) of each of a tile's 32 rows: row = (r & 3) + 8 (r >> 2) + 4 half, bit = r - (r & 1) + 16 (r & 1)."""
    row = torch.arange(32)
    half, r = (row >> 2) & 1, (row & 3) + 4 * (row >> 3)
    return half, (r & ~1) + 16 * (r & 1)


def _mask_words(buf, n_seg):
    """(n_seg, 21 groups, 64 lanes, 4 words) int32 view of the mask records at the head of `buf` (uint8)."""
    return buf[:n_seg * MSK_WORDS * 256].view(torch.int32).view(n_seg, MSK_WORDS // 4, 64, 4)


def encode_masks(masks, has_t=True, count=None):
    """Boolean tensors -> mask records (uint8, n_seg * 84 * 256 bytes).  Words of fields that are not given, and the bits no
    accumulator owns, are zero.  `count` ((84, 64, 32) int): incremented at every (word, lane, bit) written."""
    n_seg = next(iter(masks.values())).shape[0] // 32
    dev = next(iter(masks.values())).device
    buf = torch.zeros(n_seg * MSK_WORDS * 256, dtype=torch.uint8, device=dev)
    words = _mask_words(buf, n_seg)
    half, bit = (x.to(dev) for x in mask_bit_of_row())
    for name, (w0, tiles) in mask_fields(has_t).items():
        if name not in masks:
            continue
        m = masks[name]
        assert m.dtype == torch.bool and m.shape == (n_seg * 32, 32 * tiles), (name, tuple(m.shape))
        m = m.view(n_seg, 32, tiles, 32).permute(0, 2, 1, 3).to(torch.int32)          # (segment, tile, sample, row)
        for t in range(tiles):
            w = w0 + t
            for h in (0, 1):
                rows = (half == h).nonzero().flatten()
                val = (m[:, t][:, :, rows] << bit[rows].to(torch.int32)).sum(-1).to(torch.int32)      # (segment, sample)
                words[:, w >> 2, 32 * h:32 * h + 32, w & 3] = val
                if count is not None:
                    count[w, 32 * h:32 * h + 32, bit[rows]] += 1
    return buf


def decode_masks(buf, n_seg, has_t=True):
    """Mask records (the bytes from mask_offset on) -> name -> boolean (n_seg * 32, width)."""
    words = _mask_words(buf, n_seg)
    half, bit = (x.to(buf.device) for x in mask_bit_of_row())
    out = {}
    for name, (w0, tiles) in mask_fields(has_t).items():
        m = torch.zeros(n_seg, tiles, 32, 32, dtype=torch.bool, device=buf.device)
        for t in range(tiles):
            w = w0 + t
            for h in (0, 1):
                rows = (half == h).nonzero().flatten()
                val = words[:, w >> 2, 32 * h:32 * h + 32, w & 3]                              # (segment, sample)
                m[:, t][:, :, rows] = ((val[..., None] >> bit[rows].to(torch.int32)) & 1).bool()
        out[name] = m.permute(0, 2, 1, 3).reshape(n_seg * 32, 32 * tiles)
    return out


# ---- which stash operands form which gradient (the tests' oracle) ----------------------------------------------------
# layer -> (gradient field, [(input field, first weight column it multiplies)]).  "feat" is the output of
# xyz_encoding_final, which is never stashed: feat = W_fin h8 + b_fin, so
#   sum_s delta (x) feat = (sum_s delta (x) h8) W_fin^T + (sum_s delta) (x) b_fin
# and xyz_encoding_final's own gradient is sum_s delta_feat (x) h8 with delta_feat = Wd^T delta_dirh (+ Wt^T delta_g1),
# Wd / Wt the first 256 columns of dir_encoding.0 / transient_encoding.0.
def grad_map(layout, use_transient):
    m = {}
    for l in range(1, 9):
        ins = [("pe", 0)] if l == 1 else [("pe", 0), ("h4", layout.cx)] if l == 5 else [(f"h{l - 1}", 0)]
        m[f"xyz_encoding_{l}.0"] = (f"delta{l}", ins)
    m["static_sigma.0"] = ("heads0", [("h8", 0)])
    m["dir_encoding.0"] = ("delta_dirh", [("feat", 0), ("dir_side", W)])
    m["static_rgb.0"] = ("heads1", [("dirh", 0)])
    if use_transient:
        m["transient_encoding.0"] = ("delta_g1", [("feat", 0), ("tau", W)])
        for k, j in enumerate((2, 4, 6)):
            m[f"transient_encoding.{j}"] = (f"delta_g{k + 2}", [(f"g{k + 1}", 0)])
        m["transient_sigma.0"] = ("heads2", [("g4", 0)])
        m["transient_rgb.0"] = ("heads3", [("g4", 0)])
        m["transient_beta.0"] = ("heads4", [("g4", 0)])
    return m


def reference_grads(layout, hi, lo, params, use_transient, rows=None, absolute=False):
    """float64 weight / bias gradients (still carrying the stashes' loss scale) from decoded operands, by `grad_map`.
    One-product (lo None): sum delta (x) h, sum delta.  Split: sum (d_hi + d_lo) (x) h_hi + d_hi (x) h_lo, sum (d_hi + d_lo),
    as nfl_mlp_wgrad documents.  `rows`: indices of the samples that take part.  `absolute`: the sum of the absolute values
    of every element's terms instead (all operands and weights replaced by their magnitudes): what bounds its rounding.
    `params`: name -> tensor, needs xyz_encoding_final and the layers that read its output.  Also returns `_G` (and `_Gt`)."""
    dev = hi["h8"].device

    def op(d, name):
        x = d[name].double()
        if rows is not None:
            x = x[rows]
        return x.abs() if absolute else x

    def par(name):
        p = params[name].detach().to(dev).double()
        return p.abs() if absolute else p

    def outer(dn, hn):
        d, h = op(hi, dn), op(hi, hn)
        if lo is None:
            return d.t() @ h
        return (d + op(lo, dn)).t() @ h + d.t() @ op(lo, hn)      # with magnitudes: |d_hi| |h_hi| + |d_lo| |h_hi| + |d_hi| |h_lo|

    def bias(dn):
        return op(hi, dn).sum(0) + (op(lo, dn).sum(0) if lo is not None else 0.0)

    out, feat_readers = {}, []
    for layer, (dn, ins) in grad_map(layout, use_transient).items():
        n_in = max(c0 + (W if hn == "feat" else layout.width(hn)) for hn, c0 in ins)
        dw = torch.zeros(layout.width(dn), n_in, dtype=torch.float64, device=dev)
        db = bias(dn)
        for hn, c0 in ins:
            if hn == "feat":
                G = outer(dn, "h8")
                dw[:, c0:c0 + W] = G @ par("xyz_encoding_final.weight").t() + torch.outer(db, par("xyz_encoding_final.bias"))
                feat_readers.append((layer, G, db))
            else:
                dw[:, c0:c0 + layout.width(hn)] = outer(dn, hn)
        out[layer + ".weight"], out[layer + ".bias"] = dw, db
    dwf, dbf = torch.zeros(W, W, dtype=torch.float64, device=dev), torch.zeros(W, dtype=torch.float64, device=dev)
    for layer, G, db in feat_readers:
        wr = par(layer + ".weight")[:, :W]
        dwf += wr.t() @ G
        dbf += wr.t() @ db
        out["_G" if layer == "dir_encoding.0" else "_Gt"] = G
    out["xyz_encoding_final.weight"], out["xyz_encoding_final.bias"] = dwf, dbf
    return out
