"""PSNR, masked PSNR, SSIM and depth images on the device (the reference's metrics.py and utils/visualization.py).

One HIP entry point, nfl_image_metrics (csrc/nfl_metrics.hip), reads the fp32 prediction and the ground truth where they
lie -- the uint8 image of a data.ImageBank, or an fp32 tensor -- and leaves one row of 8 fp64 numbers (METRIC_COLUMNS) in
a table on the device: a whole split is scored without a host sync and read back with one copy.  `psnr` and `ssim` keep
the reference's argument order and return 0-d device tensors.  SSIM is kornia 0.4.1's (window 3, sigma 1.5, reflected
border), as the reference's metrics.ssim calls it; its definition is written out in include/nerf_fl_amd.h.

There is no CPU path.
"""
import ctypes as C

import torch

from . import _lib

__all__ = ["METRIC_COLUMNS", "image_metrics", "psnr", "ssim", "depth_image"]

METRIC_COLUMNS = ("sse", "count", "sse_valid", "count_valid", "ssim_sum", "psnr", "psnr_valid", "ssim")
assert len(METRIC_COLUMNS) == _lib.NFL_METRIC_COLUMNS


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _region(region, H, W):
    x0, x1, y0, y1 = (0, W, 0, H) if region is None else (int(v) for v in region)
    if not (0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H):
        raise ValueError(f"region {(x0, x1, y0, y1)} (x0, x1, y0, y1) outside the {W} x {H} image")
    return x0, x1, y0, y1


def _device_tensor(t, dtype, numel, what, dev):
    if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of {numel} elements on {dev}")
    return t


def image_metrics(pred, H, W, *, bank=None, image=None, target=None, mask=None, region=None, clip=True, table=None,
                  slot=0, want_uint8=False, want_map=False):
    """Score the (H*W, 3) fp32 prediction `pred` (pixel order, on the device) against its ground truth:
    bank form `bank=ImageBank, image=i` (the H x W uint8 image i, converted as ImageBank.gather converts it; valid =
    alpha > 0 for RGBA), or tensor form `target` (H*W, 3) fp32 with an optional `mask` (H*W,) bool / uint8 (valid =
    mask != 0).  region = (x0, x1, y0, y1) crops both first (default: the whole image; at least 2 x 2 pixels, or empty);
    clip clamps the prediction to [0, 1] first.

    Row `slot` of `table` ((n, 8) fp64 on the device; None: a new torch.zeros(1, 8)) receives METRIC_COLUMNS; an empty
    region leaves it untouched.  Returns the table, or (table, uint8 (h, w, 3) by eval.to_uint8's rule if want_uint8,
    fp32 SSIM map (h, w, 3) if want_map).  Nothing here synchronises with the host."""
    H, W = int(H), int(W)
    if not torch.is_tensor(pred) or pred.device.type != "cuda":
        raise RuntimeError("nerf_fl_amd.metrics needs tensors on a ROCm device (this build has no CPU path)")
    dev = pred.device
    _device_tensor(pred, torch.float32, H * W * 3, "pred", dev)
    if (bank is None) == (target is None):
        raise ValueError("image_metrics: give the ground truth as bank=, image= or as target=")
    a = _lib.MetricsArgs()
    keep = []
    if bank is not None:
        if mask is not None:
            raise ValueError("image_metrics: mask= goes with target= (a bank's valid pixels are its alpha > 0)")
        if bank.device is None or bank.device != dev:
            raise ValueError(f"image_metrics: the bank is on {bank.device}, the prediction on {dev}")
        image = int(image)
        if not 0 <= image < bank.n_images:
            raise ValueError(f"image {image} outside the bank's {bank.n_images} images")
        rec = bank.host_table[image]
        if (int(rec["height"]), int(rec["width"])) != (H, W):
            raise ValueError(f"image {image} is {int(rec['width'])} x {int(rec['height'])}, the prediction {W} x {H}")
        a.d_pixels, a.d_table, a.n_images, a.image = _ptr(bank.pixels), _ptr(bank.table), bank.n_images, image
    else:
        if image is not None:
            raise ValueError("image_metrics: image= goes with bank=")
        a.d_target = _ptr(_device_tensor(target, torch.float32, H * W * 3, "target", dev))
        if mask is not None:
            if torch.is_tensor(mask) and mask.dtype == torch.bool:
                mask = mask.contiguous().view(torch.uint8)
            keep.append(_device_tensor(mask, torch.uint8, H * W, "mask", dev))
            a.d_mask = _ptr(mask)
    x0, x1, y0, y1 = _region(region, H, W)
    w, h = x1 - x0, y1 - y0
    if w * h and (w < 2 or h < 2):
        raise ValueError("image_metrics: a region is at least 2 x 2 pixels (the SSIM border is a reflection)")
    if table is None:
        table = torch.zeros(1, len(METRIC_COLUMNS), dtype=torch.float64, device=dev)
    _device_tensor(table, torch.float64, table.numel() if torch.is_tensor(table) else 0, "table", dev)
    if table.dim() != 2 or table.shape[1] != len(METRIC_COLUMNS) or not 0 <= int(slot) < table.shape[0]:
        raise ValueError(f"table must be (n, {len(METRIC_COLUMNS)}) with slot < n")
    lib = _lib.lib()
    nbytes = lib.nfl_image_metrics_scratch_bytes(h, w)
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    u8 = torch.empty(h, w, 3, dtype=torch.uint8, device=dev) if want_uint8 else None
    smap = torch.empty(h, w, 3, dtype=torch.float32, device=dev) if want_map else None
    a.d_pred, a.width, a.height = _ptr(pred), W, H
    a.x0, a.x1, a.y0, a.y1 = x0, x1, y0, y1
    a.clip, a.slot = int(bool(clip)), int(slot)
    a.d_results, a.n_slots = _ptr(table), table.shape[0]
    a.d_scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * 8
    a.d_pred_u8, a.d_ssim_map = _ptr(u8), _ptr(smap)
    with torch.cuda.device(dev):
        _lib.check(lib.nfl_image_metrics(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "nfl_image_metrics")
    if not (want_uint8 or want_map):
        return table
    return (table,) + ((u8,) if want_uint8 else ()) + ((smap,) if want_map else ())


def _rows(x, what):
    """(N, 3) fp32 contiguous view of an image tensor of the reference's shapes ((N, 3), (H, W, 3))."""
    if x.shape[-1] != 3:
        raise ValueError(f"{what}: expected (..., 3) colours, got {tuple(x.shape)}")
    return x.to(torch.float32).reshape(-1, 3).contiguous()


def psnr(image_pred, image_gt, valid_mask=None):
    """The reference's metrics.psnr(image_pred, image_gt, valid_mask) with reduction='mean': -10 log10 of the mean squared
    error over all elements, or over the pixels of `valid_mask` ((N,) or (H, W) bool).  (..., 3) tensors on the device;
    returns a 0-d fp64 device tensor.  The prediction is not clipped."""
    p, t = _rows(image_pred, "image_pred"), _rows(image_gt, "image_gt")
    n = p.shape[0]
    if t.shape[0] != n:
        raise ValueError("psnr: prediction and ground truth differ in size")
    if n < 2:
        raise ValueError("psnr: at least 2 pixels")
    col = METRIC_COLUMNS.index("psnr" if valid_mask is None else "psnr_valid")
    if valid_mask is not None:
        valid_mask = valid_mask.reshape(-1).to(torch.bool).contiguous()
    # the squared error has no neighbourhood, so the pixels are scored as an image 64 (.. 2) columns wide; an odd count
    # (or 2 pixels) as two rows holding the pixels twice: both sums double and the means are unchanged
    w = next((w for w in (64, 32, 16, 8, 4, 2) if n % w == 0 and n // w >= 2), None)
    if w is not None:
        h = n // w
    else:
        h, w = 2, n
        p, t = torch.cat([p, p]), torch.cat([t, t])
        valid_mask = None if valid_mask is None else torch.cat([valid_mask, valid_mask])
    return image_metrics(p, h, w, target=t, mask=valid_mask, clip=False)[0, col]


def ssim(image_pred, image_gt, H=None, W=None):
    """The reference's metrics.ssim(image_pred, image_gt) with reduction='mean': `1 - 2 * kornia.losses.ssim(pred, gt, 3)`.
    Takes the reference's (1, 3, H, W) layout, or (H*W, 3) / (H, W, 3) with H, W given.  Returns a 0-d fp64 device
    tensor.  The prediction is not clipped."""
    if H is None:
        if image_pred.dim() != 4 or image_pred.shape[0] != 1 or image_pred.shape[1] != 3:
            raise ValueError("ssim: expected (1, 3, H, W), or (H*W, 3) with H and W")
        H, W = image_pred.shape[2:]
        image_pred, image_gt = (x[0].permute(1, 2, 0) for x in (image_pred, image_gt))
    return image_metrics(_rows(image_pred, "image_pred"), H, W, target=_rows(image_gt, "image_gt"), clip=False)[0, 7]


def depth_image(depth, H, W, region=None, lut=None):
    """utils/visualization.py's visualize_depth on the device: NaN -> 0, normalised by the minimum and maximum over the
    region, 256 levels; returns uint8 (h, w, 3): the level in all three channels, or lut[level] of a (256, 3) uint8 table
    (the reference applies OpenCV's JET table; none ships here)."""
    H, W = int(H), int(W)
    if not torch.is_tensor(depth) or depth.device.type != "cuda":
        raise RuntimeError("nerf_fl_amd.metrics needs tensors on a ROCm device (this build has no CPU path)")
    dev = depth.device
    _device_tensor(depth, torch.float32, H * W, "depth", dev)
    x0, x1, y0, y1 = _region(region, H, W)
    w, h = x1 - x0, y1 - y0
    if lut is not None:
        _device_tensor(lut, torch.uint8, 768, "lut", dev)
    out = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    if h * w == 0:
        return out
    lib = _lib.lib()
    scratch = torch.empty(max(lib.nfl_depth_image_scratch_bytes(h, w) // 4, 1), dtype=torch.float32, device=dev)
    a = _lib.DepthArgs(_ptr(depth), W, H, x0, x1, y0, y1, _ptr(lut), _ptr(out), _ptr(scratch), scratch.numel() * 4)
    with torch.cuda.device(dev):
        _lib.check(lib.nfl_depth_image(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_depth_image")
    return out
