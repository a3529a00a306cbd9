"""Chunked no-grad inference for whole images / video frames (reference eval.py:80-110).

`batched_inference` mirrors the reference helper of the same name: it walks the rays in
chunks of `chunk` rays, calls render_rays(..., test_time=True) on each and concatenates the
per-key results.  Differences that matter on MI355X:

  * results stay on the GPU (the reference moves every chunk to the host, eval.py:106);
  * every chunk has the same shape -- the last, ragged one is padded with copies of its final
    ray and the padding is dropped on write-back -- so one chunk can be captured ONCE into a
    HIP graph (`use_graph=True`) and replayed: a frame becomes a handful of graph launches
    with no per-kernel host work (config 5: 128+128 samples, chunk 131072).
"""
import torch

from . import parallel
from . import rendering as rnd
from .rendering import CameraRays, render_rays

__all__ = ["batched_inference", "GraphedChunk", "frame_rays", "to_uint8", "dolly_path", "render_frame", "render_video",
           "fit_and_evaluate_halves", "evaluate_bank", "clipped_inference", "render_mesh_video", "evaluate_mesh"]


def _chunks(rays, ts, chunk, per_ray=None):
    """Walk B rays in chunks of at most `chunk`: yields (lo, hi, rays chunk, ts chunk, per-ray kwargs of the chunk).
    `rays`: a CameraRays (CameraRays.slice) or a matrix (row slice); `ts` may be None (reference eval.py:94).  A per-ray
    kwarg follows its chunk: a (B, C) tensor is sliced, a (1, C) one (one latent code for the whole frame,
    test_phototourism.ipynb cell 11) is expanded to the chunk's length; None entries are dropped."""
    B = rays.shape[0]
    for lo in range(0, B, chunk):
        hi = min(lo + chunk, B)
        r = rays.slice(lo, hi) if isinstance(rays, CameraRays) else rays[lo:hi]
        kw = {k: v[lo:hi] if v.shape[0] == B and B != 1 else v.expand(hi - lo, -1)
              for k, v in (per_ray or {}).items() if v is not None}
        yield lo, hi, r, None if ts is None else ts[lo:hi], kw


def _fill_padded(buf, v, n):
    """Fill the static buffer `buf` from the n rows `v` of a (possibly ragged) chunk: rows [0, n) are v, the rest repeat
    its last row; a 1-row `v` fills every row."""
    if v.shape[0] == 1:
        buf.copy_(v.expand_as(buf))
        return
    buf[:n].copy_(v)
    if n < buf.shape[0]:
        buf[n:].copy_(v[-1:].expand(buf.shape[0] - n, *v.shape[1:]))


class GraphedChunk:
    """One fixed-shape render_rays(test_time=True) call captured in a HIP graph.

    Everything that varies between replays lives in static device buffers the captured kernels read: the ray matrix (or,
    for `CameraRays` input, the camera struct: the render kernel's prologue generates the rays from it -- C ABI
    nfl_pass_args::d_cam), `ts`, and the per-ray kwargs `a_embedded` / `t_embedded` / `view_dir`.  The packed weight
    streams are NOT part of the graph: `__call__` compares the fields' parameter keys (data pointers + version counters)
    with the ones the streams were packed from and re-packs eagerly before the replay when they moved (an optimizer
    step, load_state_dict), so a cached graph never renders stale weights."""

    PER_RAY = ("a_embedded", "t_embedded", "view_dir")

    def __init__(self, models, embeddings, chunk, device, N_samples, use_disp, N_importance, white_back, camera=False,
                 **kwargs):
        import weakref
        self.chunk, self.device = chunk, torch.device(device)
        self.camera = bool(camera)
        self.model_refs = {k: weakref.ref(m) for k, m in models.items()}
        self.rays = torch.zeros(chunk, 8, device=device)
        self.rays[:, 3:6] = torch.tensor([0.0, 0.0, -1.0], device=device)
        self.rays[:, 6], self.rays[:, 7] = 2.0, 6.0
        self.ts = torch.zeros(chunk, dtype=torch.long, device=device)
        self.kw_static = {}
        for k in self.PER_RAY:       # per-frame latent overrides (test_phototourism.ipynb cell 11), per-ray view directions
            if kwargs.get(k) is not None:
                v = kwargs[k].to(device=device, dtype=torch.float32)
                self.kw_static[k] = v[:1].expand(chunk, -1).contiguous().clone()
        other = {k: v for k, v in kwargs.items() if k not in self.PER_RAY}
        self.cam_rays = None
        if self.camera:             # a 1 x 1 frame as a placeholder; __call__ overwrites the device-side struct
            self.cam_rays = CameraRays(torch.eye(4)[:3], torch.eye(3), 1, 1, 2.0, 6.0, device, count=0)
            self.cam_rays.count, self.cam_rays.shape = chunk, (chunk, 8)
            self.cam_rays.to_device()

        def run():
            return render_rays(models, embeddings, self.cam_rays if self.camera else self.rays, self.ts, N_samples, use_disp,
                               0, 0, N_importance, chunk, white_back, True, **self.kw_static, **other)

        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side), torch.no_grad():      # warm-up: packs weights, sets kernel attributes
            run()
        torch.cuda.current_stream(device).wait_stream(side)
        n_xyz, n_dir = rnd._n_freqs(embeddings["xyz"]), rnd._n_freqs(embeddings["dir"])
        self.fields = [rnd._field(m, n_xyz, n_dir, self.device, pack=False) for m in models.values()]
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, **rnd._capture_mode()):
            self.out = run()

    def alive_for(self, models):
        """The captured launches read THESE models' packed streams: a cache hit must be for the same module objects."""
        return set(models) == set(self.model_refs) and all(self.model_refs[k]() is m for k, m in models.items())

    def __call__(self, rays, ts, **per_ray):
        n = rays.shape[0]
        if n > self.chunk:
            raise ValueError(f"GraphedChunk captured for {self.chunk} rays, got {n}")
        if isinstance(rays, CameraRays):
            if self.camera:          # 88 bytes to the device-side camera struct the captured prologue reads
                self.cam_rays.load(rays)
            else:                    # captured on a ray matrix: materialise the rows with nfl_gen_rays
                rays = frame_rays_of(rays)
        elif self.camera:
            raise ValueError("this GraphedChunk was captured for CameraRays input")
        if not isinstance(rays, CameraRays):
            _fill_padded(self.rays, rays, n)
        if ts is not None:
            _fill_padded(self.ts, ts, n)
        if set(per_ray) - set(self.kw_static):
            raise ValueError(f"per-ray kwargs {sorted(set(per_ray) - set(self.kw_static))} were not part of the capture")
        for k, buf in self.kw_static.items():
            if k not in per_ray:
                raise ValueError(f"this GraphedChunk was captured with `{k}`: pass it on every call")
            _fill_padded(buf, per_ray[k], n)
        # weights moved since the streams were packed (optimizer step, load_state_dict)?  re-pack eagerly: the captured
        # kernels read the same buffers
        rnd._pack_streams(self.fields, bwd=False, rays_grad=False)
        self.graph.replay()
        return {k: v[:n] for k, v in self.out.items()}


_GRAPH_CACHE = {}      # default cache of batched_inference(use_graph=True): one capture per distinct launch sequence


def _graph_key(models, embeddings, rays, chunk, N_samples, N_importance, use_disp, white_back, kwargs):
    """Everything that changes the captured launch sequence or the buffers it reads."""
    return (chunk, N_samples, N_importance, bool(use_disp), bool(white_back), str(rays.device), isinstance(rays, CameraRays),
            tuple(sorted((k, id(m)) for k, m in models.items())), tuple(sorted((k, id(e)) for k, e in embeddings.items())),
            tuple(sorted(k for k in kwargs if kwargs[k] is not None and k in GraphedChunk.PER_RAY)),
            tuple(sorted((k, repr(v)) for k, v in kwargs.items() if k not in GraphedChunk.PER_RAY)),
            rnd.get_precision())


@torch.no_grad()
def batched_inference(models, embeddings, rays, ts, N_samples, N_importance, use_disp=False, chunk=1024 * 128,
                      white_back=False, use_graph=False, _graph_cache=None, **kwargs):
    """Same arguments as the reference's eval.batched_inference (eval.py:80-88) plus `use_graph`.
    Returns a dict of GPU tensors covering all `rays`.  With `use_graph` the chunk is captured once per distinct call
    signature (models, kwargs present, `output_transient`, shapes, precision) and kept in `_graph_cache` (default: a
    module-level cache), so repeated calls replay instead of re-capturing."""
    results = {}
    runner = None
    if use_graph:
        key = _graph_key(models, embeddings, rays, chunk, N_samples, N_importance, use_disp, white_back, kwargs)
        cache = _graph_cache if _graph_cache is not None else _GRAPH_CACHE
        if key not in cache or not cache[key].alive_for(models):
            cache[key] = GraphedChunk(models, embeddings, chunk, rays.device, N_samples, use_disp, N_importance,
                                      white_back, camera=isinstance(rays, CameraRays), **kwargs)
        runner = cache[key]
    for _, _, r, t, per_ray in _chunks(rays, ts, chunk, {k: kwargs.get(k) for k in GraphedChunk.PER_RAY}):
        if runner is not None:
            out = {k: v.clone() for k, v in runner(r, t, **per_ray).items()}
        else:
            out = render_rays(models, embeddings, r, t, N_samples, use_disp, 0, 0, N_importance, chunk, white_back,
                              True, **{**kwargs, **per_ray})
        for k, v in out.items():
            results.setdefault(k, []).append(v)
    return {k: torch.cat(v, 0) for k, v in results.items()}


@torch.no_grad()
def clipped_inference(models, embeddings, rays, ts, grid, N_samples, N_importance, use_disp=False, chunk=1024 * 128,
                      white_back=False, **kwargs):
    """batched_inference with empty space skipped: `rays` ((B, 8) matrix) are clipped to the geometry.OccupancyGrid
    `grid` (geometry.clip_rays) -- or to the band round a surface of a raycast.MeshBand (its clip: the first hit of every
    ray against a mesh, -+ the band) -- the rays that meet an occupied cell are rendered between their tightened bounds with
    the same N_samples + N_importance, and the rows of the others are filled with what the compositing gives when every
    weight is zero: 1 (white_back) or 0 for every key containing `rgb`, the fine model's beta_min for `beta`, 0 for the
    rest.  `ts` and the per-ray kwargs (GraphedChunk.PER_RAY) with B rows follow their rays; a (1, C) one stays
    broadcast; the other kwargs go to batched_inference (use_graph among them).  Keys beginning with `_` are internal to
    the backward and are not returned.  When no ray hits, no render launch is made.

    ONE host synchronisation per call: the hit rays are compacted, in their original order, with torch.nonzero.
    Space outside the grid's box renders as empty."""
    from . import geometry
    from .raycast import MeshBand
    B = rays.shape[0]
    clipped, hit = grid.clip(rays) if isinstance(grid, MeshBand) else geometry.clip_rays(grid, rays)
    idx = torch.nonzero(hit).squeeze(1)                             # the host synchronisation
    n = idx.shape[0]
    kw = dict(kwargs)
    for k in GraphedChunk.PER_RAY:
        v = kwargs.get(k)
        if v is not None and v.shape[0] == B:
            kw[k] = v[idx]
    ts_hit = ts[idx] if ts is not None else None
    if n:
        res = batched_inference(models, embeddings, clipped[idx], ts_hit, N_samples, N_importance, use_disp, chunk,
                                white_back, **kw)
    else:           # render_rays returns empty tensors of the right shapes for no rays, before any launch
        for k in GraphedChunk.PER_RAY:
            if kw.get(k) is not None:
                kw[k] = kw[k].expand(0, -1) if kw[k].shape[0] == 1 else kw[k][:0]
        for k in ("use_graph", "_graph_cache"):
            kw.pop(k, None)
        res = render_rays(models, embeddings, clipped[:0], ts_hit, N_samples, use_disp, 0, 0, N_importance, chunk,
                          white_back, True, **kw)
    beta_min = float(getattr(models.get("fine", models["coarse"]), "beta_min", 0.0))
    out = {}
    for k, v in res.items():
        if k.startswith("_"):
            continue
        fill = (1.0 if white_back else 0.0) if "rgb" in k else beta_min if k == "beta" else 0.0
        full = torch.full((B,) + tuple(v.shape[1:]), fill, dtype=v.dtype, device=v.device)
        full[idx] = v
        out[k] = full
    return out


def frame_rays(c2w, K, H, W, near, far, device, start=0, count=None):
    """(count, 8) ray matrix [o, d, near, far] of pixels [start, start + count) of an H x W frame seen from pose `c2w`
    (3|4, 4) with intrinsics `K` (3, 3), generated on the device by nfl_gen_rays (reference datasets/ray_utils.py:5-55
    + the near/far columns the datasets append, e.g. blender.py:65-69).  Only the 12 pose floats cross the bus."""
    import ctypes as C

    from . import _lib
    count = H * W - start if count is None else int(count)
    if start < 0 or count < 0 or start + count > H * W:
        raise ValueError("pixel range outside the frame")
    c2w = torch.as_tensor(c2w, dtype=torch.float32).cpu()[:3, :4].contiguous()
    K = torch.as_tensor(K, dtype=torch.float32).cpu()
    pose = (C.c_float * 12)(*c2w.reshape(-1).tolist())
    dev = torch.device(device)
    rays = torch.empty(count, 8, dtype=torch.float32, device=dev)
    if count == 0:
        return rays
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nfl_gen_rays(pose, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), int(W),
                                           int(start), count, float(near), float(far), C.c_void_p(rays.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_gen_rays")
    return rays


def frame_rays_of(cam_rays):
    """The (count, 8) matrix a CameraRays stands for."""
    c = cam_rays.cam
    c2w = torch.tensor(list(c.c2w), dtype=torch.float32).reshape(3, 4)
    K = torch.tensor([[c.fx, 0.0, c.cx], [0.0, c.fy, c.cy], [0.0, 0.0, 1.0]])
    return frame_rays(c2w, K, cam_rays.H, cam_rays.W, c.near, c.far, cam_rays.device, cam_rays.start, cam_rays.count)


def fit_and_evaluate_halves(models, embeddings, c2w, K, H, W, near, far, rgb, N_samples=64, N_importance=64, n_iters=300,
                            lr=0.05, init=None, use_disp=False, white_back=False, chunk=1024 * 128, use_graph=False,
                            device="cuda:0", **kwargs):
    """The NeRF-W evaluation protocol for one image (H x W, pose `c2w`, intrinsics `K`, colours `rgb` (H, W, 3) or
    (H*W, 3)): fit its appearance code on the left half's rays (appearance.AppearanceFit, `n_iters` iterations of Adam
    at `lr`, starting from `init` (N_a,) or the mean of the table), render the right half with
    batched_inference(test_time, output_transient=False, a_embedded=code[None]) and return (code (N_a,), PSNR of the
    right half).  `barf_weights` / `current_epoch` (refine_pose fields) go to both the fit and the right-half render;
    `view_dir` is given for the whole image (H*W, 3) and split into the halves; any other kwarg (max_cache_bytes, ...)
    goes to AppearanceFit."""
    import math
    dev = torch.device(device)
    rays = frame_rays(c2w, K, H, W, near, far, dev)
    rgb = torch.as_tensor(rgb).to(dev, torch.float32).reshape(H * W, 3)
    render_kw = {k: kwargs.pop(k) for k in ("barf_weights", "current_epoch", "view_dir") if kwargs.get(k) is not None}
    if "view_dir" in render_kw:
        render_kw["view_dir"] = torch.as_tensor(render_kw["view_dir"]).to(dev, torch.float32).reshape(H * W, 3)
    code = _fit_left_half(models, embeddings, rays, rgb, H, W, N_samples, N_importance,
                          dict(kwargs, n_iters=n_iters, lr=lr, init=init), render_kw, use_disp=use_disp,
                          white_back=white_back, chunk=chunk, use_graph=use_graph)
    right = torch.arange(H * W, device=dev) % W >= W // 2
    if "view_dir" in render_kw:
        render_kw["view_dir"] = render_kw["view_dir"][right]
    with torch.no_grad():
        res = batched_inference(models, embeddings, rays[right], None, N_samples, N_importance, use_disp, chunk, white_back,
                                **render_kw)
    mse = ((res["rgb_fine"] - rgb[right]) ** 2).mean().item()
    return code, (-10.0 * math.log10(mse) if mse > 0 else float("inf"))


def _fit_left_half(models, embeddings, rays, rgbs, H, W, N_samples, N_importance, fit_kw, render_kw, *, use_disp,
                   white_back, chunk, use_graph):
    """Fit the appearance code of one H x W image (rays (H*W, 8), colours rgbs (H*W, 3)) on its left half, for the render
    that follows.  fit_kw: `n_iters` (default 300), `lr` (0.05), `init` ((N_a,); default the mean of the table) and any
    other AppearanceFit argument.  render_kw: the kwargs of that render: its `barf_weights` / `current_epoch` go to the
    fit as well, of its `view_dir` (H*W, 3) the fit takes the left half, and it GAINS output_transient=False and
    a_embedded=code[None].  Returns the code (N_a,); the fit's cache (512 B per padded sample) is free by then."""
    from .appearance import AppearanceFit
    dev = rays.device
    left = torch.arange(H * W, device=dev) % W < W // 2
    fit_kw = dict(fit_kw)
    n_iters, init = fit_kw.pop("n_iters", 300), fit_kw.pop("init", None)
    fit_kw.setdefault("lr", 0.05)
    fit_kw.update({k: render_kw[k] for k in ("barf_weights", "current_epoch") if render_kw.get(k) is not None})
    if render_kw.get("view_dir") is not None:
        fit_kw["view_dir"] = render_kw["view_dir"][left]
    rays_l = rays[left]
    fitter = AppearanceFit(models, embeddings, rays_l, rgbs[left], torch.zeros(rays_l.shape[0], dtype=torch.int64, device=dev),
                           N_samples, N_importance, use_disp=use_disp, white_back=white_back, chunk=chunk,
                           init=None if init is None else torch.as_tensor(init, dtype=torch.float32).reshape(1, -1), **fit_kw)
    code = fitter.fit(n_iters, use_graph=use_graph)[0].clone()
    render_kw.update(output_transient=False, a_embedded=code[None])
    return code


def evaluate_bank(models, embeddings, bank, N_samples, N_importance, *, images=None, ts=None, halves=False, fit=None,
                  clip=True, rank=0, world=1, use_graph=False, return_images=False, return_depth=False, poses=None,
                  **kwargs):
    """Score a held-out data.ImageBank on the device: PSNR, masked PSNR and SSIM per image (metrics.image_metrics in
    bank form), with one device-to-host copy after the last image and device memory that does not grow with the split.

    images: indices into the bank (default all); image k of them is scored into row k of one (n, 8) fp64 table
    (metrics.METRIC_COLUMNS) when k lies in parallel.shard_bounds(n, rank, world) -- the other rows stay zero, so one
    all_reduce(SUM) of `table` merges the ranks.  Each image is rendered from its record's camera (CameraRays: no rays
    are gathered or stored) by batched_inference (test_time); `kwargs` (use_disp, chunk, white_back -- default: the
    bank's --, barf_weights, ...) go there.
    ts: None renders image i with its record's id; an int, or one per entry of `images`, overrides it (the reference
    evaluates Blender val / test images with t = 0).  poses: (n, 3|4, 4) camera-to-world poses that replace the records'
    (RayTrainer.validate_bank: the learned ones).
    halves=True scores the right half only (region x0 = W // 2).  fit=dict(n_iters=..., lr=..., [init=..., other
    AppearanceFit arguments]) first fits the image's appearance code on its left half (appearance.AppearanceFit on the
    rays and colours ImageBank.gather gives for that image) and renders with a_embedded = that code, ts = None and
    output_transient=False: fit_and_evaluate_halves for a bank.
    clip: clamp the prediction to [0, 1] before scoring (eval.py:201 does, train.py:200 does not).

    Returns a dict: `table` (device), `psnr`, `psnr_valid`, `ssim` (fp64 host tensors, one per image, zero outside the
    shard) and `mean_psnr`, `mean_psnr_valid`, `mean_ssim` over this rank's shard; with fit, `codes` (n, N_a); with
    return_images / return_depth, `frames` / `depths`: lists of uint8 (h, w, 3) device tensors of the shard's images
    (the scored region; depths through metrics.depth_image)."""
    from . import metrics
    if bank.device is None:
        raise RuntimeError("evaluate_bank: the bank is not on a device (this build has no CPU path)")
    dev = bank.device
    images = list(range(bank.n_images)) if images is None else [int(i) for i in images]
    n = len(images)
    if any(not 0 <= i < bank.n_images for i in images):
        raise ValueError(f"images outside the bank's {bank.n_images}")
    if ts is not None and not isinstance(ts, int):
        ts = [int(t) for t in ts]
        if len(ts) != n:
            raise ValueError(f"ts has {len(ts)} entries for {n} images")
    if poses is not None:
        poses = torch.as_tensor(poses).detach().to("cpu", torch.float32)
        if poses.shape[0] != n:
            raise ValueError(f"poses has {poses.shape[0]} entries for {n} images")
    if fit is not None and not halves:
        raise ValueError("evaluate_bank: fit= fits on the left half, so it needs halves=True")
    kwargs.setdefault("white_back", bank.white_back)
    use_disp, chunk, white_back = kwargs.get("use_disp", False), kwargs.get("chunk", 1024 * 128), kwargs["white_back"]
    lo, hi = parallel.shard_bounds(n, rank, world)
    table = torch.zeros(n, len(metrics.METRIC_COLUMNS), dtype=torch.float64, device=dev)
    codes, frames, depths = None, [], []
    for k in range(lo, hi):
        i = images[k]
        rec = bank.host_table[i]
        H, W = int(rec["height"]), int(rec["width"])
        c2w = torch.from_numpy(rec["c2w"].reshape(3, 4).copy()) if poses is None else poses[k][:3, :4]
        K = torch.tensor([[float(rec["fx"]), 0.0, float(rec["cx"])], [0.0, float(rec["fy"]), float(rec["cy"])],
                          [0.0, 0.0, 1.0]])
        near, far = float(rec["near"]), float(rec["far"])
        region = (W // 2, W, 0, H) if halves else (0, W, 0, H)
        render_kw = dict(kwargs)
        t = None
        if fit is not None:
            if poses is None:
                rays, rgbs, _ = bank.frame(i)
            else:
                rays, rgbs = frame_rays(c2w, K, H, W, near, far, dev), bank.frame(i)[1]
            code = _fit_left_half(models, embeddings, rays, rgbs, H, W, N_samples, N_importance, fit, render_kw,
                                  use_disp=use_disp, white_back=white_back, chunk=chunk, use_graph=use_graph)
            del rays, rgbs
            if codes is None:
                codes = torch.zeros(n, code.shape[0], dtype=torch.float32, device=dev)
            codes[k] = code
        else:
            t_id = int(rec["id"]) if ts is None else (ts if isinstance(ts, int) else ts[k])
            t = torch.full((H * W,), t_id, dtype=torch.long, device=dev)
        cam = CameraRays(c2w, K, H, W, near, far, dev)
        res = batched_inference(models, embeddings, cam, t, N_samples, N_importance,
                                use_graph=use_graph and fit is None, **render_kw)
        tag = "fine" if "rgb_fine" in res else "coarse"
        out = metrics.image_metrics(res[f"rgb_{tag}"], H, W, bank=bank, image=i, region=region, clip=clip, table=table,
                                    slot=k, want_uint8=return_images)
        if return_images:
            frames.append(out[1])
        if return_depth:
            depths.append(metrics.depth_image(res[f"depth_{tag}"].contiguous(), H, W, region=region))
        del res, out
    host = table.cpu()                                              # the one device-to-host copy
    col = {name: host[:, j] for j, name in enumerate(metrics.METRIC_COLUMNS)}
    result = dict(table=table, first=lo, count=hi - lo, psnr=col["psnr"], psnr_valid=col["psnr_valid"], ssim=col["ssim"])
    for name in ("psnr", "psnr_valid", "ssim"):
        result[f"mean_{name}"] = float(col[name][lo:hi].mean()) if hi > lo else float("nan")
    if codes is not None:
        result["codes"] = codes
    if return_images:
        result["frames"] = frames
    if return_depth:
        result["depths"] = depths
    return result


def to_uint8(rgb):
    """clip to [0, 1], x 255, truncate -- the reference's image conversion (eval.py:201-203: np.clip(...), (img * 255)
    .astype(np.uint8)) -- on the device, so a frame leaves the GPU as 3 bytes per pixel instead of 12."""
    return (rgb.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def dolly_path(c2w0, n_frames=120, dx=0.03, dy=-0.1, dz=0.5):
    """Camera path of the reference's novel-view video (eval.py:169-183): `n_frames` copies of a training pose whose
    translation moves linearly by (dx, dy, dz) -- the reference hard-codes exactly this for brandenburg_gate (pose of
    image 1123, 30 * 4 frames, 0.03 / -0.1 / 0.5) and raises NotImplementedError for every other scene; here it is the
    path of any scene (configs[4], trevi_fountain: choose the start pose and the deltas).  Returns (n_frames, 3, 4)."""
    c2w0 = torch.as_tensor(c2w0, dtype=torch.float32)[:3, :4]
    poses = c2w0[None].repeat(n_frames, 1, 1)
    for axis, d in enumerate((dx, dy, dz)):
        poses[:, axis, 3] += torch.linspace(0, d, n_frames)
    return poses


def fov60_intrinsics(W, H):
    """The reference's test camera (eval.py:164-168): fov 60 degrees, principal point at the image centre."""
    import math
    f = W / 2 / math.tan(math.pi / 6)
    return torch.tensor([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])


@torch.no_grad()
def render_frame(models, embeddings, c2w, K, H, W, near, far, N_samples, N_importance, ts=None, use_disp=False,
                 chunk=1024 * 128, white_back=False, device="cuda:0", use_graph=False, _graph_cache=None, occupancy=None,
                 **kwargs):
    """One H x W frame from (pose, intrinsics): the rays are generated in the render kernel's prologue (CameraRays), the
    image is converted on the device.  Returns (uint8 (H, W, 3), dict of the float outputs).  `ts`: image id for the
    latent tables -- an int, a (H*W,) tensor, or None when `a_embedded` is given / the model has no latent inputs.
    `occupancy`: a geometry.OccupancyGrid, or a raycast.MeshBand (a surface and a band round it); the frame's rays are then a matrix (frame_rays: the bounds are per ray) and go
    through clipped_inference, which skips the pixels that see no occupied cell (one host synchronisation per frame)."""
    if occupancy is not None:
        rays = frame_rays(c2w, K, H, W, near, far, device)
        if isinstance(ts, int):
            ts = torch.full((H * W,), ts, dtype=torch.long, device=rays.device)
        res = clipped_inference(models, embeddings, rays, ts, occupancy, N_samples, N_importance, use_disp, chunk,
                                white_back, use_graph=use_graph, _graph_cache=_graph_cache, **kwargs)
        return to_uint8(res["rgb_fine" if "rgb_fine" in res else "rgb_coarse"]).view(H, W, 3), res
    cam = CameraRays(c2w, K, H, W, near, far, device)
    if isinstance(ts, int):
        ts = torch.full((H * W,), ts, dtype=torch.long, device=cam.device)
    res = batched_inference(models, embeddings, cam, ts, N_samples, N_importance, use_disp, chunk, white_back,
                            use_graph=use_graph, _graph_cache=_graph_cache, **kwargs)
    return to_uint8(res["rgb_fine" if "rgb_fine" in res else "rgb_coarse"]).view(H, W, 3), res


@torch.no_grad()
def render_video(models, embeddings, poses, K, H, W, near, far, N_samples, N_importance, rank=0, world=1, **kwargs):
    """Frames of a camera path, sharded over ranks with no collective: rank r renders the contiguous block
    parallel.shard_bounds(n_frames, r, world) and returns (first frame index, uint8 (n_local, H, W, 3)).  (The
    reference renders every frame on one GPU, eval.py:186-194.)"""
    lo, hi = parallel.shard_bounds(len(poses), rank, world)
    cache = kwargs.pop("_graph_cache", None)        # None: the module-level cache of batched_inference
    frames = [render_frame(models, embeddings, poses[i], K, H, W, near, far, N_samples, N_importance, _graph_cache=cache,
                           **kwargs)[0] for i in range(lo, hi)]
    dev = kwargs.get("device", "cuda:0")
    return lo, (torch.stack(frames) if frames else torch.empty(0, H, W, 3, dtype=torch.uint8, device=dev))


def render_mesh_video(mesh, poses, K, H, W, rank=0, world=1, **kwargs):
    """render_video for a mesh: the frames of a camera path through geometry.render_mesh (`kwargs`: colors, shade,
    background, texture), sharded over ranks with no collective.  Rank r renders the contiguous block
    parallel.shard_bounds(n_frames, r, world) and returns (first frame index, uint8 (n_local, H, W, 3)) on the mesh's
    device.  No host synchronisation when `poses` and `K` are tensors on that device."""
    from . import geometry
    lo, hi = parallel.shard_bounds(len(poses), rank, world)
    frames = [geometry.render_mesh(mesh, poses[i], K, H, W, **kwargs)["rgb"] for i in range(lo, hi)]
    dev = mesh["vertices"].device
    return lo, (torch.stack(frames) if frames else torch.empty(0, int(H), int(W), 3, dtype=torch.uint8, device=dev))


def evaluate_mesh(mesh, bank, *, colors=None, images=None, background=None, rank=0, world=1, return_images=False,
                  texture=None):
    """evaluate_bank for a coloured mesh: every selected image of a data.ImageBank (on the mesh's device) is rendered from
    its record's camera by geometry.render_mesh (`colors`: default the mesh's own; `texture`: an atlas, as render_mesh
    takes it, scores the textured render instead) and scored on the device against the
    bank's image, with one device-to-host copy after the last image.

    What is scored is the 8-bit frame, byte / 255 (what `frames` holds and a viewer sees; the photographs are 8-bit
    too), so a bank rendered from the mesh itself scores an error of exactly zero.  `psnr` and `ssim` are over the whole
    frame, the background included (`background`: 3 numbers; default white when bank.white_back, black otherwise);
    `psnr_valid` is over the pixels the mesh covers (metrics.image_metrics in tensor form, mask = covered).

    images: indices into the bank (default all); image k of them is scored into row k of one (n, 8) fp64 table
    (metrics.METRIC_COLUMNS) when k lies in parallel.shard_bounds(n, rank, world) -- the other rows stay zero, so one
    all_reduce(SUM) of `table` merges the ranks.  An image is at least 2 x 2 pixels (the SSIM border is a reflection).

    Returns the dict evaluate_bank returns: `table` (device), `psnr`, `psnr_valid`, `ssim` (fp64 host tensors, one per
    image, zero outside the shard), `mean_psnr`, `mean_psnr_valid`, `mean_ssim` over this rank's shard, `first`, `count`;
    with return_images, `frames`: a list of uint8 (h, w, 3) device tensors of the shard's images."""
    from . import geometry, metrics
    if bank.device is None:
        raise RuntimeError("evaluate_mesh: the bank is not on a device (this build has no CPU path)")
    dev = bank.device
    images = list(range(bank.n_images)) if images is None else [int(i) for i in images]
    n = len(images)
    if any(not 0 <= i < bank.n_images for i in images):
        raise ValueError(f"images outside the bank's {bank.n_images}")
    if background is None:
        background = (1.0, 1.0, 1.0) if bank.white_back else (0.0, 0.0, 0.0)
    lo, hi = parallel.shard_bounds(n, rank, world)
    table = torch.zeros(n, len(metrics.METRIC_COLUMNS), dtype=torch.float64, device=dev)
    frames = []
    for k in range(lo, hi):
        i = images[k]
        rec = bank.host_table[i]
        H, W = int(rec["height"]), int(rec["width"])
        out = geometry.render_mesh(mesh, bank=bank, image=i, colors=colors, background=background, texture=texture)
        # byte / 255.0f as the bank's own pixels are converted (nfl_pixel.h: a correctly rounded fp32 quotient).  Taken
        # through fp64: torch divides an fp32 tensor by a number by multiplying with its reciprocal, which is one ulp off
        # for some bytes; the fp64 quotient is within 2^-52 of k / 255 whichever way it is formed, and no k / 255 lies
        # within 2^-33 (relative) of a point where fp32 rounding changes, so rounding it once more gives the same bits.
        pred = (out["rgb"].reshape(H * W, 3).to(torch.float64) / 255.0).to(torch.float32)
        target = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
        bank.gather(int(rec["pix0"]), H * W, 0, out=(None, target, None))
        metrics.image_metrics(pred, H, W, target=target, mask=out["covered"].reshape(H * W), clip=False, table=table, slot=k)
        if return_images:
            frames.append(out["rgb"])
        del out, pred, target
    host = table.cpu()                                              # the one device-to-host copy
    col = {name: host[:, j] for j, name in enumerate(metrics.METRIC_COLUMNS)}
    result = dict(table=table, first=lo, count=hi - lo, psnr=col["psnr"], psnr_valid=col["psnr_valid"], ssim=col["ssim"])
    for name in ("psnr", "psnr_valid", "ssim"):
        result[f"mean_{name}"] = float(col[name][lo:hi].mean()) if hi > lo else float("nan")
    if return_images:
        result["frames"] = frames
    return result
