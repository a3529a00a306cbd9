"""NeRF-W appearance codes for images the fields were not trained on (test-time optimisation).

The NeRF-W paper evaluates Phototourism by fitting the appearance code of each test image on the left half of that image
and measuring PSNR on the right half; the reference only interpolates between existing codes.  `AppearanceFit` fits
codes with the fields frozen and deterministic sampling (perturb 0, noise 0, no transient head).  Then everything but the
colour branch is constant across iterations, and the code of image i enters the field in one linear place, the appearance
columns W_a of dir_encoding.0 (include/nerf_fl_amd.h, "appearance codes of unseen images"):

    construction   coarse pass, importance sampling, and ONE fine pass that also writes the pre-activation Z_s of
                   dir_encoding.0 with a zero appearance input (512 B per padded sample): C ABI nfl_appearance_cache
    step()         nfl_appearance_fit (stream Z, colour branch forward + backward, per-image reduction into the codes'
                   gradient, loss) + the one-launch Adam: three launches, no atomics, no memset / memcpy

instead of render_rays' two passes, two dgrad and two wgrad launches per iteration.
"""
import ctypes as C

import torch

from . import _lib
from . import rendering as rnd
from .eval import _chunks
from .train import Adam

__all__ = ["AppearanceFit"]

_F = 128            # output width of dir_encoding.0
_MAX_PAD = 256      # samples per ray the fit kernel holds (include/nerf_fl_amd.h: n_pad <= 256)


class AppearanceFit:
    """Fit the appearance codes of the images behind `rays` (R, 8) with colours `rgbs` (R, 3) to the MSE of the fine
    colour, the fields and embedding tables frozen.

    image_index: (R,) int64, the code row of every ray, 0 .. n_images - 1 in any order (n_images = init.shape[0] when
    `init` is given, else image_index.max() + 1).  init: (n_images, N_a) starting codes; default: every row the mean of
    embeddings['a'].weight.  The codes are an nn.Parameter (`codes`) stepped by train.Adam(lr, capturable=True).
    Pass-through kwargs as in render_rays: `view_dir` (R, 3), `z_fine` (R, N_samples + N_importance) injected fine depths,
    `barf_weights` / `current_epoch` for refine_pose fields.  `chunk` bounds the rays of one cache-building pass.
    The cache takes 512 B per ray and padded sample (N_samples + N_importance rounded up to 64): more than
    `max_cache_bytes` raises ValueError before anything is allocated."""

    def __init__(self, models, embeddings, rays, rgbs, image_index, N_samples, N_importance, use_disp=False,
                 white_back=False, init=None, lr=0.05, chunk=1024 * 128, max_cache_bytes=64 << 30, **kwargs):
        fine = models.get("fine")
        if N_importance is None or int(N_importance) <= 0 or fine is None:
            raise ValueError("AppearanceFit needs a fine pass (N_importance > 0 and models['fine'])")
        if not getattr(fine, "encode_appearance", False):
            raise ValueError("AppearanceFit needs a fine field with the appearance input (encode_appearance=True)")
        S, I = int(N_samples), int(N_importance)
        if S < 3:
            raise ValueError("N_samples must be >= 3 when N_importance > 0")
        F = S + I
        n_pad = (F + 63) // 64 * 64
        if n_pad > _MAX_PAD:
            raise ValueError(f"N_samples + N_importance = {F}: the fit kernel holds at most {_MAX_PAD} samples per ray")
        if rays.dim() != 2 or rays.shape[1] < 8:
            raise ValueError("rays must be (N_rays, 8): origin, direction, near, far")
        R = int(rays.shape[0])
        if R < 1:
            raise ValueError("no rays to fit on")
        cache_bytes = R * _F * n_pad * 4
        if cache_bytes > max_cache_bytes:
            raise ValueError(f"the appearance cache needs {cache_bytes} bytes ({R} rays x {n_pad} padded samples x 512 B), "
                             f"more than max_cache_bytes = {max_cache_bytes}")
        if tuple(rgbs.shape) != (R, 3):
            raise ValueError(f"rgbs must be ({R}, 3)")
        if tuple(image_index.shape) != (R,):
            raise ValueError(f"image_index must be ({R},)")
        dev = rays.device
        if not rays.is_cuda:
            raise RuntimeError("nerf_fl_amd.AppearanceFit: rays must be a ROCm device tensor (there is no CPU path)")
        n_a = int(fine.in_channels_a)
        idx = image_index.detach().to(device=dev, dtype=torch.int64)
        lo_i, hi_i = int(idx.min()), int(idx.max())
        n_images = int(init.shape[0]) if init is not None else hi_i + 1
        if lo_i < 0 or hi_i >= n_images:
            raise ValueError(f"image_index values must lie in [0, {n_images})")
        if init is not None and tuple(init.shape) != (n_images, n_a):
            raise ValueError(f"init must be (n_images, {n_a})")

        self.R, self.S, self.I, self.F, self.n_pad = R, S, I, F, n_pad
        self.n_images, self.n_a, self.device = n_images, n_a, dev
        self.white_back = bool(white_back)
        # rays grouped by image once: the fit kernel's work items are ray ranges of one image
        self.order = torch.sort(idx, stable=True)[1]
        counts = torch.bincount(idx, minlength=n_images).cpu().tolist()
        with torch.cuda.device(dev):
            self._build_items(counts)
            self._build_cache(models, embeddings, rays, use_disp, white_back, chunk, kwargs)
            self.target = rnd._f32c(rgbs.detach().to(dev, torch.float32), "rgbs").index_select(0, self.order).contiguous()
            with torch.no_grad():
                start = (init.detach().to(dev, torch.float32).clone() if init is not None
                         else embeddings["a"].weight.detach().to(dev, torch.float32).mean(0, keepdim=True).repeat(n_images, 1))
            self.codes = torch.nn.Parameter(start.contiguous())
            self.codes.grad = torch.zeros_like(self.codes)
            self.opt = Adam([self.codes], lr=lr, capturable=True)
            self.loss = torch.zeros((), dtype=torch.float32, device=dev)
            self.partials = torch.empty(_lib.lib().nfl_appfit_partials_floats(self.n_items), dtype=torch.float32, device=dev)
            # fp32 weights of the colour branch, ORIGINAL parameters (the kernel reads W_a from dir_encoding.0.weight)
            named = dict(fine.named_parameters())
            self._w_dir = rnd._f32c(named["dir_encoding.0.weight"], "dir_encoding.0.weight")
            self._w_rgb = rnd._f32c(named["static_rgb.0.weight"], "static_rgb.0.weight")
            self._b_rgb = rnd._f32c(named["static_rgb.0.bias"], "static_rgb.0.bias")
            cd = int(fine.in_channels_dir)
            if self._w_dir.shape != (_F, 256 + cd + n_a) or self._w_rgb.shape != (3, _F):
                raise ValueError("unexpected dir_encoding.0 / static_rgb.0 shapes")
            self.col_a = 256 + cd
        self._graph = None

    # ---- construction ------------------------------------------------------------------------------------------------
    def _build_items(self, counts):
        """Work items of the fit kernel: (image, first ray, end ray) ranges in the sorted order, sized so that a launch has
        about 2048 wavefronts; the items of image i are [image_items[i], image_items[i + 1])."""
        rpi = max(1, -(-self.R // 2048))
        items, image_items, r = [], [0], 0
        for i, n in enumerate(counts):
            for a in range(r, r + n, rpi):
                items.append((i, a, min(a + rpi, r + n)))
            r += n
            image_items.append(len(items))
        self.n_items = len(items)
        self.items = torch.tensor(items, dtype=torch.int32).reshape(-1, 3).to(self.device)
        self.image_items = torch.tensor(image_items, dtype=torch.int32).to(self.device)

    @torch.no_grad()
    def _build_cache(self, models, embeddings, rays, use_disp, white_back, chunk, kwargs):
        R, S, I, F, dev = self.R, self.S, self.I, self.F, self.device
        rays_s = rnd._f32c(rays[:, :8], "rays").index_select(0, self.order).contiguous()
        n_xyz, n_dir = rnd._n_freqs(embeddings["xyz"]), rnd._n_freqs(embeddings["dir"])
        f16x3 = _lib.NFL_PREC_F16X3          # the cache is fp32-class whatever set_precision() says
        f_c = rnd._field(models["coarse"], n_xyz, n_dir, dev, pack=False, prec=f16x3)
        f_f = rnd._field(models["fine"], n_xyz, n_dir, dev, pack=False, prec=f16x3)
        rnd._pack_streams([f_c, f_f])
        if kwargs.get("barf_weights") is not None:      # as render_rays takes them, but from any device or dtype
            kwargs = dict(kwargs, barf_weights=tuple(rnd._f32c(w.detach().to(dev, torch.float32), f"barf_weights[{k}]")
                                                     for k, w in enumerate(kwargs["barf_weights"])))
        pe_w_xyz, pe_w_dir = rnd._pe_weights(models, embeddings, kwargs, dev)
        view_dir = kwargs.get("view_dir")
        if view_dir is not None:
            view_dir = rnd._f32c(view_dir.to(dev), "view_dir", (R, 3)).index_select(0, self.order).contiguous()
        z_in = kwargs.get("z_fine")
        if z_in is not None:
            z_in = rnd._f32c(z_in.to(dev), "z_fine", (R, F)).index_select(0, self.order).contiguous()
        self.zcache = torch.empty(R, _F, self.n_pad, dtype=torch.float32, device=dev)
        self.weights = torch.empty(R, F, dtype=torch.float32, device=dev)
        self.opacity = torch.empty(R, dtype=torch.float32, device=dev)
        self.z_sorted = torch.empty(R, F, dtype=torch.float32, device=dev)
        zeros_a = torch.zeros(min(chunk, R), self.n_a, dtype=torch.float32, device=dev)
        for lo, hi, r, _, kw in _chunks(rays_s, None, chunk, dict(view_dir=view_dir, z_fine=z_in)):
            vd = kw.get("view_dir")
            if z_in is not None:
                self.z_sorted[lo:hi] = kw["z_fine"]
            else:
                oc = rnd._run_pass(f_c, r, S, lin=rnd._linspace(S, dev), use_disp=use_disp, view_dir=vd, sigma_only=True,
                                   white_back=white_back, want_z=True, pe_w_xyz=pe_w_xyz, pe_w_dir=pe_w_dir)
                _lib.check(_lib.lib().nfl_sample_pdf(rnd._ptr(oc["z"]), rnd._ptr(oc["weights"]), C.c_void_p(0),
                                                     rnd._ptr(rnd._linspace(I, dev)), hi - lo, S, I,
                                                     rnd._ptr(self.z_sorted[lo:hi]), C.c_void_p(0), rnd._stream()),
                           "nfl_sample_pdf")
            of = rnd._run_pass(f_f, r, F, z=self.z_sorted[lo:hi], a_emb=zeros_a[:hi - lo], view_dir=vd, white_back=white_back,
                               want_rgb=False, pe_w_xyz=pe_w_xyz, pe_w_dir=pe_w_dir, zcache=self.zcache[lo:hi])
            self.weights[lo:hi] = of["weights"]
            self.opacity[lo:hi] = of["opacity"]

    # ---- the fit -----------------------------------------------------------------------------------------------------
    def _launch(self, grad, loss, rgb=None):
        a = _lib.AppFitArgs()
        a.d_zcache, a.d_weights, a.d_opacity = rnd._ptr(self.zcache), rnd._ptr(self.weights), rnd._ptr(self.opacity)
        a.d_target, a.d_items, a.d_image_items = rnd._ptr(self.target), rnd._ptr(self.items), rnd._ptr(self.image_items)
        a.d_codes, a.d_w_dir = rnd._ptr(self.codes), rnd._ptr(self._w_dir)
        a.d_w_rgb, a.d_b_rgb = rnd._ptr(self._w_rgb), rnd._ptr(self._b_rgb)
        a.n_rays, a.n_samples, a.n_pad, a.n_items = self.R, self.F, self.n_pad, self.n_items
        a.n_images, a.n_a, a.ld_dir, a.col_a = self.n_images, self.n_a, self._w_dir.shape[1], self.col_a
        a.white_back, a.reserved = int(self.white_back), 0
        a.d_partials, a.d_grad, a.d_loss, a.d_rgb = rnd._ptr(self.partials), rnd._ptr(grad), rnd._ptr(loss), rnd._ptr(rgb)
        _lib.check(_lib.lib().nfl_appearance_fit(C.byref(a), rnd._stream()), "nfl_appearance_fit")

    def _iteration(self):
        self._launch(self.codes.grad, self.loss)
        self.opt.step()

    def step(self):
        """One iteration (gradient of the MSE at the current codes, then the Adam update).  Returns the device scalar
        loss at the codes BEFORE the update (overwritten by the next iteration)."""
        with torch.cuda.device(self.device):
            self._iteration()
        return self.loss

    def fit(self, n_iters, use_graph=False):
        """`n_iters` iterations; returns the codes (n_images, N_a).  use_graph=True captures one iteration (three kernel
        launches on one stream) and replays it: the same bits as eager iterations."""
        n_iters = int(n_iters)
        with torch.cuda.device(self.device):
            if not use_graph:
                for _ in range(n_iters):
                    self._iteration()
                return self.codes.detach()
            done = 0
            if self._graph is None:
                if n_iters == 0:
                    return self.codes.detach()
                self._iteration()                # the optimiser state and its device-side step exist before capture
                done = 1
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph(keep_graph=True)     # kept after instantiation, so that its nodes can be inspected
                with torch.cuda.graph(g, **rnd._capture_mode()):
                    self._iteration()
                g.instantiate()
                self._graph = g
            self.opt.sync_hyper()
            for _ in range(n_iters - done):
                self._graph.replay()
                self.opt.note_replay()
        return self.codes.detach()

    @torch.no_grad()
    def render(self):
        """rgb_fine (R, 3) of the cached rays, in the caller's ray order, under the current codes."""
        with torch.cuda.device(self.device):
            rgb = torch.empty(self.R, 3, dtype=torch.float32, device=self.device)
            grad = torch.empty_like(self.codes)
            loss = torch.empty((), dtype=torch.float32, device=self.device)
            self._launch(grad, loss, rgb)
            out = torch.empty_like(rgb)
            out[self.order] = rgb
        return out

    @property
    def z_fine(self):
        """The fine depths (R, N_samples + N_importance) the cache was built from, in the caller's ray order."""
        out = torch.empty_like(self.z_sorted)
        out[self.order] = self.z_sorted
        return out
