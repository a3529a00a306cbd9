"""Training data kept on the device as uint8 images: ImageBank.

The reference's datasets build `all_rays` / `all_rgbs` (datasets/blender.py:73-101, datasets/phototourism.py:150-183):
32 B of ray, 12 B of colour and 8 B of image id per pixel, for what the image holds in 3 or 4 bytes.  The ray of a pixel
depends only on its image's pose and intrinsics, so an ImageBank keeps the packed uint8 pixels and one record per image
on the device, and one HIP kernel (nfl_gather_batch, csrc/nfl_gather.hip) writes a training batch -- rays, colours and
image ids of a range of a keyed, computed permutation of all pixels -- straight into the buffers a step reads.

There is no CPU path: a bank without a device holds its host arrays (for inspection and tests) and cannot gather.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _lib
from .colmap import read_phototourism

# one record per image: numpy mirror of nfl_image_rec (include/nerf_fl_amd.h)
RECORD = np.dtype([("pix0", "<i8"), ("byte0", "<i8"), ("width", "<i4"), ("height", "<i4"), ("channels", "<i4"),
                   ("id", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("near", "<f4"),
                   ("far", "<f4"), ("c2w", "<f4", (12,))])
assert RECORD.itemsize == C.sizeof(_lib.ImageRec)
LAYOUTS = {"world": (_lib.NFL_LAYOUT_WORLD, 8), "camera": (_lib.NFL_LAYOUT_CAMERA, 5)}
_M64 = (1 << 64) - 1


def splitmix64(state):
    """One splitmix64 output from `state` (the stream nfl_gather_batch draws its round keys from)."""
    z = (state + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def epoch_key(seed, epoch):
    """The permutation key of epoch `epoch` of a run seeded `seed`: a function of the two alone, so every rank computes
    the same order and a resumed run continues it.  Never 0 (0 is the identity order)."""
    return splitmix64((int(seed) * 1000003 + int(epoch)) & _M64) or 1


def batch_range(step, rank, world, batch_size):
    """Permuted positions [start, start + batch_size) of step `step` on rank `rank` of `world`: the ranks' batches of a
    step are consecutive, so all batches of an epoch are disjoint (DistributedSampler semantics)."""
    return (int(step) * int(world) + int(rank)) * int(batch_size)


def _add_perturbation(img, perturbation, seed):
    """datasets/blender.py:11-29 restated as written (the uint8 cast of all four channels included: it can lower alpha
    by one code value)."""
    from PIL import Image, ImageDraw
    if "color" in perturbation:
        np.random.seed(seed)
        img_np = np.array(img) / 255.0
        s = np.random.uniform(0.8, 1.2, size=3)
        b = np.random.uniform(-0.2, 0.2, size=3)
        img_np[..., :3] = np.clip(s * img_np[..., :3] + b, 0, 1)
        img = Image.fromarray((255 * img_np).astype(np.uint8))
    if "occ" in perturbation:
        draw = ImageDraw.Draw(img)
        np.random.seed(seed)
        left = np.random.randint(200, 400)
        top = np.random.randint(200, 400)
        for i in range(10):
            np.random.seed(10 * seed + i)
            random_color = tuple(np.random.choice(range(256), 3))
            draw.rectangle(((left + 20 * i, top), (left + 20 * (i + 1), top + 200)), fill=random_color)
    return img


def depth_bounds(xyz, w2c, q=(0.001, 0.999), device=None):
    """(near, far, count) per image: the q[0] and q[1] quantiles (numpy's default `linear` definition, in fp64) of the
    depths of the points `xyz` (P, 3) that lie in front of each camera `w2c` (N, 3|4, 4) world-to-camera, and how many
    do -- the reference's loop of phototourism.py:127-131 as one launch of nfl_depth_bounds (csrc/nfl_bounds.hip), which
    builds no (N, P) intermediate.  near, far: (N,) fp64 device tensors (two rows of one (2, N) tensor: `near._base`
    copies to the host in one go); count: (N,) int32.  An image with nothing in front of it has count 0 and NaN bounds.
    Stream-ordered; nothing is synchronised.  Inputs may be numpy arrays or tensors; they are converted to fp64 on
    `device` (default: the device of `xyz` if it is a device tensor)."""
    if device is None and torch.is_tensor(xyz) and xyz.is_cuda:
        device = xyz.device
    dev = torch.device(device) if device is not None else None
    if dev is None or dev.type != "cuda":
        raise RuntimeError("nerf_fl_amd.data.depth_bounds needs a ROCm device (this build has no CPU path)")
    xyz = torch.as_tensor(xyz).to(device=dev, dtype=torch.float64).contiguous()
    w2c = torch.as_tensor(w2c).to(device=dev, dtype=torch.float64)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
        raise ValueError(f"xyz must be (P, 3) with P >= 1, got {tuple(xyz.shape)}")
    if w2c.dim() != 3 or w2c.shape[0] < 1 or w2c.shape[1] not in (3, 4) or w2c.shape[2] != 4:
        raise ValueError(f"w2c must be (N, 3|4, 4) with N >= 1, got {tuple(w2c.shape)}")
    q_lo, q_hi = float(q[0]), float(q[1])
    if not (0.0 <= q_lo <= 1.0 and 0.0 <= q_hi <= 1.0):
        raise ValueError(f"quantiles must lie in [0, 1], got {q}")
    n = w2c.shape[0]
    row = w2c[:, 2, :].contiguous()                      # the depth needs the third row alone
    bounds = torch.empty(2, n, dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    a = _lib.BoundsArgs(C.c_void_p(xyz.data_ptr()), C.c_void_p(row.data_ptr()), xyz.shape[0], n, q_lo, q_hi,
                        C.c_void_p(bounds.data_ptr()), C.c_void_p(count.data_ptr()))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nfl_depth_bounds(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "nfl_depth_bounds")
    return bounds[0], bounds[1], count


def scene_bounds(scene, device):
    """Unscaled (near, far), two (N,) fp64 host arrays, of every image of a colmap.PhototourismScene: depth_bounds at
    the reference's percentiles 0.1 and 99.9 (phototourism.py:130-131) and ONE copy of 2 N doubles to the host.  An
    image with no point in front of it raises ValueError naming it."""
    near, _, _ = depth_bounds(scene.xyz_world, scene.w2c, q=(0.1 / 100, 99.9 / 100), device=device)
    both = near._base.cpu().numpy()
    bad = np.flatnonzero(np.isnan(both).any(0))
    if len(bad):
        i = int(bad[0])
        raise ValueError(f"image {scene.filenames[i]!r} (id {int(scene.img_ids[i])}) has no sparse point in front of it: "
                         "no depth bounds")
    return both[0], both[1]


class ImageBank:
    """uint8 images with their cameras, packed for nfl_gather_batch.

    images: list of uint8 (H, W, 3) or (H, W, 4) arrays (all RGB or all RGBA; sizes may differ).
    c2w: (N, 3|4, 4) camera-to-world poses.  K: (3, 3) or (N, 3, 3) intrinsics.  near / far: scalars or one per image.
    ids: the image ids written to `ts` (default 0 .. N-1).  Everything is rounded to fp32 once, here, as the reference's
    fp32 tensor arithmetic rounds its fp64 intrinsics and bounds.
    device: None keeps the host arrays only (`host_pixels`, `host_table`); otherwise they are uploaded (to()).

    n_images, n_pixels; nbytes = bytes held on the device (pixels + table); white_back = True iff RGBA (the colours are
    then blended onto white, datasets/blender.py:89)."""

    def __init__(self, images, c2w, K, near, far, ids=None, device=None):
        n = len(images)
        if n < 1:
            raise ValueError("ImageBank needs at least one image")
        c2w = np.asarray(torch.as_tensor(c2w).detach().cpu().numpy() if torch.is_tensor(c2w) else c2w, dtype=np.float64)
        if c2w.ndim != 3 or c2w.shape[0] != n or c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4:
            raise ValueError(f"c2w must be ({n}, 3|4, 4), got {c2w.shape}")
        K = np.asarray(K.detach().cpu().numpy() if torch.is_tensor(K) else K, dtype=np.float64)
        if K.shape == (3, 3):
            K = np.broadcast_to(K, (n, 3, 3))
        if K.shape != (n, 3, 3):
            raise ValueError(f"K must be (3, 3) or ({n}, 3, 3), got {K.shape}")
        near = np.broadcast_to(np.asarray(near, dtype=np.float64).reshape(-1), (n,))
        far = np.broadcast_to(np.asarray(far, dtype=np.float64).reshape(-1), (n,))
        ids = np.arange(n) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
        if ids.shape != (n,) or ids.min() < 0 or ids.max() >= 2 ** 31:
            raise ValueError(f"ids must be {n} integers in [0, 2^31)")
        table = np.zeros(n, dtype=RECORD)
        pix = byte = 0
        for i, im in enumerate(images):
            im = np.asarray(im)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] not in (3, 4) or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError(f"image {i}: expected uint8 (H, W, 3|4), got {im.dtype} {im.shape}")
            if im.shape[2] != np.asarray(images[0]).shape[2]:
                raise ValueError("ImageBank: all images RGB or all RGBA")
            table[i]["pix0"], table[i]["byte0"] = pix, byte
            table[i]["height"], table[i]["width"], table[i]["channels"] = im.shape
            pix += im.shape[0] * im.shape[1]
            byte += im.size
        if pix >= 1 << 40:
            raise ValueError("ImageBank holds fewer than 2^40 pixels")
        if K[:, 0, 0].min() == 0 or K[:, 1, 1].min() == 0:
            raise ValueError("K: zero focal length")
        table["id"] = ids
        table["fx"], table["fy"], table["cx"], table["cy"] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
        table["near"], table["far"] = near, far
        table["c2w"] = c2w[:, :3, :4].reshape(n, 12)
        self.host_table = table
        self.host_pixels = np.concatenate([np.asarray(im).reshape(-1) for im in images])
        self.n_images, self.n_pixels = n, int(pix)
        self.channels = int(table[0]["channels"])
        self.white_back = self.channels == 4
        self.device = self.pixels = self.table = None
        if device is not None:
            self.to(device)

    def to(self, device):
        """Upload pixels and table to `device`; the host copy of the pixels is dropped (the table stays)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("nerf_fl_amd.data.ImageBank needs a ROCm device (this build has no CPU path)")
        if self.pixels is None:
            self.pixels = torch.from_numpy(self.host_pixels).to(dev)
            self.host_pixels = None
        else:
            self.pixels = self.pixels.to(dev)
        self.table = torch.from_numpy(self.host_table.view(np.uint8).reshape(-1)).to(dev)
        self.device = dev
        return self

    @property
    def nbytes(self):
        return self.n_pixels * self.channels + self.n_images * RECORD.itemsize

    @classmethod
    def from_blender(cls, root_dir, split="train", img_wh=(800, 800), perturbation=(), device=None):
        """The training images of a Blender-format scene as the reference's BlenderDataset reads them
        (datasets/blender.py:49-99): transforms_{split}.json, focal from camera_angle_x at 800 px scaled to img_wh,
        principal point (w/2, h/2), near 2, far 6, id = frame index t, every frame except the first perturbed with seed
        t ('color', 'occ'; before the resize), LANCZOS resize to img_wh.  Needs Pillow."""
        from PIL import Image
        if img_wh[0] != img_wh[1]:
            raise ValueError("image width must equal image height!")
        if not set(perturbation).issubset({"color", "occ"}):
            raise ValueError('Only "color" and "occ" perturbations are supported!')
        with open(os.path.join(root_dir, f"transforms_{split.split('_')[-1]}.json"), "r") as f:
            meta = json.load(f)
        w, h = img_wh
        focal = 0.5 * 800 / np.tan(0.5 * meta["camera_angle_x"])
        focal *= img_wh[0] / 800
        K = np.eye(3)
        K[0, 0] = K[1, 1] = focal
        K[0, 2] = w / 2
        K[1, 2] = h / 2
        images, poses = [], []
        for t, frame in enumerate(meta["frames"]):
            poses.append(np.array(frame["transform_matrix"])[:3, :4])
            img = Image.open(os.path.join(root_dir, f"{frame['file_path']}.png"))
            if t != 0:
                img = _add_perturbation(img, perturbation, t)
            img = img.resize(tuple(img_wh), Image.LANCZOS)
            images.append(np.array(img))
        return cls(images, np.stack(poses), K, 2.0, 6.0, ids=np.arange(len(images)), device=device)

    @classmethod
    def from_phototourism(cls, root_dir, split="train", img_downscale=1, device=None):
        """The `split` ("train" or "test") images of a Phototourism scene as the reference's PhototourismDataset
        prepares them (datasets/phototourism.py:44-183): colmap.read_phototourism; near / far of EVERY image of the
        TSV, train and test together, from the sparse points on the device (scene_bounds); scale_factor =
        float32(largest far) / 5, which divides the pose translations, near, far and xyz_world (:133-140); the split's
        images from dense/images/ as RGB, LANCZOS-resized to (w // s, h // s) of the image's OWN size for
        img_downscale s > 1 (:162-168); ids = the COLMAP image ids.  "test" is the held-out list eval.evaluate_bank(
        halves=True) and AppearanceFit are for.  The reference's forced downscale of its `val` split is an
        out-of-memory workaround and is not reproduced.

        Beyond an ImageBank's fields the bank carries scale_factor (np.float32), xyz_world (scaled, host, fp64),
        img_ids (this split's ids in order) and max_id (over both splits: N_vocab must exceed it).  Needs a device (the
        bounds run there) and Pillow."""
        from PIL import Image
        if split not in ("train", "test"):
            raise ValueError(f'split must be "train" or "test", got {split!r}')
        if device is None:
            raise RuntimeError("ImageBank.from_phototourism needs a ROCm device (this build has no CPU path)")
        scene = read_phototourism(root_dir, img_downscale)
        near, far = scene_bounds(scene, device)
        scale_factor = np.float32(far.max()) / np.float32(5)              # so that the max far is scaled to 5
        poses = scene.poses.copy()
        poses[..., 3] /= scale_factor
        near, far = near / scale_factor, far / scale_factor
        want = scene.img_ids_train if split == "train" else scene.img_ids_test
        rows = [i for i, sp in enumerate(scene.splits) if sp == split]
        assert [int(scene.img_ids[i]) for i in rows] == want
        if not rows:
            raise ValueError(f"{root_dir}: the TSV lists no {split} image")
        s = scene.img_downscale
        images = []
        for i in rows:
            img = Image.open(os.path.join(root_dir, "dense", "images", scene.filenames[i])).convert("RGB")
            if s > 1:
                img_w, img_h = img.size
                img = img.resize((img_w // s, img_h // s), Image.LANCZOS)
            images.append(np.array(img))
        bank = cls(images, poses[rows], scene.K[rows], near[rows], far[rows], ids=scene.img_ids[rows], device=device)
        bank.scale_factor = scale_factor
        bank.xyz_world = scene.xyz_world / scale_factor
        bank.img_ids = list(want)
        bank.max_id = int(scene.img_ids.max())
        return bank

    # ---- batches ------------------------------------------------------------------------------------------------
    def gather(self, start, count, key=0, layout="world", out=None):
        """(rays, rgbs, ts) of permuted positions [start, start + count): position p is flat pixel p for key 0 and
        perm_{key, n_pixels}(p) otherwise (include/nerf_fl_amd.h).  rays: (count, 8) world rays [o, d, near, far], or with
        layout="camera" (count, 5) [camera-frame direction, near, far], what RayTrainer(refine_pose=True) takes; rgbs
        (count, 3) fp32; ts (count,) int64 image ids.  out: a triple of existing contiguous device buffers with at
        least `count` rows, written in place (an entry may be None: that output is skipped and returned as None)."""
        if self.device is None:
            raise RuntimeError("ImageBank.gather: the bank is not on a device (this build has no CPU path)")
        code, width = LAYOUTS[layout]
        start, count, key = int(start), int(count), int(key)
        if start < 0 or count < 0 or start + count > self.n_pixels:
            raise ValueError(f"positions [{start}, {start + count}) outside the bank's {self.n_pixels} pixels")
        if not 0 <= key <= _M64:
            raise ValueError("key must fit 64 bits")
        dev = self.device
        if out is None:
            out = (torch.empty(count, width, dtype=torch.float32, device=dev),
                   torch.empty(count, 3, dtype=torch.float32, device=dev),
                   torch.empty(count, dtype=torch.int64, device=dev))
        else:
            for t, shape, dtype in zip(out, ((width,), (3,), ()), (torch.float32, torch.float32, torch.int64)):
                if t is not None and (t.device != dev or t.dtype != dtype or not t.is_contiguous() or t.dim() != 1 + len(shape)
                                      or t.shape[0] < count or tuple(t.shape[1:]) != shape):
                    raise ValueError(f"ImageBank.gather: out buffer {tuple(t.shape)} {t.dtype} does not hold "
                                     f"{(count,) + shape} {dtype} on {dev}")
        rays, rgbs, ts = out
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
        a = _lib.GatherArgs(C.c_void_p(self.pixels.data_ptr()), C.c_void_p(self.table.data_ptr()), self.n_images, code,
                            self.n_pixels, start, key, count, 0, ptr(rays), ptr(ts), ptr(rgbs))
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().nfl_gather_batch(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "nfl_gather_batch")
        return rays, rgbs, ts

    def materialise(self, layout="world"):
        """gather(0, n_pixels): the reference's all_rays[:, :8], all_rgbs and ts (52 B per pixel: small scenes, tests)."""
        return self.gather(0, self.n_pixels, 0, layout)

    def frame(self, i, layout="world"):
        """(rays, rgbs, ts) of image `i` alone, in pixel order: what RayTrainer.validate and eval.batched_inference take."""
        rec = self.host_table[int(i)]
        return self.gather(int(rec["pix0"]), int(rec["width"]) * int(rec["height"]), 0, layout)
