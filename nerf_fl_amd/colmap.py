"""Host reader of a Phototourism scene: COLMAP's binary sparse model and the split table.

read_phototourism restates what the reference's PhototourismDataset.read_meta does between the files on disk and its ray
buffers (datasets/phototourism.py:44-148), up to -- not including -- the depth bounds and the scene scaling, which need
the device (data.depth_bounds, data.ImageBank.from_phototourism).  It needs numpy alone: no device, pandas or Pillow.

The three binary files are parsed from one bytes buffer each with struct.unpack_from (COLMAP's documented layout,
little-endian, unaligned):
  cameras.bin    u64 n;  n x { i32 camera_id, i32 model_id, u64 width, u64 height, f64 params[n_params(model)] }
  images.bin     u64 n;  n x { i32 image_id, f64 qvec[4] (w, x, y, z), f64 tvec[3], i32 camera_id, name '\\0',
                               u64 n2d, n2d x { f64 x, f64 y, i64 point3D_id } }          (the 2D points are skipped)
  points3D.bin   u64 n;  n x { u64 point3D_id, f64 xyz[3], u8 rgb[3], f64 error, u64 track, track x { i32, i32 } }
"""
import csv
import dataclasses
import glob
import os
import struct

import numpy as np

# COLMAP's camera models: id -> (name, number of parameters).  Only PINHOLE (fx, fy, cx, cy) is supported.
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}


@dataclasses.dataclass
class PhototourismScene:
    """What read_phototourism returns; N images in TSV row order, everything on the host and UNSCALED.

    img_ids (N,) int64 COLMAP image ids; filenames: N names under dense/images/; splits: N strings of the TSV's `split`
    column; K (N, 3, 3) fp32 intrinsics at img_downscale; w2c (N, 4, 4) fp64 world-to-camera; poses (N, 3, 4) fp64
    camera-to-world in "right up back" axes; xyz_world (P, 3) fp64 in file order; img_ids_train / img_ids_test: lists."""
    root_dir: str
    scene_name: str
    img_downscale: int
    img_ids: np.ndarray
    filenames: list
    splits: list
    K: np.ndarray
    w2c: np.ndarray
    poses: np.ndarray
    xyz_world: np.ndarray
    img_ids_train: list
    img_ids_test: list


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def read_cameras_bin(path):
    """{camera_id: (model name, width, height, params fp64)} of a cameras.bin."""
    buf = _read(path)
    (n,), off = struct.unpack_from("<Q", buf, 0), 8
    cams = {}
    for _ in range(n):
        cam_id, model, width, height = struct.unpack_from("<iiQQ", buf, off)
        off += 24
        if model not in CAMERA_MODELS:
            raise ValueError(f"{path}: camera {cam_id} has unknown COLMAP camera model id {model}")
        name, n_params = CAMERA_MODELS[model]
        cams[cam_id] = (name, width, height, np.array(struct.unpack_from(f"<{n_params}d", buf, off)))
        off += 8 * n_params
    return cams


def read_images_bin(path):
    """{file name: (image_id, camera_id, qvec (4,), tvec (3,))} of an images.bin; the 2D observations are skipped."""
    buf = _read(path)
    (n,), off = struct.unpack_from("<Q", buf, 0), 8
    images = {}
    for _ in range(n):
        rec = struct.unpack_from("<i7di", buf, off)
        off += 64
        end = buf.index(b"\0", off)
        name = buf[off:end].decode("utf-8")
        (n2d,) = struct.unpack_from("<Q", buf, end + 1)
        off = end + 9 + 24 * n2d
        images[name] = (rec[0], rec[8], np.array(rec[1:5]), np.array(rec[5:8]))
    return images


def read_points3d_bin(path):
    """(P, 3) fp64 positions of a points3D.bin, in file order (the reference's dict keeps insertion order too,
    phototourism.py:123).  Records have variable length (their tracks), so they are walked; colours, errors and tracks
    are not decoded."""
    buf = _read(path)
    (n,), off = struct.unpack_from("<Q", buf, 0), 8
    xyz = np.empty((n, 3), dtype=np.float64)
    unpack_xyz, unpack_track = struct.Struct("<3d").unpack_from, struct.Struct("<Q").unpack_from
    for i in range(n):
        xyz[i] = unpack_xyz(buf, off + 8)
        off += 51 + 8 * unpack_track(buf, off + 43)[0]
    if off != len(buf):
        raise ValueError(f"{path}: {len(buf) - off} bytes left after {n} points")
    return xyz


def qvec_to_rotmat(q):
    """(N, 4) unit quaternions (w, x, y, z) -> (N, 3, 3) rotation matrices (COLMAP's Hamilton convention)."""
    w, x, y, z = np.asarray(q, dtype=np.float64).T
    return np.stack([
        np.stack([1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y], -1),
        np.stack([2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x], -1),
        np.stack([2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2], -1)], -2)


def read_phototourism(root_dir, img_downscale=1):
    """The scene under `root_dir` (a *.tsv beside dense/sparse/{cameras,images,points3D}.bin) as a PhototourismScene.

    - The first *.tsv (sorted by name) lists the images: rows whose `id` field is empty are dropped, and the column is
      not used otherwise (it is unreliable, phototourism.py:53-54): an image's id is the one images.bin gives its FILE
      NAME, in TSV row order; images the TSV does not name are ignored (:46-75).  A TSV file name images.bin does not
      hold raises KeyError.
    - Intrinsics come from the image's COLMAP camera (cameras may be shared): img_w, img_h = int(2 cx), int(2 cy); at
      downscale s the size is img_w // s, img_h // s, and fx, cx scale by the ratio of widths, fy, cy by the ratio of
      heights; stored as fp32 (:85-96).  A camera of another model than PINHOLE raises ValueError.
    - w2c = [[R(qvec), tvec], [0 0 0 1]]; poses = inv(w2c)[:, :3] in fp64 with columns 1 and 2 negated (:102-112).
    - xyz_world: every point of points3D.bin (:122-123).
    - The train / test id lists follow the TSV's `split` column, in TSV order (:143-148)."""
    s = int(img_downscale)
    if s < 1:
        raise ValueError("image can only be downsampled, please set img_downscale>=1!")
    tsvs = sorted(glob.glob(os.path.join(root_dir, "*.tsv")))
    if not tsvs:
        raise FileNotFoundError(f"no *.tsv in {root_dir}")
    with open(tsvs[0], newline="") as f:
        rows = [r for r in csv.DictReader(f, delimiter="\t") if (r.get("id") or "").strip() != ""]
    sparse = os.path.join(root_dir, "dense", "sparse")
    by_name = read_images_bin(os.path.join(sparse, "images.bin"))
    cams = read_cameras_bin(os.path.join(sparse, "cameras.bin"))
    filenames = [r["filename"] for r in rows]
    splits = [r["split"] for r in rows]
    recs = [by_name[name] for name in filenames]                          # KeyError: not in images.bin
    n = len(recs)
    img_ids = np.array([r[0] for r in recs], dtype=np.int64)

    K = np.zeros((n, 3, 3), dtype=np.float32)
    for i, (img_id, cam_id, _, _) in enumerate(recs):
        model, _, _, p = cams[cam_id]
        if model != "PINHOLE":
            raise ValueError(f"image {filenames[i]!r} (id {img_id}): camera {cam_id} has model {model}; only PINHOLE is "
                             "supported")
        img_w, img_h = int(p[2] * 2), int(p[3] * 2)
        img_w_, img_h_ = img_w // s, img_h // s
        K[i, 0, 0] = p[0] * img_w_ / img_w
        K[i, 1, 1] = p[1] * img_h_ / img_h
        K[i, 0, 2] = p[2] * img_w_ / img_w
        K[i, 1, 2] = p[3] * img_h_ / img_h
        K[i, 2, 2] = 1

    w2c = np.zeros((n, 4, 4), dtype=np.float64)
    w2c[:, :3, :3] = qvec_to_rotmat(np.stack([r[2] for r in recs]))
    w2c[:, :3, 3] = np.stack([r[3] for r in recs])
    w2c[:, 3, 3] = 1.0
    poses = np.linalg.inv(w2c)[:, :3]
    poses[..., 1:3] *= -1                                                 # "right down front" -> "right up back"

    return PhototourismScene(
        root_dir=root_dir, scene_name=os.path.basename(tsvs[0])[:-4], img_downscale=s, img_ids=img_ids,
        filenames=filenames, splits=splits, K=K, w2c=w2c, poses=poses,
        xyz_world=read_points3d_bin(os.path.join(sparse, "points3D.bin")),
        img_ids_train=[int(i) for i, sp in zip(img_ids, splits) if sp == "train"],
        img_ids_test=[int(i) for i, sp in zip(img_ids, splits) if sp == "test"])
