"""What the GPU tests of the geometry package share (test_mesh, test_simplify, test_meshsmooth, test_meshcolor,
test_meshrender and test_atlas `_gpu.py`): uploads and raw pointers for the C ABI, sentinel frames, the two bit
comparisons, and the ball, frames and cameras several of them look at.  A plain module, imported as gpu_util.py is."""
import ctypes as C

import numpy as np
import torch

import meshcolor_ref as mref
from gpu_util import DEV
from nerf_fl_amd import geometry

F = np.float32
PAD = 64                    # words of sentinel before and behind a framed buffer


# ---- the C ABI by hand

def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def to_dev(mesh):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in mesh.items()}


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def framed(n, tail, fill, dtype):
    return torch.full((n + 2 * PAD,) + tail, fill, dtype=dtype, device=DEV)


def unframe(buf, n, sentinel, what):
    h = buf.cpu().numpy()
    assert (h[:PAD] == sentinel).all() and (h[PAD + n:] == sentinel).all(), what
    return h[PAD:PAD + n]


# ---- equality on the bits.  Two pairs, because they do different things: `bits` / `same` take ONE tensor or array, fetch it
# from the device and insist on equal dtype and shape (the mesh, simplify and smoothing tests); `field_bits` / `same_fields`
# take host arrays only and walk the keys two DICTS share, reporting the first words that differ (the render and atlas
# tests).  test_simplify_cpu.py and test_occupancy_gpu.py have `_bits` of their own that are neither.

def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(got, exp, what):
    g, e = bits(got), bits(exp)
    assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), what


def field_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_fields(got, exp, what):
    for k in exp:
        if k in got:
            bad = field_bits(got[k]) != field_bits(exp[k])
            assert not bad.any(), (what, k, int(bad.sum()), "differ", got[k][bad][:4], exp[k][bad][:4])


# ---- what the image tests look at.  The banks themselves stay with their files: test_meshcolor_gpu.py draws random images
# of a channel count, test_meshrender_gpu.py takes the images it is given.

EYES = [(3, 0, 0), (0, 3, 0), (0, 0, 3), (-3, 0, 0), (0, -3, 0), (0, 0, -3)]


def frame(W, H):
    if (W, H) == (65, 33):
        return mref.camera(**mref.SOUP_CAMERA)
    return mref.camera(W, H, 0.6 * W + 3.0, 0.6 * W + 3.0, W / 2 - 0.25, H / 2 - 0.2)


def ball_mesh(radius=0.8, n=17):
    c = torch.linspace(-1.0, 1.0, n, device=DEV, dtype=torch.float64)
    lat = (radius - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()
    return geometry.extract_surface(lat, 0.0, (-1.0,) * 3, (1.0,) * 3)


def pose(eye):
    return mref.look_at(eye, up=(0.0, 0.0, 1.0) if eye[2] == 0 else (0.0, 1.0, 0.0))


def intrinsics(w, h):
    return np.array([[50.0, 0, w / 2 - 0.25], [0, 50.0, h / 2 - 0.5], [0, 0, 1]])
