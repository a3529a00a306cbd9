"""Test-side restatements for nerf_fl_amd.data (shared by test_data_cpu.py and test_data_gpu.py): the keyed permutation
of include/nerf_fl_amd.h in numpy, the row formulas of nfl_gather_batch in CPU torch, and the fixture loaders.  Nothing
here calls the code under test."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENE = os.path.join(GOLDEN, "data_blender")
SCENE_SMALL = os.path.join(SCENE, "small")
RAY_TOL = 2e-7          # tests/test_eval_gpu.py's bound for the same arithmetic
M64 = (1 << 64) - 1


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


def round_keys(key, rounds=6):
    keys, state = [], int(key)
    for _ in range(rounds):
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        keys.append((z ^ (z >> 31)) & 0xFFFFFFFF)
    return keys


def _mix(v):
    v = v ^ (v >> np.uint32(16))
    v = v * np.uint32(0x85EBCA6B)
    v = v ^ (v >> np.uint32(13))
    v = v * np.uint32(0xC2B2AE35)
    return v ^ (v >> np.uint32(16))


def perm(key, n, p):
    """perm_{key, n}(p) for an int64 array p of positions in [0, n); key 0 is the identity."""
    p = np.asarray(p, dtype=np.int64)
    if key == 0:
        return p.copy()
    bits = 0
    while (1 << bits) < n:
        bits += 1
    h = max(1, (bits + 1) // 2)
    mask = np.uint32((1 << h) - 1)
    keys = [np.uint32(k) for k in round_keys(key)]
    x = p.copy()
    todo = np.arange(x.size)
    with np.errstate(over="ignore"):
        while todo.size:
            v = x[todo]
            l, r = (v >> h).astype(np.uint32), (v & int(mask)).astype(np.uint32)
            for k in keys:
                l, r = r, l ^ (_mix(r * np.uint32(0x9E3779B1) + k) & mask)
            v = (l.astype(np.int64) << h) | r.astype(np.int64)
            x[todo] = v
            todo = todo[v >= n]
    return x


def expected_rows(table, pixels, q, layout="world"):
    """Rows of flat pixels q from a bank's host arrays, in CPU torch fp32, one rounding per operation: (rays, rgbs, ts)."""
    q = np.asarray(q, dtype=np.int64)
    img = np.searchsorted(table["pix0"], q, side="right") - 1
    rec = table[img]
    local = q - rec["pix0"]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    x, y = f32(local % rec["width"]), f32(local // rec["width"])
    fx, fy, cx, cy = (f32(rec[k]) for k in ("fx", "fy", "cx", "cy"))
    d = torch.stack([(x - cx) / fx, -(y - cy) / fy, -torch.ones_like(x)], -1)
    near, far = f32(rec["near"])[:, None], f32(rec["far"])[:, None]
    if layout == "camera":
        rays = torch.cat([d, near, far], 1)
    else:
        c2w = f32(rec["c2w"]).reshape(-1, 3, 4)
        w = (d[:, None, :] * c2w[:, :, :3]).sum(-1)
        w = w / torch.norm(w, dim=-1, keepdim=True)
        rays = torch.cat([c2w[:, :, 3], w, near, far], 1)
    ch = rec["channels"].astype(np.int64)
    base = rec["byte0"] + local * ch
    c = torch.stack([torch.from_numpy(pixels[base + k]) for k in range(3)], -1).to(torch.float32).div(255)
    if (ch == 4).all():
        a = torch.from_numpy(pixels[base + 3]).to(torch.float32).div(255)[:, None]
        c = c * a + (1 - a)
    else:
        assert (ch == 3).all()
    return rays, c, torch.from_numpy(rec["id"].astype(np.int64))


def photo_inputs():
    g = golden("g23_data_photo.npz")
    images = [g[f"image{i}"] for i in range(len(g["ids"]))]
    return g, dict(images=images, c2w=g["c2w"], K=g["K"], near=g["near"], far=g["far"], ids=g["ids"])


def check_rays(got, exp, layout="world"):
    """Origins / near / far exact, directions within RAY_TOL (world); camera rows: the divisions are one correctly
    rounded operation each, so the same bound holds with room."""
    got, exp = torch.as_tensor(got).cpu(), torch.as_tensor(exp).cpu()
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if layout == "world":
        assert torch.equal(got[:, :3], exp[:, :3]) and torch.equal(got[:, 6:], exp[:, 6:])
        err = (got[:, 3:6] - exp[:, 3:6]).abs().max().item()
    else:
        assert torch.equal(got[:, 2:], exp[:, 2:])
        err = (got[:, :2] - exp[:, :2]).abs().max().item()
    assert err <= RAY_TOL, err
    return err
