"""Empty space of a lattice: OccupancyGrid, occupancy_grid, clip_rays."""
import numpy as np
import torch

from .. import _lib
from ._call import _is, _launch, _on_device, _ptr, _scratch
from .lattice import _lattice


class OccupancyGrid:
    """One bit per cell of a lattice (the definition is written out in include/nerf_fl_amd.h, "occupancy").

        bits        (cz, cy, wx) int32 on the device: cell (i, j, k) is bit i & 31 of bits[k, j, i >> 5]
        lo, spacing 3 floats each, (x, y, z): lattice plane b of an axis lies at lo + b * spacing (fp32)
        cells       (cx, cy, cz)
        threshold, dilate   what the grid was built with"""

    def __init__(self, bits, lo, spacing, cells, threshold, dilate):
        self.bits, self.lo, self.spacing, self.cells = bits, tuple(lo), tuple(spacing), tuple(cells)
        self.threshold, self.dilate = float(threshold), int(dilate)

    def to_dense(self):
        """(cz, cy, cx) bool tensor on the device: the cells, unpacked with torch bit operations."""
        cx, cy, cz = self.cells
        shifts = torch.arange(32, dtype=torch.int32, device=self.bits.device)
        return ((self.bits[..., None] >> shifts) & 1).bool().reshape(cz, cy, -1)[..., :cx]

    def fraction(self):
        """Share of occupied cells.  ONE host read."""
        cx, cy, cz = self.cells
        return float(self.to_dense().sum().item()) / (cx * cy * cz)


def occupancy_grid(lattice, threshold, lo, hi, dilate=1):
    """The OccupancyGrid of `lattice` ((nz, ny, nx) fp32, contiguous, on the device; density_lattice returns one) over
    the box [lo, hi]: a cell is occupied when one of its 8 corner values is >= `threshold` (NaN never is), or when a
    cell within `dilate` (0 .. 8) cells of it, in the Chebyshev sense, is.  Built on the device in four launches, without
    atomics: two calls give the same bits.  Nothing here synchronises with the host.

    The default of ONE cell of dilation is the usual practice and not a measured choice: the density between lattice
    points is not bounded by the corner values, so a thin structure that passes between the points of a cell is missed
    at any threshold, and the dilation only makes that less likely.  Choose the lattice fine enough for the scene."""
    nx, ny, nz, lo, sp = _lattice(lattice, lo, hi)
    dilate = int(dilate)
    if not 0 <= dilate <= 8:
        raise ValueError("dilate: 0 .. 8 cells")
    dev = lattice.device
    lib = _lib.lib()
    nbytes, sbytes = lib.nfl_occ_bytes(nx, ny, nz), lib.nfl_occ_build_bytes(nx, ny, nz, dilate)
    if nbytes == 0 or sbytes == 0:
        raise ValueError(f"lattice {nx} x {ny} x {nz}: at most 2^30 points, and 65535 rows and planes")
    bits = torch.empty(nz - 1, ny - 1, (nx - 1 + 31) // 32, dtype=torch.int32, device=dev)
    scratch = _scratch(sbytes, dev)
    a = _lib.OccBuildArgs()
    a.d_lattice, a.nx, a.ny, a.nz, a.threshold, a.dilate = _ptr(lattice), nx, ny, nz, float(threshold), dilate
    a.d_scratch, a.scratch_bytes, a.d_bits = _ptr(scratch), scratch.numel() * 8, _ptr(bits)
    with torch.cuda.device(dev):
        _launch("nfl_occ_build", a)
    f32 = lambda v: float(np.float32(v))
    return OccupancyGrid(bits, [f32(v) for v in lo], [f32(v) for v in sp], (nx - 1, ny - 1, nz - 1), threshold, dilate)


def clip_rays(grid, rays):
    """Walk `rays` ((R, 8) fp32 rows [o, d, near, far] on the grid's device) through the OccupancyGrid `grid`.  Returns
    (rays', hit): rays' is a copy whose columns 6 and 7 hold, for a ray that meets an occupied cell inside [near, far],
    the depth at which it enters the first one and the depth at which it leaves the last one, and the ray's own near and
    far otherwise; hit (R,) bool tells the two apart.  The direction need not be normalised: the depths are in the
    ray's own parameter, as the renderer samples them.

    Space outside the grid's box is EMPTY: a ray that does not cross the box hits nothing, whatever the field holds
    there.  A ray with a NaN in it hits nothing.  No host synchronisation."""
    if not isinstance(grid, OccupancyGrid):
        raise ValueError("clip_rays: `grid` is what occupancy_grid returns")
    _on_device(rays)
    if not _is(rays, torch.float32, 2, (8,), contiguous=False):
        raise ValueError("rays: expected an fp32 (R, 8) tensor")
    dev = grid.bits.device
    if rays.device != dev:
        raise ValueError("rays and grid on different devices")
    out = rays.clone(memory_format=torch.contiguous_format)
    R = rays.shape[0]
    near_far = torch.empty(R, 2, dtype=torch.float32, device=dev)
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    cx, cy, cz = grid.cells
    a = _lib.OccClipArgs()
    a.d_rays, a.n_rays, a.d_bits, a.nx, a.ny, a.nz = _ptr(out), R, _ptr(grid.bits), cx + 1, cy + 1, cz + 1
    a.lo[:], a.spacing[:] = grid.lo, grid.spacing
    a.d_near_far, a.d_hit = _ptr(near_far), _ptr(hit)
    with torch.cuda.device(dev):
        _launch("nfl_occ_clip_rays", a)
    out[:, 6:8] = near_far
    return out, hit.view(torch.bool)
