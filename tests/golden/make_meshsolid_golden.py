"""The fixtures of tests/test_meshsolid_cpu.py and tests/test_meshsolid_gpu.py.

    python tests/golden/make_meshsolid_golden.py ball      (needs the device)
        meshsolid_ball_08_17.npz: geom_gpu_util.ball_mesh(0.8, 17), vertices and triangles as extract_surface emits them.
        The GPU tests compare the file with the device's bits every run, so it cannot go stale unnoticed.
    python tests/golden/make_meshsolid_golden.py lattice   (numpy alone, about half a minute)
        meshsolid_lattice_17.npz: the restated composition of solid.solid_lattice(ball, [-1, 1]^3, 17^3) before the lattice
        value -- the signed distance within trunc = 0.375 (meshdist_ref.closest), the flags and the votes of three directions
        (meshsolid_ref.inside) -- which takes too long to compute in every run of the suite.  No box: the grid that
        solid_lattice builds is triangle_grid's over the same mesh, whose box holds every point of every triangle (lo is the
        least vertex coordinate itself, and lo + dims * cell lies beyond the greatest), so THE BOX RULE refuses nothing."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import meshsolid_ref as sref  # noqa: E402

if sys.argv[1:] == ["ball"]:
    from geom_gpu_util import ball_mesh
    mesh = ball_mesh(0.8, 17)
    np.savez_compressed(os.path.join(HERE, "meshsolid_ball_08_17.npz"), vertices=mesh["vertices"].cpu().numpy(),
                        triangles=mesh["triangles"].cpu().numpy())
elif sys.argv[1:] == ["lattice"]:
    ver, tri = sref.ball()
    box, res = ((-1.0,) * 3, (1.0,) * 3), (17, 17, 17)
    pts = sref.lattice_points(*box, res).reshape(-1, 3)
    sd, inside, votes = sref.signed_distance(pts, ver, tri, 3, None, sref.default_trunc(*box, res))
    np.savez_compressed(os.path.join(HERE, "meshsolid_lattice_17.npz"), sd=sd, inside=inside, votes=votes)
else:
    sys.exit(__doc__)
