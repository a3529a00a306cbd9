#!/usr/bin/env python3
"""What the edge table, the boundary loops and the hole filling cost on one MI355X (csrc/nfl_meshedge.hip through
nerf_fl_amd.topology): on the closed surface of a ball of radius 0.8 in [-1, 1]^3 extracted on a `--lattice`^3 lattice (no
loop), on a ball of radius 1.2 in the same box (the box cuts it: six rim loops of many hundreds of edges each, every one
folded by one thread in walk order), and on meshsmooth_ref's fan (a hub of 4096 triangles, a rim loop of 4096 edges).
Not a test: prints one JSON record per mesh (and writes all to --out).

Every call is timed under a host clock, the device idle before and after, since each holds one host read; the tables a call
can be given are given, so that a row is that call alone."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from geom_timing import host_timed  # noqa: E402


def ball(n, radius, dev):
    c = torch.linspace(-1.0, 1.0, n, device=dev, dtype=torch.float64)
    return (radius - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()


def measure(name, mesh, a):
    from nerf_fl_amd import _lib, geometry, topology
    V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
    adj = geometry.mesh_adjacency(mesh)
    ed = topology.mesh_edges(mesh, adjacency=adj)
    lp = topology.boundary_loops(mesh, edges=ed)
    filled, info = topology.fill_holes(mesh, loops=lp)
    lib = _lib.lib()
    case = {"mesh": name, "vertices": V, "triangles": T, "edges": ed["n_edges"], "boundary_edges": ed["n_boundary"],
            "loops": lp["n_loops"], "longest_loop": int(lp["length"].max()) if lp["n_loops"] else 0, "filled": info["n_filled"],
            "edges_scratch_bytes": lib.nfl_mesh_edges_bytes(V, T), "loops_scratch_bytes": lib.nfl_mesh_loops_bytes(T),
            "mesh_adjacency_host_ms": host_timed(lambda: geometry.mesh_adjacency(mesh), a.warmup, a.iters),
            "mesh_edges_host_ms": host_timed(lambda: topology.mesh_edges(mesh, adjacency=adj), a.warmup, a.iters),
            "boundary_loops_host_ms": host_timed(lambda: topology.boundary_loops(mesh, edges=ed), a.warmup, a.iters),
            "fill_holes_host_ms": host_timed(lambda: topology.fill_holes(mesh, loops=lp), a.warmup, a.iters),
            "mesh_topology_host_ms": host_timed(lambda: topology.mesh_topology(mesh, edges=ed, loops=lp), a.warmup, a.iters)}
    print(json.dumps(case), flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=257)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "meshedge.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_meshedge.py measures on the GPU; there is none here")
    from nerf_fl_amd import geometry
    import meshsmooth_ref as mr
    dev = torch.device("cuda:0")
    box = (-1.0,) * 3, (1.0,) * 3
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "meshes": []}
    rec["meshes"].append(measure(f"closed ball {a.lattice}^3", geometry.extract_surface(ball(a.lattice, 0.8, dev), 0.0, *box), a))
    rec["meshes"].append(measure(f"ball cut by the box {a.lattice}^3", geometry.extract_surface(ball(a.lattice, 1.2, dev), 0.0, *box), a))
    fan = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in mr.fan(4096, 300, seed=0).items()}
    rec["meshes"].append(measure("fan, hub of 4096", fan, a))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
