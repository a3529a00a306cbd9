"""The topology of a triangle mesh, on the device: its edge table, whether it is closed, manifold and oriented, where it is open,
and the caps that close it -- what solid.py's queries (inside_mesh, signed_distance, solid_lattice, remesh, volume_overlap,
mesh_volume) ask of their mesh and could not check.

    mesh_edges       nfl_mesh_edges_count / _emit: the unique edges, the half-edges on each, every half-edge's twin, a kind per edge
    boundary_loops   nfl_mesh_loops_count / _emit: the boundary half-edges chained into closed loops, with a table per loop
    mesh_topology    closed? manifold? oriented? Euler characteristic, loops and genus per component
    fill_holes       nfl_mesh_fill_count / _emit: the selected loops capped, everything that existed kept bit for bit

The definitions are written out in include/nerf_fl_amd.h, "mesh edges"; DESIGN.md section 39.  A mesh is the geometry package's
dict (vertices, normals, triangles, colors where it has them, on a ROCm device).  Every table is integer work or an fp64 sum in a
fixed order: two calls give the same bits.  There is no CPU path."""
import torch

from . import _lib
from .geometry import mesh_components
from .geometry._call import _call, _is, _mesh_tensors, _on_device, _positive, _ptr, _refuse_outside, _scratch
from .geometry.mesh import _adjacency_of

__all__ = ["mesh_edges", "mesh_topology", "boundary_loops", "fill_holes"]

_EDGE_TOTALS = ("n_edges", "n_halves", "n_boundary", "n_flipped", "n_nonmanifold", "n_degenerate")


def _totals(name, n, dev, *args):
    """The counting half of a sized call with plain arguments: entry point `name` fills `n` int64 totals, the last argument
    before the stream, and they come back as Python ints -- the one place this module reads the device."""
    totals = torch.zeros(n, dtype=torch.int64, device=dev)
    _call(name, *args, _ptr(totals))
    return [int(v) for v in totals.tolist()]                                  # THE host read


def _new(dev):
    return lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)


def mesh_edges(mesh, adjacency=None):
    """The edge table of `mesh`, a dict:

        edges (E, 2) int32                                   the unordered pairs {a, b}, a < b, that have a half-edge, ascending;
        half_edge (3T,) int32                                the edge of half-edge 3 t + c (tri[t][c] -> tri[t][(c + 1) % 3]), -1
                                                             for one whose ends are equal;
        edge_offsets (E + 1,) int64, edge_halves (H,) int32  the half-edges on every edge, ascending;
        kind (E,) uint8                                      _lib.EDGE_KINDS: interior (two half-edges, one each way), boundary
                                                             (one), flipped (two the same way), nonmanifold (three or more);
        twin (3T,) int32                                     the other half-edge of an interior edge, else -1;
        n_edges, n_halves, n_boundary, n_flipped, n_nonmanifold, n_degenerate   Python ints.

    `adjacency` is what geometry.mesh_adjacency(mesh) returned; without it that call is made here (its synchronisation too).
    ValueError when a triangle has an index outside [0, V).  ONE host synchronisation of its own: the totals."""
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    totals = [0] * (_lib.EDGE_TOTALS - 1) + [T if V == 0 else 0]
    with torch.cuda.device(dev):
        if V and T:
            adj = _adjacency_of(adjacency, mesh, V, dev)
            N = adj["neighbors"].shape[0]
            if N > 6 * T:
                raise ValueError(f"adjacency: {N} neighbours are not those of a mesh of {T} triangles")
            scratch = _scratch(_lib.lib().nfl_mesh_edges_bytes(V, T), dev)
            head = (_ptr(tri), V, T)
            totals = _totals("nfl_mesh_edges_count", _lib.EDGE_TOTALS, dev, *head, _ptr(adj["offsets"]), _ptr(adj["neighbors"]), N,
                             _ptr(scratch), scratch.numel() * 8)
        _refuse_outside(totals[-1], T, V)
        E, H = totals[:2]
        new = _new(dev)
        out = {"edges": new((E, 2), torch.int32), "half_edge": new(3 * T, torch.int32), "edge_offsets": new(E + 1, torch.int64),
               "edge_halves": new(H, torch.int32), "kind": new(E, torch.uint8), "twin": new(3 * T, torch.int32)}
        if V and T:
            _call("nfl_mesh_edges_emit", *head, _ptr(scratch), scratch.numel() * 8, E, H, _ptr(out["edges"]), _ptr(out["half_edge"]),
                  _ptr(out["edge_offsets"]), _ptr(out["edge_halves"]), _ptr(out["kind"]), _ptr(out["twin"]))
        else:
            out["edge_offsets"].zero_()
    out.update(zip(_EDGE_TOTALS, totals))
    return out


def _count_ok(n, top):
    return isinstance(n, int) and not isinstance(n, bool) and 0 <= n <= top


def _edges_of(edges, mesh, T, dev):
    """`edges` (what mesh_edges returned) checked against T triangles on `dev`; built from `mesh` when None."""
    if edges is None:
        return mesh_edges(mesh)
    try:
        he, twin, kind, pairs, nb = (edges[k] for k in ("half_edge", "twin", "kind", "edges", "n_boundary"))
    except (TypeError, KeyError):
        raise ValueError("edges: the dict mesh_edges returns") from None
    _on_device(he, twin, kind, pairs)
    E = kind.shape[0] if kind.dim() == 1 else -1
    if not (_is(he, torch.int32, 1, (3 * T,), dev) and _is(twin, torch.int32, 1, (3 * T,), dev) and _is(kind, torch.uint8, 1, device=dev)
            and _is(pairs, torch.int32, 2, (E, 2), dev) and E <= 3 * T and _count_ok(nb, 3 * T)):
        raise ValueError(f"edges: not the edge table of a mesh of {T} triangles on the mesh's device")
    return edges


def boundary_loops(mesh, edges=None):
    """The boundary of `mesh` as closed loops, a dict.  The successor of a boundary half-edge a -> b is found by rotating about
    b through the twins, so a loop does not cross at a vertex where two sheets pinch; where the rotation ends on a flipped or
    non-manifold edge the chain is open and belongs to no loop.

        loop_offsets (L + 1,) int64, loop_halves (B',) int32   the half-edges of every loop in walk order, from its smallest one;
                                                               loops are numbered by that smallest half-edge;
        loop_of (3T,) int32                                    the loop of a half-edge, -1 on none;
        length (L,) int32, perimeter (L,) fp32, centroid (L, 3) fp32   fp64 sums in walk order, rounded once; a loop with a
                                                               non-finite vertex has perimeter +inf and centroid 0;
        n_loops, n_open                                        Python ints: L, and the boundary half-edges on open chains.

    `edges` is what mesh_edges(mesh) returned; without it that call is made here (its synchronisations too).  ONE host
    synchronisation of its own: the totals."""
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    ed = _edges_of(edges, mesh, T, dev)
    totals = [0] * _lib.LOOP_TOTALS
    with torch.cuda.device(dev):
        if V and T:
            scratch = _scratch(_lib.lib().nfl_mesh_loops_bytes(T), dev)
            totals = _totals("nfl_mesh_loops_count", _lib.LOOP_TOTALS, dev, _ptr(ver), _ptr(tri), V, T, _ptr(ed["half_edge"]),
                             _ptr(ed["twin"]), _ptr(ed["kind"]), ed["kind"].shape[0], ed["n_boundary"], _ptr(scratch),
                             scratch.numel() * 8)
        L, B, n_open = totals
        new = _new(dev)
        out = {"loop_offsets": new(L + 1, torch.int64), "loop_halves": new(B, torch.int32), "loop_of": new(3 * T, torch.int32),
               "length": new(L, torch.int32), "perimeter": new(L, torch.float32), "centroid": new((L, 3), torch.float32)}
        if V and T:
            _call("nfl_mesh_loops_emit", T, _ptr(scratch), scratch.numel() * 8, L, B, _ptr(out["loop_offsets"]),
                  _ptr(out["loop_halves"]), _ptr(out["loop_of"]), _ptr(out["length"]), _ptr(out["perimeter"]), _ptr(out["centroid"]))
        else:
            out["loop_offsets"].zero_()
            out["loop_of"].fill_(-1)
    out.update(n_loops=L, n_open=n_open)
    return out


def _loops_of(loops, mesh, edges, T, dev):
    """`loops` (what boundary_loops returned) checked against T triangles on `dev`; built from `mesh` when None."""
    if loops is None:
        return boundary_loops(mesh, edges=edges)
    try:
        rows = [loops[k] for k in ("loop_offsets", "loop_halves", "loop_of", "length", "perimeter", "centroid")]
        n_open = loops["n_open"]
    except (TypeError, KeyError):
        raise ValueError("loops: the dict boundary_loops returns") from None
    _on_device(*rows)
    off, halves, loop_of, length, perimeter, centroid = rows
    L = length.shape[0] if length.dim() == 1 else -1
    if not (_is(off, torch.int64, 1, (L + 1,), dev) and _is(halves, torch.int32, 1, device=dev) and _is(loop_of, torch.int32, 1, (3 * T,), dev)
            and _is(length, torch.int32, 1, device=dev) and _is(perimeter, torch.float32, 1, (L,), dev)
            and _is(centroid, torch.float32, 2, (L, 3), dev) and L <= T and halves.shape[0] <= 3 * T and _count_ok(n_open, 3 * T)):
        raise ValueError(f"loops: not the boundary loops of a mesh of {T} triangles on the mesh's device")
    return loops


def mesh_topology(mesh, edges=None, loops=None):
    """What solid.py's queries need to know of `mesh`, a dict.  Whole mesh (Python values): `closed` (no boundary edge),
    `manifold` (no non-manifold edge), `oriented` (no flipped edge), `n_loops`, `n_open`, `n_components`.  Per component, (C,)
    int64 tensors on the device, components numbered as geometry.mesh_components numbers them (`component` (V,) int32):

        vertices, edges, triangles   an edge and a triangle count for the component of their first vertex;
        euler                        vertices - edges + triangles;
        loops                        boundary loops;
        genus                        (2 - euler - loops) / 2 where the component has neither a flipped nor a non-manifold edge
                                     and that number is a non-negative integer, else -1.

    `edges` and `loops` are what mesh_edges and boundary_loops returned; what is missing is built here.  Host synchronisations:
    mesh_components', and those of what it has to build."""
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    ed = _edges_of(edges, mesh, T, dev)
    lp = _loops_of(loops, mesh, ed, T, dev)
    parts = mesh_components(mesh)
    C, comp = parts["n_components"], parts["component"].long()
    count = lambda idx: torch.zeros(C, dtype=torch.int64, device=dev).scatter_add_(0, idx, torch.ones_like(idx))
    e_comp = comp[ed["edges"][:, 0].long()]
    first = lp["loop_halves"].long()[lp["loop_offsets"][:-1]]                 # a loop's first half-edge starts in its component
    n_v, n_e, n_t = parts["vertices"].long(), count(e_comp), parts["triangles"].long()
    n_l = count(comp[tri.reshape(-1).long()[first]])
    kind = ed["kind"]
    bad = count(e_comp[(kind == _lib.EDGE_KINDS["flipped"]) | (kind == _lib.EDGE_KINDS["nonmanifold"])]) > 0
    euler = n_v - n_e + n_t
    twice = 2 - euler - n_l
    genus = torch.where(~bad & (twice >= 0) & (twice % 2 == 0), twice // 2, torch.full_like(twice, -1))
    return {"closed": ed["n_boundary"] == 0, "manifold": ed["n_nonmanifold"] == 0, "oriented": ed["n_flipped"] == 0,
            "n_loops": lp["n_loops"], "n_open": lp["n_open"], "n_components": C, "component": parts["component"],
            "vertices": n_v, "edges": n_e, "triangles": n_t, "euler": euler, "loops": n_l, "genus": genus}


def _max_edges(max_edges):
    if max_edges is None:
        return 2 ** 62
    if isinstance(max_edges, bool) or not isinstance(max_edges, int) or max_edges < 3:
        raise ValueError(f"max_edges: None or an int of at least 3, got {max_edges!r}")
    return min(max_edges, 2 ** 62)


def fill_holes(mesh, max_edges=None, max_perimeter=None, keep=None, loops=None, edges=None):
    """`mesh` with its selected boundary loops capped: (new mesh dict, info).  A loop is selected when it has at least 3
    half-edges and at most `max_edges` (None: no limit), a finite perimeter of at most `max_perimeter` (compared in fp32; None: no
    limit), and `keep` ((L,) bool on the mesh's device, loops as boundary_loops numbers them), where given, names it -- so small
    holes are closed and the outer rim of a scene is left alone.  A loop of 3 gets the one triangle that covers it; a longer
    one gets a new vertex at its centroid (normal: the normalised sum of the fan's triangle vectors; colour: the mean of the
    loop's) and a triangle per half-edge.  Input rows are kept bit for bit; new vertices and triangles follow them in loop order
    and, within a loop, walk order, each new triangle running against the half-edge it covers.

    info: `n_filled`, `n_new_vertices`, `n_new_triangles`, and the bool tensors `new_vertices` (V',) and `new_triangles` (T',):
    geometry.smooth_mesh(filled, pinned=~info["new_vertices"]) relaxes the caps alone.  With nothing selected `mesh` itself is
    returned.  `loops` and `edges` are what boundary_loops and mesh_edges returned; what is missing is built here (its
    synchronisations too).  ONE host synchronisation of its own: the totals."""
    max_edges = _max_edges(max_edges)
    max_perimeter = _positive(max_perimeter, "max_perimeter: None or a positive number")
    ver, nrm, col, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    lp = _loops_of(loops, mesh, edges, T, dev)
    L, B = lp["length"].shape[0], lp["loop_halves"].shape[0]
    if keep is not None:
        _on_device(keep)
        if not _is(keep, torch.bool, 1, (L,), dev):
            raise ValueError(f"keep: expected a contiguous bool ({L},) tensor on the mesh's device")
    totals = [0] * _lib.FILL_TOTALS
    with torch.cuda.device(dev):
        if V and T and L:
            scratch = _scratch(_lib.lib().nfl_mesh_fill_bytes(L), dev)
            totals = _totals("nfl_mesh_fill_count", _lib.FILL_TOTALS, dev, L, _ptr(lp["length"]), _ptr(lp["perimeter"]), _ptr(keep),
                             max_edges, max_perimeter, _ptr(scratch), scratch.numel() * 8)
        n_filled, nv, nt = totals
        new = _new(dev)
        info = {"n_filled": n_filled, "n_new_vertices": nv, "n_new_triangles": nt, "new_vertices": new(V + nv, torch.bool),
                "new_triangles": new(T + nt, torch.bool)}
        if n_filled == 0:
            info["new_vertices"].zero_()
            info["new_triangles"].zero_()
            return mesh, info
        out = {"vertices": new((V + nv, 3), torch.float32), "normals": new((V + nv, 3), torch.float32),
               "triangles": new((T + nt, 3), torch.int32)}
        if col is not None:
            out["colors"] = new((V + nv, 3), torch.float32)
        _call("nfl_mesh_fill_emit", _ptr(ver), _ptr(nrm), _ptr(col), _ptr(tri), V, T, _ptr(lp["loop_offsets"]), _ptr(lp["loop_halves"]),
              _ptr(lp["loop_of"]), _ptr(lp["centroid"]), L, B, _ptr(scratch), scratch.numel() * 8, nv, nt, _ptr(out["vertices"]),
              _ptr(out["normals"]), _ptr(out.get("colors")), _ptr(out["triangles"]), _ptr(info["new_vertices"]),
              _ptr(info["new_triangles"]))
    return out, info
