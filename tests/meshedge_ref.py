"""numpy restatement of the mesh edges of csrc/nfl_meshedge.hip (include/nerf_fl_amd.h, "mesh edges"), for
tests/test_meshedge_cpu.py and tests/test_meshedge_gpu.py.  numpy alone, int64 and fp64, sort based; nothing of the product
package.  Plain loops where the order matters (the walk of a loop), and sums that run over the loops side by side but, within
a loop, strictly in walk order.

The same definitions as the kernels:

* a triangle with an index outside [0, V) is counted and takes part in nothing;
* half-edge h = 3 t + c runs from tri[t][c] to tri[t][(c + 1) % 3]; equal ends: degenerate, edge id -1;
* edges are the unordered pairs with a half-edge, numbered in ascending (a, b); the half-edges of an edge ascending;
* kind: INTERIOR two half-edges in opposite directions, BOUNDARY one, FLIPPED two in the same direction, NONMANIFOLD three or more;
* twin: the other half-edge of an INTERIOR edge, else -1;
* succ of a boundary half-edge: the rotation about its end vertex through the twins, -1 unless it stops on a BOUNDARY edge;
* a loop is a cycle of succ, numbered by its smallest half-edge and listed from it; chains are open;
* perimeter, centroid: fp64 sums in walk order, rounded once; a non-finite vertex: perimeter +inf, centroid 0;
* fill: a loop of 3 gets the triangle (b, a, c); a longer one a vertex z at its centroid and (b, a, z) per half-edge a -> b.
"""
import numpy as np

INTERIOR, BOUNDARY, FLIPPED, NONMANIFOLD = 0, 1, 2, 3
F = np.float32


def _ends(triangles):
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return tri, tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)


def _nxt(h):
    return h - h % 3 + (h % 3 + 1) % 3


def edges(triangles, V):
    """-> dict(edges (E, 2) int32, half_edge (3T,) int32, edge_offsets (E + 1,) int64, edge_halves (H,) int32, kind (E,) uint8,
    twin (3T,) int32, totals [E, H, boundary, flipped, nonmanifold, degenerate, out of range])."""
    tri, start, end = _ends(triangles)
    T = len(tri)
    inside = np.repeat(((tri >= 0) & (tri < V)).all(axis=1), 3)
    live = inside & (start != end)
    hs = np.flatnonzero(live)                               # ascending
    key = np.minimum(start[hs], end[hs]) * max(V, 1) + np.maximum(start[hs], end[hs])
    uniq, inv = np.unique(key, return_inverse=True)         # ascending (a, b)
    E = len(uniq)
    half_edge = np.full(3 * T, -1, dtype=np.int64)
    half_edge[hs] = inv
    halves = hs[np.argsort(inv, kind="stable")]             # by (edge, half-edge)
    count = np.bincount(inv, minlength=E)
    offsets = np.zeros(E + 1, dtype=np.int64)
    np.cumsum(count, out=offsets[1:])
    kind = np.full(E, NONMANIFOLD, dtype=np.uint8)
    kind[count == 1] = BOUNDARY
    two = np.flatnonzero(count == 2)
    h0, h1 = halves[offsets[two]], halves[offsets[two] + 1]
    opposite = (start[h0] < end[h0]) != (start[h1] < end[h1])
    kind[two] = np.where(opposite, INTERIOR, FLIPPED)
    twin = np.full(3 * T, -1, dtype=np.int64)
    twin[h0[opposite]] = h1[opposite]
    twin[h1[opposite]] = h0[opposite]
    totals = [E, len(hs), int((kind == BOUNDARY).sum()), int((kind == FLIPPED).sum()), int((kind == NONMANIFOLD).sum()),
              int((inside & (start == end)).sum()), int((~inside).sum()) // 3]
    return {"edges": np.stack([uniq // max(V, 1), uniq % max(V, 1)], axis=1).astype(np.int32).reshape(-1, 2),
            "half_edge": half_edge.astype(np.int32), "edge_offsets": offsets, "edge_halves": halves.astype(np.int32), "kind": kind,
            "twin": twin.astype(np.int32), "totals": totals}


def successor(ed):
    """succ (3T,) int64: -2 for a half-edge that is not on a BOUNDARY edge, -1 for a dead end."""
    he, twin, kind = ed["half_edge"].astype(np.int64), ed["twin"].astype(np.int64), ed["kind"]
    H3 = len(he)
    on_boundary = np.zeros(H3, dtype=bool)
    on_boundary[he >= 0] = kind[he[he >= 0]] == BOUNDARY
    succ = np.full(H3, -2, dtype=np.int64)
    hs = np.flatnonzero(on_boundary)
    g = _nxt(hs)
    active = np.ones(len(hs), dtype=bool)
    for _ in range(H3 + 1):                                 # every walk one step of the rotation at a time
        w = twin[g]
        stop = active & (w < 0)
        succ[hs[stop]] = np.where(on_boundary[g[stop]], g[stop], -1)
        active &= ~stop
        if not active.any():
            break
        g = np.where(active, _nxt(np.maximum(w, 0)), g)
    succ[hs[active]] = -1                                   # longer than 3 T steps
    return succ


def loops(vertices, triangles, ed):
    """-> dict(loop_offsets (L + 1,) int64, loop_halves (B',) int32, loop_of (3T,) int32, length (L,) int32, perimeter (L,) fp32,
    centroid (L, 3) fp32, n_loops, n_open)."""
    ver = np.asarray(vertices, dtype=F).reshape(-1, 3)
    _, start, end = _ends(triangles)
    succ = successor(ed)
    H3 = len(succ)
    state = np.zeros(H3, dtype=np.int8)                     # 0 not seen, 1 on a loop, 2 open
    loop_of = np.full(H3, -1, dtype=np.int64)
    rows = []
    for h in np.flatnonzero(succ != -2).tolist():           # ascending: a loop is met at its smallest half-edge first
        if state[h]:
            continue
        path, g = [h], int(succ[h])
        while g >= 0 and g != h and state[g] == 0:
            path.append(g)
            g = int(succ[g])
        if g == h:
            state[path] = 1
            loop_of[path] = len(rows)
            rows.append(path)
        else:
            state[path] = 2
    L = len(rows)
    length = np.array([len(r) for r in rows], dtype=np.int64)
    offsets = np.zeros(L + 1, dtype=np.int64)
    np.cumsum(length, out=offsets[1:])
    halves = np.array([h for r in rows for h in r], dtype=np.int64)
    v64 = ver.astype(np.float64)
    with np.errstate(all="ignore"):
        a, b = np.clip(start, 0, max(len(ver) - 1, 0)), np.clip(end, 0, max(len(ver) - 1, 0))
        d = v64[b] - v64[a] if len(ver) else np.zeros((H3, 3))
        seg = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        s, c, finite = np.zeros(L), np.zeros((L, 3)), np.ones(L, dtype=bool)
        for k in range(int(length.max()) if L else 0):      # step k of every loop that has one: walk order within a loop
            on = np.flatnonzero(length > k)
            h = halves[offsets[on] + k]
            s[on] += seg[h]
            c[on] += v64[a[h]]
            finite[on] &= np.isfinite(v64[a[h]]).all(axis=1)
        perimeter = np.where(finite, s.astype(F), F(np.inf)).astype(F)
        centroid = np.where(finite[:, None], (c / np.maximum(length, 1)[:, None].astype(np.float64)).astype(F), F(0)).astype(F)
    return {"loop_offsets": offsets, "loop_halves": halves.astype(np.int32), "loop_of": loop_of.astype(np.int32),
            "length": length.astype(np.int32), "perimeter": perimeter, "centroid": centroid.reshape(-1, 3), "n_loops": L,
            "n_open": int((state == 2).sum())}


def selected(lp, max_edges=None, max_perimeter=None, keep=None):
    sel = (lp["length"] >= 3) & np.isfinite(lp["perimeter"])
    if max_edges is not None:
        sel &= lp["length"] <= max_edges
    if max_perimeter is not None:
        sel &= lp["perimeter"] <= F(max_perimeter)
    if keep is not None:
        sel &= np.asarray(keep).astype(bool)
    return sel


def fill(mesh, lp, max_edges=None, max_perimeter=None, keep=None):
    """-> (mesh dict, info dict), what nerf_fl_amd.topology.fill_holes returns, on arrays."""
    ver, nrm, tri = (np.asarray(mesh[k]) for k in ("vertices", "normals", "triangles"))
    col = mesh.get("colors")
    _, start, end = _ends(tri)
    V, T = len(ver), len(tri)
    sel = np.flatnonzero(selected(lp, max_edges, max_perimeter, keep))
    length, off, halves = lp["length"].astype(np.int64), lp["loop_offsets"], lp["loop_halves"].astype(np.int64)
    new_v, new_n, new_c, new_t = [], [], [], []
    for l in sel.tolist():
        row = halves[off[l]:off[l] + length[l]]
        if length[l] == 3:
            new_t.append([start[row[1]], start[row[0]], start[row[2]]])
            continue
        z = V + len(new_v)
        zf = lp["centroid"][l]
        p2 = zf.astype(np.float64)
        s, cs = np.zeros(3), np.zeros(3)
        with np.errstate(all="ignore"):
            for h in row.tolist():                          # walk order
                a, b = start[h], end[h]
                new_t.append([b, a, z])
                p0, p1 = ver[b].astype(np.float64), ver[a].astype(np.float64)
                e1, e2 = p1 - p0, p2 - p0
                s[0] += e1[1] * e2[2] - e1[2] * e2[1]
                s[1] += e1[2] * e2[0] - e1[0] * e2[2]
                s[2] += e1[0] * e2[1] - e1[1] * e2[0]
                if col is not None:
                    cs += np.asarray(col)[a].astype(np.float64)
            norm = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
            ok = np.isfinite(norm) and norm > 0.0
            new_v.append(zf)
            new_n.append((s / norm).astype(F) if ok else np.zeros(3, F))
            new_c.append((cs / np.float64(length[l])).astype(F))
    rows = lambda old, new: np.concatenate([np.asarray(old, F).reshape(-1, 3), np.asarray(new, F).reshape(-1, 3)])
    out = {"vertices": rows(ver, new_v), "normals": rows(nrm, new_n),
           "triangles": np.concatenate([tri.reshape(-1, 3), np.asarray(new_t, np.int32).reshape(-1, 3)]).astype(np.int32)}
    if col is not None:
        out["colors"] = rows(col, new_c)
    info = {"n_filled": len(sel), "n_new_vertices": len(new_v), "n_new_triangles": len(new_t),
            "new_vertices": np.arange(len(out["vertices"])) >= V, "new_triangles": np.arange(len(out["triangles"])) >= T}
    return out, info


def components(triangles, V):
    """(component (V,) int64 numbered by smallest vertex, C): two vertices are connected when a triangle in range names both."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    tri = tri[((tri >= 0) & (tri < V)).all(axis=1)]
    label = np.arange(V)
    while True:                                             # the smallest label of a triangle spreads over it
        low = label[tri].min(axis=1) if len(tri) else np.zeros(0, np.int64)
        nxt = label.copy()
        for c in range(3):
            np.minimum.at(nxt, tri[:, c], low)
        nxt = nxt[nxt]
        if (nxt == label).all():
            break
        label = nxt
    roots, comp = np.unique(label, return_inverse=True)
    return comp, len(roots)


def topology(mesh, ed=None, lp=None):
    """The report of nerf_fl_amd.topology.mesh_topology, on arrays."""
    ver, tri = np.asarray(mesh["vertices"]), np.asarray(mesh["triangles"], dtype=np.int64).reshape(-1, 3)
    V = len(ver)
    ed = edges(tri, V) if ed is None else ed
    lp = loops(ver, tri, ed) if lp is None else lp
    comp, C = components(tri, V)
    kind = ed["kind"]
    inside = ((tri >= 0) & (tri < V)).all(axis=1)
    e_comp = comp[ed["edges"][:, 0].astype(np.int64)]
    n_v = np.bincount(comp, minlength=C)
    n_e = np.bincount(e_comp, minlength=C)
    n_t = np.bincount(comp[tri[inside, 0]], minlength=C)
    first = lp["loop_halves"].astype(np.int64)[lp["loop_offsets"][:-1]]
    n_l = np.bincount(comp[tri.reshape(-1)[first]], minlength=C)
    bad = np.bincount(e_comp[(kind == FLIPPED) | (kind == NONMANIFOLD)], minlength=C) > 0
    euler = n_v - n_e + n_t
    twice = 2 - euler - n_l
    genus = np.where(~bad & (twice >= 0) & (twice % 2 == 0), twice // 2, -1)
    return {"closed": not (kind == BOUNDARY).any(), "manifold": not (kind == NONMANIFOLD).any(),
            "oriented": not (kind == FLIPPED).any(), "n_loops": lp["n_loops"], "n_open": lp["n_open"], "n_components": C,
            "component": comp.astype(np.int32), "vertices": n_v, "edges": n_e, "triangles": n_t, "euler": euler, "loops": n_l,
            "genus": genus}


def signed_volume(vertices, triangles):
    """The sum over the triangles of a . (b x c) / 6 in fp64: the volume of a closed mesh wound outward."""
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64).reshape(-1, 3)]
    return float((p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def lowest_caps(mesh, lp):
    """The triangles that close every loop of `lp` by a fan from one of the loop's OWN vertices (no new vertex), the vertex
    chosen so that the signed volume is smallest.  The volume of a fan is linear in its apex, and the centroid is the mean of
    the loop's vertices, so the fan fill_holes makes has the mean of these volumes: at least the smallest."""
    ver = np.asarray(mesh["vertices"], dtype=np.float64)
    _, start, end = _ends(mesh["triangles"])
    caps = []
    for l in range(lp["n_loops"]):
        row = lp["loop_halves"][lp["loop_offsets"][l]:lp["loop_offsets"][l + 1]].astype(np.int64)
        fans = [[[end[h], start[h], start[k]] for h in row] for k in row]
        caps += min(fans, key=lambda f: signed_volume(ver, f))
    return np.asarray(caps, dtype=np.int32).reshape(-1, 3)


# ---- the meshes of the tests

def _mesh(ver, tri):
    ver = np.asarray(ver, dtype=F).reshape(-1, 3)
    return {"vertices": ver, "normals": np.tile(F([0, 0, 1]), (len(ver), 1)), "triangles": np.asarray(tri, dtype=np.int32).reshape(-1, 3)}


def moebius(n=8):
    """A strip of n quads whose last one is joined to the first with a half twist: vertices 2 k (one side) and 2 k + 1."""
    ang = 2.0 * np.pi * np.arange(n) / n
    ver = []
    for k in range(n):
        for s in (-0.3, 0.3):
            r = 1.0 + s * np.cos(ang[k] / 2)
            ver.append([r * np.cos(ang[k]), r * np.sin(ang[k]), s * np.sin(ang[k] / 2)])
    tri = []
    for k in range(n):
        a, b = 2 * k, 2 * k + 1
        c, d = (2 * (k + 1), 2 * (k + 1) + 1) if k + 1 < n else (1, 0)          # the twist
        tri += [[a, c, b], [b, c, d]]
    return _mesh(ver, tri)


def book(pages=300):
    """`pages` triangles on the one edge (0, 1), alternating in direction."""
    ang = 2.0 * np.pi * np.arange(pages) / pages
    ver = [[0, 0, 0], [0, 0, 1]] + [[np.cos(a), np.sin(a), 0.5] for a in ang]
    tri = [[0, 1, 2 + k] if k % 2 == 0 else [1, 0, 2 + k] for k in range(pages)]
    return _mesh(ver, tri)


def lattice_mesh(n, shape="ball"):
    """The marching-tetrahedra surface (tests/geometry_ref.py) of a ball of radius 0.6 or a torus on an n^3 lattice over [-1, 1]^3."""
    import geometry_ref as gr
    if shape == "ball":
        lat, lo, sp = gr.sphere_lattice(n)
    else:
        c = np.linspace(-1.0, 1.0, n)
        z, y, x = np.meshgrid(c, c, c, indexing="ij")
        lat = (0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z)).astype(F)
        lo, sp = (-1.0,) * 3, (2.0 / (n - 1),) * 3
    return gr.extract(lat, 0.0, lo, sp)


def punch(mesh, k=5, seed=0):
    """`mesh` without the one-rings of k vertices no two of which share a neighbour: (mesh, the vertices, their valences)."""
    tri = np.asarray(mesh["triangles"], dtype=np.int64)
    V = len(mesh["vertices"])
    nbrs = [set() for _ in range(V)]
    for a, b, c in tri.tolist():
        nbrs[a] |= {b, c}
        nbrs[b] |= {a, c}
        nbrs[c] |= {a, b}
    rng = np.random.default_rng(seed)
    chosen, blocked = [], set()
    for v in rng.permutation(V).tolist():
        ring = nbrs[v] | {v}
        if len(nbrs[v]) >= 3 and not (ring & blocked):
            chosen.append(v)
            blocked |= ring | {w for u in nbrs[v] for w in nbrs[u]}
        if len(chosen) == k:
            break
    keep = ~np.isin(tri, chosen).any(axis=1)
    out = dict(mesh, triangles=np.ascontiguousarray(tri[keep]).astype(np.int32))
    return out, chosen, [len(nbrs[v]) for v in chosen]
