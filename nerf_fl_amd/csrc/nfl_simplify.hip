// nfl_simplify.hip -- simplifying an indexed triangle mesh on the device by uniform vertex clustering
// (include/nerf_fl_amd.h, "mesh simplification").  DESIGN.md section 21.
//
//   count  init      both tables empty, the two counters of d_totals = 0
//          vertices  a thread per vertex: cell and key in fp64, linear probing from a mixed hash, the key claimed by a 64-bit
//                    compare-and-swap on a slot that reads empty; then the slot's atomic minimum of the vertex index.  A
//                    probe sequence ends at the key or at the first empty slot; the table is at most half full, so one
//                    exists, and the loop is bounded by the capacity besides.  Nobody waits for anybody.
//          leader    cluster[v] = the smallest vertex index of v's slot, flag[v] = (that is v)
//          scan      exclusive scan of the flags (nm_scan of nfl_mesh_scan.hip): the rank of every leader; the total is V'
//          rank      cluster[v] = rank[cluster[v]]
//          map       a thread per triangle: the three new ids; dropped (canon[3 t] = -1) when out of range, on a vertex
//                    without a cluster or with two equal ids; else the triple rotated so that its smallest id comes first
//          triangles the NEXT launch, so that every canonical triple is published: a slot of the second table is claimed
//                    write-once by a triangle index (compare-and-swap from -1) and recognised by the claimant's triple;
//                    then the slot's atomic minimum of the triangle index
//          survive   flag[t] = (t is the minimum of its slot);  scan: the offsets of the survivors, the total is T'
//   emit   zero the accumulators of V' clusters; a thread per vertex adds its fixed-point position, normal and colour
//          (int64 atomic adds: any order, the same sums); QUADRIC: a thread per triangle adds w n n^T and w d n to the
//          clusters of its corners (fp64 atomic adds); the LEADER of every cluster writes the cluster's rows, solving the
//          3 x 3 system itself; a thread per triangle writes the survivors.
//
// Table loads and stores that race are agent-scope atomics; everything compared or copied is an integer or a bit pattern,
// and only the nine quadric sums depend on the order of arrival.  Nothing here allocates, sets or copies memory through
// the runtime.
#include <math.h>

#include "nfl_geom.h"

typedef unsigned long long u64;

#define NC_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull                  // a key has 63 bits
#define NC_NO_SLOT 0xFFFFFFFFu                              // the triangle table has at most 2^31 slots
#define NC_HALF 1048576                                     // 2^20 cells either side of the origin
#define NC_FIX 1073741824.0                                 // 2^30

struct NcGrid {
    double cell;
    double origin[3];
};

// the scratch of count and emit: nc_layout (nfl_geom_layout.h)
typedef NgLayout<NC_REGIONS> NcScratch;

extern "C" size_t nfl_mesh_simplify_bytes(int64_t V, int64_t T) {
    if (!nm_sizes_ok(V, T)) return 0;
    return ng_bytes(nc_layout(V, T));
}

// Checks shared by count and emit.  NFL_OK with V == 0 means: nothing to do.
static int nc_carve(const nfl_mesh_simplify_args* a, NcScratch& S) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    if (!(a->cell > 0.0) || !isfinite(a->cell)) return NFL_EINVAL;
    for (int k = 0; k < 3; ++k)
        if (!isfinite(a->origin[k])) return NFL_EINVAL;
    if (a->placement != NFL_SIMPLIFY_MEAN && a->placement != NFL_SIMPLIFY_QUADRIC) return NFL_EINVAL;
    S = nc_layout(a->n_vertices, a->n_triangles);
    if (a->n_triangles && !a->d_triangles) return NFL_EINVAL;
    if (a->n_vertices == 0) return NFL_OK;
    if (!a->d_vertices || !a->d_cluster) return NFL_EINVAL;
    return ng_carve(S, a->d_scratch, a->scratch_bytes);
}

// --------------------------------------------------------------------------------------------------------------- cells

// The cell of vertex v: pd = the position in fp64, ijk = its cell.  False when the vertex belongs to no cluster.
__device__ __forceinline__ bool nc_cell(const float* pos, i64 v, const NcGrid& G, double pd[3], i64 ijk[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = pos[3 * v + k];
        pd[k] = (double)f;
        const double fi = floor((pd[k] - G.origin[k]) / G.cell);
        ok = ok && isfinite(f) && fi >= -(double)NC_HALF && fi < (double)NC_HALF;       // a NaN fails both comparisons
        ijk[k] = ok ? (i64)fi : 0;
    }
    return ok;
}

__device__ __forceinline__ double nc_centre(const NcGrid& G, int k, i64 i) {
    return G.origin[k] + ((double)i + 0.5) * G.cell;
}

// --------------------------------------------------------------------------------------------------------------- count

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_init_kernel(u64* vkey, int32_t* vmin, u64 cap_v, int32_t* towner,
                                                                       int32_t* tmin, u64 cap_t, i64* totals) {
    const u64 i = (u64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (i < cap_v) {
        vkey[i] = NC_EMPTY_KEY;
        vmin[i] = INT32_MAX;
    }
    if (i < cap_t) {
        towner[i] = -1;
        tmin[i] = INT32_MAX;
    }
    if (i == 0) totals[2] = totals[3] = 0;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_vertices_kernel(const float* pos, i64 V, const NcGrid G, u64* vkey,
                                                                           int32_t* vmin, u64 cap_v, uint32_t* vslot,
                                                                           int32_t* cluster, i64* n_invalid) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool bad = false;
    if (v < V) {
        double pd[3];
        i64 ijk[3];
        bool placed = false;
        u64 s = 0;
        if (nc_cell(pos, v, G, pd, ijk)) {
            const u64 key = (u64)(ijk[0] + NC_HALF) | (u64)(ijk[1] + NC_HALF) << 21 | (u64)(ijk[2] + NC_HALF) << 42;
            const u64 mask = cap_v - 1;
            s = ng_mix(key) & mask;
            for (u64 n = 0; n < cap_v; ++n) {
                u64 cur = NM_LOAD(vkey + s);
                if (cur == NC_EMPTY_KEY) {                  // free when read: claim it, or learn who did
                    cur = atomicCAS(vkey + s, NC_EMPTY_KEY, key);
                    if (cur == NC_EMPTY_KEY) cur = key;
                }
                if (cur == key) {
                    placed = true;
                    break;
                }
                s = (s + 1) & mask;
            }
        }
        if (placed) {
            if (NM_LOAD(vmin + s) > (int32_t)v) atomicMin(vmin + s, (int32_t)v);        // the load spares most of a big cluster's atomics
            vslot[v] = (uint32_t)s;
            cluster[v] = 0;
        } else {
            cluster[v] = -1;
            bad = true;
        }
    }
    ng_count_bad(bad, n_invalid);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_leader_kernel(int32_t* cluster, i64 V, const int32_t* vmin,
                                                                         const uint32_t* vslot, int32_t* flag) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= V) return;
    const int32_t l = cluster[v] < 0 ? -1 : vmin[vslot[v]];
    cluster[v] = l;
    flag[v] = l == v ? 1 : 0;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_map_kernel(const int32_t* tri, const int32_t* cluster, i64 V, i64 T,
                                                                      int32_t* canon, i64* n_out_of_range) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool bad = false;
    if (t < T) {
        const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        int32_t m0 = -1, m1 = -1, m2 = -1;
        if (nm_in_range(a, b, c, V)) {
            const int32_t na = cluster[a], nb = cluster[b], nc = cluster[c];
            if (na >= 0 && nb >= 0 && nc >= 0 && na != nb && nb != nc && na != nc) {
                if (na < nb && na < nc) { m0 = na; m1 = nb; m2 = nc; }
                else if (nb < nc) { m0 = nb; m1 = nc; m2 = na; }
                else { m0 = nc; m1 = na; m2 = nb; }
            }
        } else {
            bad = true;
        }
        canon[3 * t] = m0;
        canon[3 * t + 1] = m1;
        canon[3 * t + 2] = m2;
    }
    ng_count_bad(bad, n_out_of_range);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_triangles_kernel(const int32_t* canon, i64 T, int32_t* towner,
                                                                            int32_t* tmin, u64 cap_t, uint32_t* tslot) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (t >= T) return;
    const int32_t m0 = canon[3 * t], m1 = canon[3 * t + 1], m2 = canon[3 * t + 2];
    bool placed = false;
    u64 s = 0;
    if (m0 >= 0) {
        const u64 mask = cap_t - 1;
        s = ng_mix(ng_mix((u64)(uint32_t)m0 | (u64)(uint32_t)m1 << 32) + (u64)(uint32_t)m2) & mask;
        for (u64 n = 0; n < cap_t; ++n) {
            int32_t cur = NM_LOAD(towner + s);
            if (cur == -1) {
                cur = atomicCAS(towner + s, -1, (int32_t)t);
                if (cur == -1) cur = (int32_t)t;
            }
            // an owner is a triangle of this launch that was not dropped: 0 <= cur < T, its triple written by the launch
            // before; the bounds are checked all the same.  The three words are read without short-circuit, and the slot
            // leaves the loop in `s` under ONE flag: keep this form ("a compiler note").
            const bool known = cur >= 0 && cur < T;
            const i64 o = known ? (i64)cur : t;
            placed = known & (canon[3 * o] == m0) & (canon[3 * o + 1] == m1) & (canon[3 * o + 2] == m2);
            if (placed) break;
            s = (s + 1) & mask;
        }
    }
    if (placed && NM_LOAD(tmin + s) > (int32_t)t) atomicMin(tmin + s, (int32_t)t);
    tslot[t] = placed ? (uint32_t)s : NC_NO_SLOT;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_survive_kernel(const uint32_t* tslot, const int32_t* tmin, i64 T,
                                                                          int32_t* flag) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (t >= T) return;
    const uint32_t s = tslot[t];
    flag[t] = (s != NC_NO_SLOT && tmin[s] == t) ? 1 : 0;
}

extern "C" int nfl_mesh_simplify_count(const nfl_mesh_simplify_args* a, void* stream) {
    NcScratch S;
    const int rc = nc_carve(a, S);
    if (rc != NFL_OK) return rc;
    const i64 V = a->n_vertices, T = a->n_triangles;
    if (V == 0) return NFL_OK;
    if (!a->d_totals) return NFL_EINVAL;
    const NcGrid G = {a->cell, {a->origin[0], a->origin[1], a->origin[2]}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const u64 cap_v = nc_cap(V), cap_t = nc_cap(T), cap = cap_v > cap_t ? cap_v : cap_t;
    u64* vkey = S.get<u64>(NC_VKEY);
    int32_t *vmin = S.get<int32_t>(NC_VMIN), *flag_v = S.get<int32_t>(NC_FLAG_V), *canon = S.get<int32_t>(NC_CANON);
    int32_t *towner = S.get<int32_t>(NC_TOWNER), *tmin = S.get<int32_t>(NC_TMIN), *flag_t = S.get<int32_t>(NC_FLAG_T);
    uint32_t *vslot = S.get<uint32_t>(NC_VSLOT), *tslot = S.get<uint32_t>(NC_TSLOT);
    i64 *rank = S.get<i64>(NC_RANK), *off_t = S.get<i64>(NC_OFF_T), *sums = S.get<i64>(NC_SUMS);
    hipLaunchKernelGGL(nfl_simplify_init_kernel, dim3(nm_grid((i64)cap)), dim3(NM_THREADS), 0, s, vkey, vmin, cap_v, towner,
                       tmin, cap_t, a->d_totals);
    hipLaunchKernelGGL(nfl_simplify_vertices_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_vertices, V, G, vkey, vmin,
                       cap_v, vslot, a->d_cluster, a->d_totals + 3);
    hipLaunchKernelGGL(nfl_simplify_leader_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_cluster, V, vmin, vslot, flag_v);
    nm_scan(flag_v, rank, V, sums, a->d_totals, s);
    nm_rank(a->d_cluster, V, rank, s);
    if (T) {
        hipLaunchKernelGGL(nfl_simplify_map_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_triangles, a->d_cluster, V, T,
                           canon, a->d_totals + 2);
        hipLaunchKernelGGL(nfl_simplify_triangles_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, canon, T, towner, tmin,
                           cap_t, tslot);
        hipLaunchKernelGGL(nfl_simplify_survive_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, tslot, tmin, T, flag_t);
    }
    nm_scan(flag_t, off_t, T, sums, a->d_totals + 1, s);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------- emit

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_zero_kernel(i64 n_out, int32_t* count, i64* fixed, double* quadric,
                                                                       int with_quadric) {
    const i64 c = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (c >= n_out) return;
    count[c] = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) fixed[9 * c + k] = 0;
    if (with_quadric) {
#pragma unroll
        for (int k = 0; k < 9; ++k) quadric[9 * c + k] = 0.0;
    }
}

__device__ __forceinline__ void nc_add_fixed(i64* dst, double x) {
    atomicAdd(reinterpret_cast<u64*>(dst), (u64)llrint(x * NC_FIX));                   // two's complement: the signed sum
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_accumulate_kernel(const float* pos, const float* nrm, const float* col,
                                                                             const int32_t* cluster, i64 V, i64 n_out, const NcGrid G,
                                                                             int32_t* count, i64* fixed) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= V) return;
    const int32_t c = cluster[v];
    if (c < 0 || c >= n_out) return;
    double pd[3];
    i64 ijk[3];
    if (!nc_cell(pos, v, G, pd, ijk)) return;
    atomicAdd(count + c, 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        nc_add_fixed(fixed + 9 * (i64)c + k, (pd[k] - nc_centre(G, k, ijk[k])) / G.cell);
        const float n = nrm[3 * v + k];
        if (isfinite(n)) nc_add_fixed(fixed + 9 * (i64)c + 3 + k, (double)n);
        if (col) {
            const float q = col[3 * v + k];
            if (isfinite(q)) nc_add_fixed(fixed + 9 * (i64)c + 6 + k, (double)q);
        }
    }
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_quadric_kernel(const float* pos, const int32_t* tri, const int32_t* cluster,
                                                                          i64 V, i64 T, i64 n_out, const NcGrid G, double* quadric) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (t >= T) return;
    const int32_t idx[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    if (!nm_in_range(idx[0], idx[1], idx[2], V)) return;
    double p[3][3];
    i64 ijk[3][3];
    int32_t cl[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        cl[j] = cluster[idx[j]];
        if (cl[j] < 0 || cl[j] >= n_out || !nc_cell(pos, idx[j], G, p[j], ijk[j])) return;
    }
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double len = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
    const double area = 0.5 * len;
    if (!(area > 0.0) || !isfinite(area)) return;
    const double n[3] = {cr[0] / len, cr[1] / len, cr[2] / len};
    const double w = area / (G.cell * G.cell);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double u0[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) u0[k] = (p[0][k] - nc_centre(G, k, ijk[j][k])) / G.cell;
        const double d = -((n[0] * u0[0] + n[1] * u0[1]) + n[2] * u0[2]);
        double* q = quadric + 9 * (i64)cl[j];
        atomicAdd(q + 0, w * n[0] * n[0]);
        atomicAdd(q + 1, w * n[0] * n[1]);
        atomicAdd(q + 2, w * n[0] * n[2]);
        atomicAdd(q + 3, w * n[1] * n[1]);
        atomicAdd(q + 4, w * n[1] * n[2]);
        atomicAdd(q + 5, w * n[2] * n[2]);
        atomicAdd(q + 6, w * d * n[0]);
        atomicAdd(q + 7, w * d * n[1]);
        atomicAdd(q + 8, w * d * n[2]);
    }
}

// (A + mu I) u = mu ub - b by cofactors; false when there is nothing to solve or the result is not finite
__device__ __forceinline__ bool nc_solve(const double* q, const double ub[3], double u[3]) {
    const double tr = (q[0] + q[3]) + q[5];
    if (tr == 0.0) return false;
    const double mu = NFL_SIMPLIFY_LAMBDA * tr;
    const double m00 = q[0] + mu, m01 = q[1], m02 = q[2], m11 = q[3] + mu, m12 = q[4], m22 = q[5] + mu;
    const double r0 = mu * ub[0] - q[6], r1 = mu * ub[1] - q[7], r2 = mu * ub[2] - q[8];
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    u[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
    u[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
    u[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
    return isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_simplify_finish_kernel(const int32_t* flag, const int32_t* cluster, i64 V, i64 n_out,
                                                                         const NcGrid G, const int32_t* count, const i64* fixed,
                                                                         const double* quadric, const NgRows R) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= V || !flag[v]) return;                         // the leader of a cluster writes the cluster's rows
    const i64 c = cluster[v];
    if (c < 0 || c >= n_out) return;
    const int32_t n = count[c];
    if (n <= 1) {                                           // alone: its own bits
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            R.out[0][3 * c + k] = R.in[0][3 * v + k];
            R.out[1][3 * c + k] = R.in[1][3 * v + k];
            if (R.in[2]) R.out[2][3 * c + k] = R.in[2][3 * v + k];
        }
        return;
    }
    double pd[3];
    i64 ijk[3];
    if (!nc_cell(R.in[0], v, G, pd, ijk)) return;
    const i64* f = fixed + 9 * c;
    const double scale = (double)n * NC_FIX;
    double ub[3], u[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = ub[k] = (double)f[k] / scale;
    double uq[3];
    if (quadric && nc_solve(quadric + 9 * c, ub, uq)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = fmin(fmax(uq[k], -0.5), 0.5);
    }
    const double s[3] = {(double)f[3], (double)f[4], (double)f[5]};
    const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        R.out[0][3 * c + k] = (float)(nc_centre(G, k, ijk[k]) + G.cell * u[k]);
        R.out[1][3 * c + k] = len > 0.0 ? (float)(s[k] / len) : 0.0f;
        if (R.in[2]) R.out[2][3 * c + k] = (float)((double)f[6 + k] / scale);
    }
}

extern "C" int nfl_mesh_simplify_emit(const nfl_mesh_simplify_args* a, void* stream) {
    NcScratch S;
    const int rc = nc_carve(a, S);
    if (rc != NFL_OK) return rc;
    const i64 V = a->n_vertices, T = a->n_triangles, Vo = a->n_out_vertices, To = a->n_out_triangles;
    if (V == 0) return NFL_OK;
    if (Vo < 0 || To < 0 || Vo > V || To > T) return NFL_EINVAL;
    if (Vo == 0 && To == 0) return NFL_OK;
    if (Vo && (!a->d_normals || !a->d_out_vertices || !a->d_out_normals || (a->d_colors && !a->d_out_colors))) return NFL_EINVAL;
    if (To && !a->d_out_triangles) return NFL_EINVAL;
    const NcGrid G = {a->cell, {a->origin[0], a->origin[1], a->origin[2]}};
    const int with_quadric = a->placement == NFL_SIMPLIFY_QUADRIC;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Vo) {
        int32_t* count = S.get<int32_t>(NC_COUNT);
        i64* fixed = S.get<i64>(NC_FIXED);
        double* quadric = S.get<double>(NC_QUADRIC);
        const NgRows R = {{a->d_vertices, a->d_normals, a->d_colors}, {a->d_out_vertices, a->d_out_normals, a->d_out_colors}};
        hipLaunchKernelGGL(nfl_simplify_zero_kernel, dim3(nm_grid(Vo)), dim3(NM_THREADS), 0, s, Vo, count, fixed, quadric, with_quadric);
        hipLaunchKernelGGL(nfl_simplify_accumulate_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_vertices, a->d_normals,
                           a->d_colors, a->d_cluster, V, Vo, G, count, fixed);
        if (with_quadric && T)
            hipLaunchKernelGGL(nfl_simplify_quadric_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_vertices, a->d_triangles,
                               a->d_cluster, V, T, Vo, G, quadric);
        hipLaunchKernelGGL(nfl_simplify_finish_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, S.get<int32_t>(NC_FLAG_V), a->d_cluster, V, Vo, G, count,
                           fixed, with_quadric ? quadric : nullptr, R);
    }
    if (To) hipLaunchKernelGGL(nfl_mesh_emit_triangles_kernel<int32_t>, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, S.get<int32_t>(NC_FLAG_T), S.get<i64>(NC_OFF_T),
                               a->d_triangles, a->d_cluster, V, T, Vo, To, a->d_out_triangles);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
