// nfl_meshcast.hip -- rays against a triangle mesh on the device (include/nerf_fl_amd.h, "mesh cast"): where an arbitrary ray
// first hits a mesh, whether it hits it at all, and how open the hemisphere over a point is.  DESIGN.md section 36.
//
//   test    THE RAY TEST of the header, written once (nc_test): Moeller-Trumbore in fp64, the hit point rounded to fp32 and
//           clamped into the triangle's box, and the consistency condition that ties the point to the ray.
//   walk    THE WALK of the header, written once (nc_walk): the slabs of grid cells along the ray's major axis, in each the
//           cells the ray can touch on the other two axes, until no later slab can hold an earlier hit.  Every bound is
//           widened by E, a per-ray constant above every tolerance the consistency condition can grant inside the grid's box.
//   cast    a thread per ray.  Brute: the workgroup stages 256 triangles' corners in LDS (nt_tiles, as nfl_mesh_closest does) and
//           every thread tries them all.  Grid: the thread walks.  Rays of a frame arrive in pixel order, so neighbouring lanes
//           walk neighbouring rows.  First-hit mode keeps (t, triangle) only and tests the answer once more for its point.
//   occlusion   a wave per point: lane l casts directions l, l + 64, ... in any-hit mode, the hits are counted by ballot.
//   solid   ("mesh solid") THE CROSSINGS of a ray, a thread per ray: the same walk run to its end, every
//           accepted hit counted in the cell of its own point alone (nc_walk_count); and INSIDE, a thread per point: the parity
//           of the crossings along the header's fixed directions, one direction after the other for the whole wave.
//
// No atomics, no scratch buffer, nothing that depends on an order.  The grid (NdGrid, nd_cellf, nd_face), the triangle fetch and
// the hash are nfl_geom.h's, the pointer checks nfl_geom_layout.h's: a ray meets the cells nfl_trigrid_emit filled.  The view
// of the mesh with its grid (NtMesh), the read of a row and the staged tiles are nfl_trigrid.h's, shared with nfl_meshdist.
#include <math.h>

#include "nfl_trigrid.h"

typedef unsigned long long u64;

#define NC_MAX_DIRECTIONS 4096
#define NC_ATTEMPTS 8
#define NC_2M19 1.9073486328125e-06                         // 2^-19
#define NC_2M20 9.5367431640625e-07                         // 2^-20
#define NC_2M23 1.1920928955078125e-07                      // 2^-23
#define NC_2M40 9.094947017729282e-13                       // 2^-40
#define NC_2M148 0x1p-148                                   // twice the smallest fp32 subnormal

#ifdef NFL_MESHCAST_COUNT_TESTS
// a diagnostic build (make variant VFLAGS=-DNFL_MESHCAST_COUNT_TESTS=1 VTU=nfl_meshcast) counts what the walk does:
// [0] ray-triangle tests, [1] cells read, [2] rays walked.  tests/time_raycast.py reads them; the product never has them.
__device__ u64 nc_debug_counts[3];
extern "C" int nfl_meshcast_debug_counts(u64* out3, int reset) {
    const u64 zero[3] = {0, 0, 0};
    if (out3 && hipMemcpyFromSymbol(out3, HIP_SYMBOL(nc_debug_counts), sizeof zero) != hipSuccess) return NFL_ELAUNCH;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(nc_debug_counts), zero, sizeof zero) != hipSuccess) return NFL_ELAUNCH;
    return NFL_OK;
}
#define NC_DEBUG_ADD(k, n) atomicAdd(&nc_debug_counts[k], (u64)(n))
#else
#define NC_DEBUG_ADD(k, n)
#endif

struct NcRay {
    double o[3], d[3];
    float near, far;
};

struct NcBox {                                              // the closed box of the grid in fp64: the faces 0 and dims[k]
    double lo[3], hi[3];
};

struct NcHit {
    float tf, bary[3], q[3];
};

struct NcBest {
    float tf;
    int32_t t;
};

// ---------------------------------------------------------------------------------------------------------- the ray test

__device__ __forceinline__ double nc_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void nc_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// a ray of 8 floats; false when it can hit nothing: a non-finite origin or direction, a NaN bound, d == 0, near > far
__device__ __forceinline__ bool nc_ray(const float* o, const float* d, float near, float far, NcRay& R) {
    bool ok = near <= far;                                  // a NaN fails
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ok = ok && ng_is_finite(o[k]) && ng_is_finite(d[k]);
        R.o[k] = (double)o[k], R.d[k] = (double)d[k];
    }
    R.near = near, R.far = far;
    return ok && !(d[0] == 0.f && d[1] == 0.f && d[2] == 0.f);
}

__device__ __forceinline__ NcBox nc_box(const NdGrid& G) {
    NcBox B;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double S;
        nd_face(G.lo[k], G.cell, 0, &B.lo[k], &S);
        nd_face(G.lo[k], G.cell, G.dims[k], &B.hi[k], &S);
    }
    return B;
}

// THE RAY TEST of the header: whether the ray hits the usable triangle (a, b, c), and then tf, the corner weights and qf
__device__ __forceinline__ bool nc_test(const NcRay& R, const NcBox& B, bool boxed, const float* a, const float* b, const float* c,
                                        NcHit& H) {
    double A[3], e1[3], e2[3], p[3], s[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = (double)a[k];
        e1[k] = (double)b[k] - A[k];
        e2[k] = (double)c[k] - A[k];
        s[k] = R.o[k] - A[k];
    }
    nc_cross(R.d, e2, p);
    const double det = nc_dot(e1, p);
    if (det == 0.0 || det != det) return false;             // parallel, degenerate, or not a number
    const double u = nc_dot(s, p) / det;
    nc_cross(s, e1, q);
    const double v = nc_dot(R.d, q) / det, t = nc_dot(e2, q) / det;
    if (!(u >= 0.0 && v >= 0.0 && u + v <= 1.0)) return false;
    const float tf = (float)t;
    if (!(ng_is_finite(tf) && R.near <= tf && tf <= R.far)) return false;
    double m = 0.0, r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double Q = (A[k] + u * e1[k]) + v * e2[k], td = t * R.d[k];
        const float mn = fminf(fminf(a[k], b[k]), c[k]), mx = fmaxf(fmaxf(a[k], b[k]), c[k]);
        float qf = (float)Q;
        qf = qf < mn ? mn : (qf > mx ? mx : qf);            // a NaN stays, and fails below
        H.q[k] = qf;
        r[k] = R.o[k] + td;
        m = fmax(m, fabs(R.o[k]) + fabs(td));
    }
    const double tol = NC_2M20 * m;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double qd = (double)H.q[k];
        ok = ok && fabs(r[k] - qd) <= tol;                  // THE CONSISTENCY CONDITION
        if (boxed) ok = ok && qd >= B.lo[k] && qd <= B.hi[k];
    }
    if (!ok) return false;
    H.tf = tf;
    H.bary[0] = (float)((1.0 - u) - v), H.bary[1] = (float)u, H.bary[2] = (float)v;
    return true;
}

__device__ __forceinline__ void nc_try(NcBest& best, const NcRay& R, const NcBox& B, bool boxed, int32_t t, const float* a,
                                       const float* b, const float* c) {
    NcHit H;
    NC_DEBUG_ADD(0, 1);
    if (nc_test(R, B, boxed, a, b, c, H) && (H.tf < best.tf || (H.tf == best.tf && t < best.t))) best.tf = H.tf, best.t = t;
}

// --------------------------------------------------------------------------------------------------------------- the walk

template <typename T>
__device__ __forceinline__ T nc_pick(const T* v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

// x (finite) rounded to fp32 towards -inf / +inf
__device__ __forceinline__ float nc_down(double x) {
    const float f = (float)x;
    return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
__device__ __forceinline__ float nc_up(double x) {
    const float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
}

// the parameter at which the ray can enter (exit) slab i of its major axis: faces F with their slack S, plus E
__device__ __forceinline__ void nc_slab(float lo32, float cell, int i, bool up, double om, double dm, double E, double* te,
                                        double* tx) {
    double F0, S0, F1, S1;
    nd_face(lo32, cell, i, &F0, &S0);
    nd_face(lo32, cell, i + 1, &F1, &S1);
    const double lo = (F0 - S0) - E, hi = (F1 + S1) + E;
    *te = ((up ? lo : hi) - om) / dm;
    *tx = ((up ? hi : lo) - om) / dm;
}

// the cells [c0, c1] of axis k that the ray can touch for parameters in [ta, tb]
__device__ __forceinline__ void nc_span(float lo, float cell, int n, double o, double d, double ta, double tb, double E, int* c0,
                                        int* c1) {
    const double xa = o + ta * d, xb = o + tb * d;
    *c0 = nd_cellf(nc_down(fmin(xa, xb) - E), lo, cell, n);
    *c1 = nd_cellf(nc_up(fmax(xa, xb) + E), lo, cell, n);
}

// THE WALK of the header, written once for what is done along it.  attempt(t, a, b, c, x, y, z) is handed every usable triangle
// of every row read, with the row's cell, and says whether the walk is over; settled(te) says whether nothing at a parameter
// from te on can change the answer.  Both are lambdas marked NT_INLINE.
template <typename Try, typename Settled>
__device__ __forceinline__ void nc_walk(const NcRay& R, const NcBox& B, const NtMesh& M, Try&& attempt, Settled&& settled) {
    const NdGrid& G = M.G;
    int m = 0;
    double am = fabs(R.d[0]);
    if (fabs(R.d[1]) > am) m = 1, am = fabs(R.d[1]);
    if (fabs(R.d[2]) > am) m = 2;
    const int k1 = m == 2 ? 0 : m + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    const double om = nc_pick(R.o, m), dm = nc_pick(R.d, m), o1 = nc_pick(R.o, k1), d1 = nc_pick(R.d, k1);
    const double o2 = nc_pick(R.o, k2), d2 = nc_pick(R.d, k2);
    const int nm = nc_pick(G.dims, m), n1 = nc_pick(G.dims, k1), n2 = nc_pick(G.dims, k2);
    const float lm = nc_pick(G.lo, m), l1 = nc_pick(G.lo, k1), l2 = nc_pick(G.lo, k2);
    double omax = 0.0, bmax = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        omax = fmax(omax, fabs(R.o[k]));
        bmax = fmax(bmax, fmax(fabs(B.lo[k]), fabs(B.hi[k])));
    }
    const double E = NC_2M19 * (2.0 * omax + bmax);
    const double tn = (double)R.near - (fabs((double)R.near) * NC_2M23 + NC_2M148);
    const double tf = (double)R.far + (fabs((double)R.far) * NC_2M23 + NC_2M148);
    const bool up = dm > 0.0;
    // the first slab that can matter, from below: the test of every slab's own interval is what decides
    double Fn, Sn;
    nd_face(lm, G.cell, nm, &Fn, &Sn);
    const double r0 = om + tn * dm, Et = E + Sn, lom = nc_pick(B.lo, m);
    const double guess = up ? floor(((r0 - Et) - lom) / (double)G.cell) - 2.0 : floor(((r0 + Et) - lom) / (double)G.cell) + 2.0;
    int i = (int)fmin(fmax(guess, 0.0), (double)(nm - 1));
    NC_DEBUG_ADD(2, 1);
    for (; up ? i < nm : i >= 0; i += up ? 1 : -1) {
        double te, tx;
        nc_slab(lm, G.cell, i, up, om, dm, E, &te, &tx);
        if (te > tf) return;                                // this slab and every later one begin beyond far
        // every hit of this slab and the later ones has t >= te
        if (settled(te)) return;
        if (tx < tn) continue;                              // the slab ends before near
        const double ta = fmax(te, tn), tb = fmin(tx, tf);
        int a0, a1, b0, b1;
        nc_span(l1, G.cell, n1, o1, d1, ta, tb, E, &a0, &a1);
        nc_span(l2, G.cell, n2, o2, d2, ta, tb, E, &b0, &b1);
        for (int j2 = b0; j2 <= b1; ++j2)
            for (int j1 = a0; j1 <= a1; ++j1) {
                const int x = m == 0 ? i : (m == 1 ? j2 : j1), y = m == 0 ? j1 : (m == 1 ? i : j2);
                const int z = m == 0 ? j2 : (m == 1 ? j1 : i);
                NC_DEBUG_ADD(1, 1);
                bool over = false;
                nt_row(M, ((i64)z * G.dims[1] + y) * G.dims[0] + x,
                       [&](int32_t t, const float* ca, const float* cb, const float* cc) NT_INLINE {
                           return over = attempt(t, ca, cb, cc, x, y, z);
                       });
                if (over) return;
            }
    }
}

// the walk for THE ANSWER.  ANY: stops at the first accepted hit.
template <bool ANY>
__device__ __forceinline__ void nc_walk_best(NcBest& best, const NcRay& R, const NcBox& B, const NtMesh& M) {
    nc_walk(R, B, M,
            [&](int32_t t, const float* ca, const float* cb, const float* cc, int, int, int) NT_INLINE {
                nc_try(best, R, B, true, t, ca, cb, cc);                // where rows are walked the box rule holds
                return ANY && best.t >= 0;
            },
            // nothing from te on can win or tie
            [&](double te) NT_INLINE { return best.t >= 0 && best.tf < nc_down(te - fabs(te) * NC_2M40); });
}

// the walk for THE CROSSINGS of "mesh solid": no early stop, and THE ONCE-ONLY RULE -- a triangle is listed in every cell of its
// bounding box and the walk reads several of them, so an accepted hit counts in the cell of its own point qf alone
__device__ __forceinline__ int32_t nc_walk_count(const NcRay& R, const NcBox& B, const NtMesh& M) {
    const NdGrid& G = M.G;
    int32_t count = 0;
    nc_walk(R, B, M,
            [&](int32_t, const float* ca, const float* cb, const float* cc, int x, int y, int z) NT_INLINE {
                NcHit H;
                NC_DEBUG_ADD(0, 1);
                if (nc_test(R, B, true, ca, cb, cc, H) && nd_cellf(H.q[0], G.lo[0], G.cell, G.dims[0]) == x &&
                    nd_cellf(H.q[1], G.lo[1], G.cell, G.dims[1]) == y && nd_cellf(H.q[2], G.lo[2], G.cell, G.dims[2]) == z) ++count;
                return false;
            },
            [](double) NT_INLINE { return false; });
    return count;
}

// ------------------------------------------------------------------------------------------------------------------ cast

struct NcCast {
    const float* rays;
    i64 n;
    NtMesh M;
    int boxed;                                              // the box rule holds: always with rows, in brute mode with a box
    float* t;
    int32_t* triangle;
    float *bary, *point;
};

template <bool GRID, bool ANY>
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_cast_kernel(const NcCast a) {
    const i64 n = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    const bool mine = n < a.n;
    float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mine) {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = a.rays[8 * n + k];
    }
    NcRay R;
    const bool asks = nc_ray(w, w + 3, w[6], w[7], R) && mine;
    const bool boxed = a.boxed != 0;
    NcBox B = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (boxed) B = nc_box(a.M.G);
    NcBest best = {INFINITY, -1};
    if (GRID) {
        if (asks) nc_walk_best<ANY>(best, R, B, a.M);
    } else {
        const auto still = [&]() NT_INLINE { return asks && !(ANY && best.t >= 0); };
        const auto attempt = [&](int32_t t, const float* ta, const float* tb, const float* tc) NT_INLINE {
            nc_try(best, R, B, boxed, t, ta, tb, tc);
        };
        nt_tiles(a.M, still, attempt);
    }
    if (!mine) return;
    if (ANY) {
        a.t[n] = best.t >= 0 ? 0.f : INFINITY;
        return;
    }
    // the answer once more, for its corner weights and its point: the test is a function of the ray and the triangle
    NcHit H;
    float ca[3], cb[3], cc[3];
    const bool hit = best.t >= 0 && nm_corners(a.M.ver, a.M.tri, a.M.V, best.t, ca, cb, cc) && nc_test(R, B, boxed, ca, cb, cc, H);
    a.t[n] = hit ? H.tf : INFINITY;
    if (a.triangle) a.triangle[n] = hit ? best.t : -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (a.bary) a.bary[3 * n + k] = hit ? H.bary[k] : NAN;
        if (a.point) a.point[3 * n + k] = hit ? H.q[k] : NAN;
    }
}

// the grid part of a call: with rows what nfl_mesh_closest asks of them; without, all zeros or the box of a grid.  `need`: the
// call cannot do without rows
static bool nc_grid_args_ok(const int64_t* d_offsets, const int32_t* d_entries, int64_t n_entries, const float* lo, float cell,
                            const int32_t* dims, bool need) {
    const bool none = dims[0] == 0 && dims[1] == 0 && dims[2] == 0;
    if (!d_offsets) return !need && (none || nd_grid_ok(lo, cell, dims));              // brute mode, with or without the box
    return nt_rows_ok(d_offsets, d_entries, n_entries, lo, cell, dims);
}

// the mesh and grid part of a call as the kernels see it: the rows where they are given, the grid's box where one is given
static NtMesh nc_view(const float* d_vertices, const int32_t* d_triangles, int64_t n_vertices, int64_t n_triangles,
                      const int64_t* d_offsets, const int32_t* d_entries, int64_t n_entries, const float* lo, float cell,
                      const int32_t* dims) {
    return {d_vertices, d_triangles, n_vertices, n_triangles, d_offsets, d_entries, d_offsets ? n_entries : 0,
            dims[0] != 0 ? nd_grid_of(lo, cell, dims) : NdGrid{{0.f, 0.f, 0.f}, 1.f, {1, 1, 1}}};
}

extern "C" int nfl_mesh_cast(const float* d_rays, int64_t n_rays, const float* d_vertices, const int32_t* d_triangles,
                             int64_t n_vertices, int64_t n_triangles, const int64_t* d_offsets, const int32_t* d_entries,
                             int64_t n_entries, float lo_x, float lo_y, float lo_z, float cell, int32_t nx, int32_t ny, int32_t nz,
                             int32_t mode, float* d_t, int32_t* d_triangle, float* d_bary, float* d_point, void* stream) {
    if (n_rays < 0 || n_rays > ND_MAX_ENTRIES) return NFL_EINVAL;
    if (!nd_mesh_ok(d_vertices, d_triangles, n_vertices, n_triangles)) return NFL_EINVAL;
    if (mode != NFL_CAST_FIRST && mode != NFL_CAST_ANY) return NFL_EINVAL;
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    if (!nc_grid_args_ok(d_offsets, d_entries, n_entries, lo, cell, dims, false)) return NFL_EINVAL;
    if (n_rays == 0) return NFL_OK;
    if (ng_bad(d_rays, 4) || ng_bad(d_t, 4)) return NFL_EINVAL;
    if (ng_misaligned(d_triangle, 4) || ng_misaligned(d_bary, 4) || ng_misaligned(d_point, 4)) return NFL_EINVAL;
    const bool grid = d_offsets != nullptr;
    NcCast a = {d_rays, n_rays, nc_view(d_vertices, d_triangles, n_vertices, n_triangles, d_offsets, d_entries, n_entries, lo, cell, dims),
                nx != 0 ? 1 : 0, d_t, d_triangle, d_bary, d_point};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 blocks(nm_grid(n_rays)), threads(NM_THREADS);
    if (grid && mode == NFL_CAST_FIRST) hipLaunchKernelGGL((nfl_mesh_cast_kernel<true, false>), blocks, threads, 0, s, a);
    else if (grid) hipLaunchKernelGGL((nfl_mesh_cast_kernel<true, true>), blocks, threads, 0, s, a);
    else if (mode == NFL_CAST_FIRST) hipLaunchKernelGGL((nfl_mesh_cast_kernel<false, false>), blocks, threads, 0, s, a);
    else hipLaunchKernelGGL((nfl_mesh_cast_kernel<false, true>), blocks, threads, 0, s, a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ------------------------------------------------------------------------------------------------------------- occlusion

struct NcOcc {
    const float *points, *normals;
    i64 n;
    NtMesh M;
    int32_t K;
    float radius, bias;
    u64 seed;
    int32_t* hits;
    float* open;
};

#define NC_2M23F 1.1920928955078125e-07f                    // 2^-23

// DIRECTION j of point i of the header: a point of the unit disc by rejection, lifted onto the hemisphere round n
__device__ __forceinline__ void nc_direction(u64 seed, i64 i, int32_t j, const float* n, float* d) {
    const u64 h = ng_mix(ng_mix(ng_mix(seed) + (u64)i) + (u64)j);
    float x = 0.f, y = 0.f, s = 0.f;
    for (int attempt = 0; attempt < NC_ATTEMPTS; ++attempt) {
        const u64 ha = ng_mix(h + (u64)(attempt + 1));
        const float cx = (float)(ha >> 40) * NC_2M23F - 1.f, cy = (float)((ha >> 16) & 0xFFFFFFull) * NC_2M23F - 1.f;
        const float cs = cx * cx + cy * cy;
        if (cs < 1.f) {
            x = cx, y = cy, s = cs;
            break;
        }
    }
    const float z = sqrtf(1.f - s);
    // the branchless orthonormal basis of Duff et al. 2017
    const float sign = copysignf(1.f, n[2]);
    const float a = -1.f / (sign + n[2]), b = (n[0] * n[1]) * a;
    const float t1[3] = {1.f + ((sign * n[0]) * n[0]) * a, sign * b, -(sign * n[0])};
    const float t2[3] = {b, sign + (n[1] * n[1]) * a, -n[1]};
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (x * t1[k] + y * t2[k]) + z * n[k];
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_occlusion_kernel(const NcOcc a) {
    const i64 i = (i64)blockIdx.x * (NM_THREADS / 64) + (threadIdx.x >> 6);              // a wave per point
    const int lane = threadIdx.x & 63;
    if (i >= a.n) return;
    float p[3], n[3], o[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = a.points[3 * i + k], n[k] = a.normals[3 * i + k];
        ok = ok && ng_is_finite(p[k]) && ng_is_finite(n[k]);
        o[k] = p[k] + a.bias * n[k];
    }
    ok = ok && !(n[0] == 0.f && n[1] == 0.f && n[2] == 0.f);
    if (!ok) {
        if (lane == 0) a.hits[i] = -1, a.open[i] = NAN;
        return;
    }
    const NcBox B = nc_box(a.M.G);
    int32_t hits = 0;
    for (int32_t base = 0; base < a.K; base += 64) {        // the same trips for every lane: a ballot inside
        const int32_t j = base + lane;
        bool hit = false;
        if (j < a.K) {
            float d[3];
            nc_direction(a.seed, i, j, n, d);
            NcRay R;
            NcBest best = {INFINITY, -1};
            if (nc_ray(o, d, 0.f, a.radius, R)) nc_walk_best<true>(best, R, B, a.M);
            hit = best.t >= 0;
        }
        hits += (int32_t)__popcll(__ballot(hit));
    }
    if (lane == 0) a.hits[i] = hits, a.open[i] = (float)(a.K - hits) / (float)a.K;
}

extern "C" int nfl_mesh_occlusion(const float* d_points, const float* d_normals, int64_t n, const float* d_vertices,
                                  const int32_t* d_triangles, int64_t n_vertices, int64_t n_triangles, const int64_t* d_offsets,
                                  const int32_t* d_entries, int64_t n_entries, float lo_x, float lo_y, float lo_z, float cell,
                                  int32_t nx, int32_t ny, int32_t nz, int32_t n_directions, float radius, float bias, uint64_t seed,
                                  int32_t* d_hits, float* d_open, void* stream) {
    if (n < 0 || n > ND_MAX_ENTRIES || n_directions < 1 || n_directions > NC_MAX_DIRECTIONS) return NFL_EINVAL;
    if (!nd_mesh_ok(d_vertices, d_triangles, n_vertices, n_triangles)) return NFL_EINVAL;
    if (!(radius > 0.f) || !(bias >= 0.f) || !ng_finite(bias)) return NFL_EINVAL;       // NaN included
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    if (!nc_grid_args_ok(d_offsets, d_entries, n_entries, lo, cell, dims, true)) return NFL_EINVAL;
    if (n == 0) return NFL_OK;
    if (ng_bad(d_points, 4) || ng_bad(d_normals, 4) || ng_bad(d_hits, 4) || ng_bad(d_open, 4)) return NFL_EINVAL;
    NcOcc a = {d_points, d_normals, n, {d_vertices, d_triangles, n_vertices, n_triangles, d_offsets, d_entries, n_entries,
                                        nd_grid_of(lo, cell, dims)},
               n_directions, radius, bias, seed, d_hits, d_open};
    hipLaunchKernelGGL(nfl_mesh_occlusion_kernel, dim3((unsigned)ng_cdiv(n, NM_THREADS / 64)), dim3(NM_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ----------------------------------------------------------------------------------------------------------------- solid

// THE CROSSINGS of the header ("mesh solid"): a thread per ray, as the cast.  Brute: every usable triangle is tried once, which
// is the definition.  Grid: the count-mode walk, which returns the same integer.
struct NcCross {
    const float* rays;
    i64 n;
    NtMesh M;
    int boxed;
    int32_t* count;
};

template <bool GRID>
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_crossings_kernel(const NcCross a) {
    const i64 n = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    const bool mine = n < a.n;
    float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (mine) {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = a.rays[8 * n + k];
    }
    NcRay R;
    const bool asks = nc_ray(w, w + 3, w[6], w[7], R) && mine;
    const bool boxed = a.boxed != 0;
    NcBox B = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (boxed) B = nc_box(a.M.G);
    int32_t count = 0;
    if (GRID) {
        if (asks) count = nc_walk_count(R, B, a.M);
    } else {
        nt_tiles(a.M, [&]() NT_INLINE { return asks; },
                 [&](int32_t, const float* ta, const float* tb, const float* tc) NT_INLINE {
                     NcHit H;
                     NC_DEBUG_ADD(0, 1);
                     if (nc_test(R, B, boxed, ta, tb, tc, H)) ++count;
                 });
    }
    if (mine) a.count[n] = count;
}

extern "C" int nfl_mesh_crossings(const float* d_rays, int64_t n_rays, const float* d_vertices, const int32_t* d_triangles,
                                  int64_t n_vertices, int64_t n_triangles, const int64_t* d_offsets, const int32_t* d_entries,
                                  int64_t n_entries, float lo_x, float lo_y, float lo_z, float cell, int32_t nx, int32_t ny,
                                  int32_t nz, int32_t* d_count, void* stream) {
    if (n_rays < 0 || n_rays > ND_MAX_ENTRIES) return NFL_EINVAL;
    if (!nd_mesh_ok(d_vertices, d_triangles, n_vertices, n_triangles)) return NFL_EINVAL;
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    if (!nc_grid_args_ok(d_offsets, d_entries, n_entries, lo, cell, dims, false)) return NFL_EINVAL;
    if (n_rays == 0) return NFL_OK;
    if (ng_bad(d_rays, 4) || ng_bad(d_count, 4)) return NFL_EINVAL;
    NcCross a = {d_rays, n_rays, nc_view(d_vertices, d_triangles, n_vertices, n_triangles, d_offsets, d_entries, n_entries, lo, cell, dims),
                 nx != 0 ? 1 : 0, d_count};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 blocks(nm_grid(n_rays)), threads(NM_THREADS);
    if (d_offsets) hipLaunchKernelGGL(nfl_mesh_crossings_kernel<true>, blocks, threads, 0, s, a);
    else hipLaunchKernelGGL(nfl_mesh_crossings_kernel<false>, blocks, threads, 0, s, a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// INSIDE of the header: a thread per point, direction j of THE DIRECTIONS after direction j - 1.  Every lane of a wave walks
// the same direction at the same time, from a neighbouring point when the points are a lattice's: the coherent case.  The
// table is read by j from constant memory; the parities are the bits of one word, so nothing is indexed in registers.
__device__ const float nc_directions[NFL_SOLID_MAX_DIRECTIONS][3] = NFL_SOLID_DIRECTIONS;

struct NcSolid {
    const float* points;
    i64 n;
    NtMesh M;
    int boxed;
    int32_t K;
    uint8_t *votes, *inside;
};

template <bool GRID>
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_inside_kernel(const NcSolid a) {
    const i64 n = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    const bool mine = n < a.n;
    float p[3] = {0.f, 0.f, 0.f};
    if (mine) {
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = a.points[3 * n + k];
    }
    const bool finite = ng_is_finite(p[0]) && ng_is_finite(p[1]) && ng_is_finite(p[2]);
    const bool asks = mine && finite;
    const bool boxed = a.boxed != 0;
    NcBox B = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (boxed) B = nc_box(a.M.G);
    const auto ray = [&](int j, NcRay& R) NT_INLINE {
        const float d[3] = {nc_directions[j][0], nc_directions[j][1], nc_directions[j][2]};
        return nc_ray(p, d, 0.f, INFINITY, R);
    };
    uint32_t odd = 0;                                       // bit j: direction j has an odd crossings count
    if (GRID) {
        for (int j = 0; j < a.K; ++j) {
            NcRay R;
            if (ray(j, R) && asks) odd |= (uint32_t)(nc_walk_count(R, B, a.M) & 1) << j;
        }
    } else {
        nt_tiles(a.M, [&]() NT_INLINE { return asks; },
                 [&](int32_t, const float* ta, const float* tb, const float* tc) NT_INLINE {
                     for (int j = 0; j < a.K; ++j) {
                         NcRay R;
                         NcHit H;
                         NC_DEBUG_ADD(0, 1);
                         if (ray(j, R) && nc_test(R, B, boxed, ta, tb, tc, H)) odd ^= 1u << j;
                     }
                 });
    }
    if (!mine) return;
    const int votes = __popc(odd);
    a.votes[n] = finite ? (uint8_t)votes : (uint8_t)255;
    if (a.inside) a.inside[n] = finite && 2 * votes > a.K ? 1 : 0;
}

extern "C" int nfl_mesh_inside(const float* d_points, int64_t n, const float* d_vertices, const int32_t* d_triangles,
                               int64_t n_vertices, int64_t n_triangles, const int64_t* d_offsets, const int32_t* d_entries,
                               int64_t n_entries, float lo_x, float lo_y, float lo_z, float cell, int32_t nx, int32_t ny, int32_t nz,
                               int32_t n_directions, void* d_votes, void* d_inside, void* stream) {
    if (n < 0 || n > ND_MAX_ENTRIES) return NFL_EINVAL;
    if (n_directions < 1 || n_directions > NFL_SOLID_MAX_DIRECTIONS || n_directions % 2 == 0) return NFL_EINVAL;
    if (!nd_mesh_ok(d_vertices, d_triangles, n_vertices, n_triangles)) return NFL_EINVAL;
    const float lo[3] = {lo_x, lo_y, lo_z};
    const int32_t dims[3] = {nx, ny, nz};
    if (!nc_grid_args_ok(d_offsets, d_entries, n_entries, lo, cell, dims, false)) return NFL_EINVAL;
    if (n == 0) return NFL_OK;
    if (ng_bad(d_points, 4) || !d_votes) return NFL_EINVAL;
    NcSolid a = {d_points, n, nc_view(d_vertices, d_triangles, n_vertices, n_triangles, d_offsets, d_entries, n_entries, lo, cell, dims),
                 nx != 0 ? 1 : 0, n_directions, static_cast<uint8_t*>(d_votes), static_cast<uint8_t*>(d_inside)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 blocks(nm_grid(n)), threads(NM_THREADS);
    if (d_offsets) hipLaunchKernelGGL(nfl_mesh_inside_kernel<true>, blocks, threads, 0, s, a);
    else hipLaunchKernelGGL(nfl_mesh_inside_kernel<false>, blocks, threads, 0, s, a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
