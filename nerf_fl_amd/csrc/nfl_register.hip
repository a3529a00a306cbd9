// nfl_register.hip -- the similarity transform that brings points onto a mesh, or onto given partners, on the device
// (include/nerf_fl_amd.h, "registration"): apply a transform, reduce correspondences to a row of fp64 moments, solve for the
// increment and compose it.  A loop of apply -> nfl_mesh_closest -> moments -> solve never returns to the host: the
// transform lives in device memory and every kernel reads it there.  DESIGN.md section 34.
//
//   apply    a thread per row, fp64 inside, one fp32 rounding at the end
//   moments  the library's fixed-order fp64 reduction (nfl_reduce.h: the kernels, the fold and so the order of additions are
//            nfl_meshdist_reduce's).  Here only its policy: what a pair adds to a thread's columns, 19 of them in point mode
//            and 38 in plane mode (the kernels are instantiated per mode and the other mode's columns are written as zeros).
//            The face normal of a pair's triangle is nm_corners + nm_face_cross of nfl_geom.h, what nfl_mesh_closest runs.
//   solve    one thread: 4 x 4 Jacobi (point mode) or a 7 x 7 Cholesky (plane mode), unrolled so that the matrices stay in
//            registers
//
// No atomics, nothing allocated, set or copied through the runtime.
#include <math.h>

#include "nfl_geom.h"
#include "nfl_reduce.h"

#define NR_COLS NFL_REGISTER_COLUMNS
#define NR_POINT_COLS 19                                    // count, sum dd, and the 17 point-mode sums: columns 0 .. 18
#define NR_PLANE_COLS 38                                    // count, sum dd, and columns NFL_REGISTER_ATA .. NR_COLS - 1

static inline bool nr_size_ok(i64 n) { return n >= 0 && n <= ND_MAX_ENTRIES; }

// ------------------------------------------------------------------------------------------------------------------ apply

__global__ __launch_bounds__(NM_THREADS) void nfl_register_apply_kernel(const float* in, float* out, i64 n, const double* T,
                                                                        int vectors) {
    const i64 i = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (i >= n) return;
    const double x0 = (double)in[3 * i], x1 = (double)in[3 * i + 1], x2 = (double)in[3 * i + 2];
    const double s = T[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double y = (T[1 + 3 * k] * x0 + T[2 + 3 * k] * x1) + T[3 + 3 * k] * x2;
        out[3 * i + k] = vectors ? (float)y : (float)(s * y + T[10 + k]);
    }
}

extern "C" int nfl_register_apply(const float* d_in, float* d_out, int64_t n, const double* d_transform, int32_t vectors,
                                  void* stream) {
    if (!nr_size_ok(n) || (vectors != 0 && vectors != 1) || ng_bad(d_transform, 8)) return NFL_EINVAL;
    if (n == 0) return NFL_OK;
    if (ng_bad(d_in, 4) || ng_bad(d_out, 4)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_register_apply_kernel, dim3(nm_grid(n)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream), d_in,
                       d_out, (i64)n, d_transform, (int)vectors);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------- moments

extern "C" size_t nfl_register_bytes(int64_t n) {
    if (!nr_size_ok(n)) return 0;
    return ng_bytes(nr_moments_layout(n));
}

struct NrPairs {
    const float *points, *closest;
    const int32_t* triangle;
    const float *distance, *vertices;
    const int32_t* triangles;
    i64 V, T;
    float max_distance;
    double c[3];
};

// The reduction's policy (nfl_reduce.h), one per mode: a thread keeps only its mode's columns (19 in point mode, 38 in
// plane mode: 38 x 128 doubles of LDS = 38 KiB), and the finish writes the other mode's columns of the row as zeros.
template <int MODE>
struct NrMoments {
    NrPairs a;
    static constexpr int cols = MODE == NFL_REGISTER_POINT ? NR_POINT_COLS : NR_PLANE_COLS, width = NR_COLS;
    __host__ __device__ static constexpr int column(int k) {
        return MODE == NFL_REGISTER_POINT || k < 2 ? k : k + (NFL_REGISTER_ATA - 2);
    }
    typedef NgAdd Combine;

    // the unit face normal of triangle t, from the corners and the cross product nfl_mesh_closest's d_dot takes; false when
    // t is not usable or has none
    __device__ __forceinline__ bool face_normal(int32_t t, float* nf) const {
        float ca[3], cb[3], cc[3], cr[3], len;
        if (t < 0 || t >= a.T || !nm_corners(a.vertices, a.triangles, a.V, t, ca, cb, cc)) return false;
        nm_face_cross(ca, cb, cc, cr, &len);
        if (!(len > 0.f && len < INFINITY)) return false;
#pragma unroll
        for (int k = 0; k < 3; ++k) nf[k] = cr[k] / len;
        return true;
    }

    // adds pair i to the thread's columns when it counts
    __device__ __forceinline__ void add(i64 i, double* acc) const {
        const float P[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
        const float Q[3] = {a.closest[3 * i], a.closest[3 * i + 1], a.closest[3 * i + 2]};
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) ok = ok && ng_is_finite(P[k]) && ng_is_finite(Q[k]);
        if (!ok) return;
        double p[3], q[3], e[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = (double)P[k] - a.c[k];
            q[k] = (double)Q[k] - a.c[k];
            e[k] = (double)P[k] - (double)Q[k];
        }
        double dd = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        if (a.distance) {
            const float d = a.distance[i];
            if (!(d < INFINITY) || !(d <= a.max_distance)) return;
            dd = (double)d * (double)d;
        }
        float nf[3] = {0.f, 0.f, 0.f};
        if (a.triangle && !face_normal(a.triangle[i], nf)) return;
        acc[0] += 1.0;
        acc[1] += dd;
        if (MODE == NFL_REGISTER_POINT) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc[NFL_REGISTER_SUM_P + k] += p[k];
                acc[NFL_REGISTER_SUM_Q + k] += q[k];
            }
            acc[NFL_REGISTER_SUM_PP] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
            acc[NFL_REGISTER_SUM_QQ] += (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
#pragma unroll
            for (int i3 = 0; i3 < 3; ++i3)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[NFL_REGISTER_SUM_PQ + 3 * i3 + j] += p[i3] * q[j];
        } else {
            const double N[3] = {(double)nf[0], (double)nf[1], (double)nf[2]};
            const double v[7] = {p[1] * N[2] - p[2] * N[1], p[2] * N[0] - p[0] * N[2], p[0] * N[1] - p[1] * N[0], N[0], N[1], N[2],
                                 (p[0] * N[0] + p[1] * N[1]) + p[2] * N[2]};
            const double r = (N[0] * e[0] + N[1] * e[1]) + N[2] * e[2];
            int at = 2;                                                 // the thread's columns: count, dd, then ATA .. SUM_RR
#pragma unroll
            for (int i7 = 0; i7 < 7; ++i7)
#pragma unroll
                for (int j = i7; j < 7; ++j) acc[at++] += v[i7] * v[j];
#pragma unroll
            for (int i7 = 0; i7 < 7; ++i7) acc[at++] += v[i7] * r;
            acc[at] += r * r;
        }
    }
};

extern "C" int nfl_register_moments(const float* d_points, const float* d_closest, const int32_t* d_triangle,
                                    const float* d_distance, const float* d_vertices, const int32_t* d_triangles, int64_t n,
                                    int64_t n_vertices, int64_t n_triangles, int32_t mode, float max_distance, double cx, double cy,
                                    double cz, void* d_scratch, size_t scratch_bytes, double* d_row, void* stream) {
    if (!nr_size_ok(n) || !nm_sizes_ok(n_vertices, n_triangles)) return NFL_EINVAL;
    if (mode != NFL_REGISTER_POINT && mode != NFL_REGISTER_PLANE) return NFL_EINVAL;
    if (!(max_distance > 0.f)) return NFL_EINVAL;                                       // NaN included
    if (!ng_finite(cx) || !ng_finite(cy) || !ng_finite(cz) || ng_bad(d_row, 8)) return NFL_EINVAL;
    if (n) {
        if (ng_bad(d_points, 4) || ng_bad(d_closest, 4)) return NFL_EINVAL;
        if (mode == NFL_REGISTER_PLANE && (!d_triangle || !d_distance)) return NFL_EINVAL;
        if (ng_misaligned(d_triangle, 4) || ng_misaligned(d_distance, 4)) return NFL_EINVAL;
        if (d_triangle && !nd_mesh_ok(d_vertices, d_triangles, n_vertices, n_triangles)) return NFL_EINVAL;
    }
    double* parts = nullptr;
    const i64 blocks = nd_reduce_blocks(n);
    if (blocks) {
        NgLayout<NR_M_REGIONS> S = nr_moments_layout(n);
        const int rc = ng_carve(S, d_scratch, scratch_bytes);
        if (rc != NFL_OK) return rc;
        parts = S.get<double>(NR_M_PARTS);
    }
    const NrPairs a = {d_points, d_closest, d_triangle, d_distance, d_vertices, d_triangles, n_vertices, n_triangles,
                       max_distance, {cx, cy, cz}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == NFL_REGISTER_POINT)
        ng_reduce_launch(NrMoments<NFL_REGISTER_POINT>{a}, n, blocks, parts, d_row, s);
    else
        ng_reduce_launch(NrMoments<NFL_REGISTER_PLANE>{a}, n, blocks, parts, d_row, s);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ------------------------------------------------------------------------------------------------------------------ solve

struct NrStep {
    double ds, dR[9], dt[3];
};

// rot(w, x, y, z) of the header
__device__ __forceinline__ void nr_rot(double w, double x, double y, double z, double* R) {
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0 - 2.0 * (yy + zz), R[1] = 2.0 * (xy - wz), R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz), R[4] = 1.0 - 2.0 * (xx + zz), R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy), R[7] = 2.0 * (yz + wx), R[8] = 1.0 - 2.0 * (xx + yy);
}

__device__ __forceinline__ void nr_mul(const double* R, const double* x, double* y) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = (R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2];
}

// one Jacobi rotation of the header on (P, Q), compile-time indices so that A and V stay in registers
template <int P, int Q>
__device__ __forceinline__ void nr_jacobi(double (*A)[4], double (*V)[4]) {
    const double g = A[P][Q];
    if (g == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * g);
    const double sgn = theta >= 0.0 ? 1.0 : -1.0;
    const double t = sgn / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * g;
    A[Q][Q] = A[Q][Q] + t * g;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// POINT of the header; false: a pivot that is not > 0
__device__ bool nr_solve_point(const double* row, bool with_scale, const double* c, NrStep& S) {
    const double n = row[NFL_REGISTER_COUNT];
    double mp[3], mq[3], M[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) mp[k] = row[NFL_REGISTER_SUM_P + k] / n, mq[k] = row[NFL_REGISTER_SUM_Q + k] / n;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = row[NFL_REGISTER_SUM_PQ + 3 * i + j] - row[NFL_REGISTER_SUM_P + i] * mq[j];
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[2][2] = (M[1][1] - M[0][0]) - M[2][2];
    A[3][3] = (M[2][2] - M[0][0]) - M[1][1];
    A[0][1] = A[1][0] = M[1][2] - M[2][1];
    A[0][2] = A[2][0] = M[2][0] - M[0][2];
    A[0][3] = A[3][0] = M[0][1] - M[1][0];
    A[1][2] = A[2][1] = M[0][1] + M[1][0];
    A[1][3] = A[3][1] = M[2][0] + M[0][2];
    A[2][3] = A[3][2] = M[1][2] + M[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
        nr_jacobi<0, 1>(A, V);
        nr_jacobi<0, 2>(A, V);
        nr_jacobi<0, 3>(A, V);
        nr_jacobi<1, 2>(A, V);
        nr_jacobi<1, 3>(A, V);
        nr_jacobi<2, 3>(A, V);
    }
    double best = A[0][0], v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int m = 1; m < 4; ++m) {
        if (A[m][m] > best) {
            best = A[m][m];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = V[r][m];
        }
    }
    const double k = 1.0 / sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = v[r] * k;
    if (v[0] < 0.0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = -v[r];
    }
    nr_rot(v[0], v[1], v[2], v[3], S.dR);
    S.ds = 1.0;
    if (with_scale) {
        const double den = row[NFL_REGISTER_SUM_PP] - ((row[NFL_REGISTER_SUM_P] * mp[0] + row[NFL_REGISTER_SUM_P + 1] * mp[1]) +
                                                       row[NFL_REGISTER_SUM_P + 2] * mp[2]);
        if (!(den > 0.0)) return false;
        double num = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) num = num + S.dR[3 * i + j] * M[j][i];
        S.ds = num / den;
        if (!(S.ds > 0.0)) return false;
    }
    const double x[3] = {mp[0] + c[0], mp[1] + c[1], mp[2] + c[2]};
    double y[3];
    nr_mul(S.dR, x, y);
#pragma unroll
    for (int i = 0; i < 3; ++i) S.dt[i] = (mq[i] + c[i]) - S.ds * y[i];
    return true;
}

// PLANE of the header with m unknowns; false: a pivot that is not > 0
template <int m>
__device__ bool nr_solve_plane(const double* row, const double* c, NrStep& S) {
    double L[m][m], y[m], x[m];
#pragma unroll
    for (int j = 0; j < m; ++j) {
        double d = row[NFL_REGISTER_ATA + 7 * j - j * (j - 1) / 2];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d > 0.0)) return false;
        L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < m; ++i) {
            double v = row[NFL_REGISTER_ATA + 7 * j - j * (j - 1) / 2 + (i - j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < m; ++i) {
        double v = -row[NFL_REGISTER_ATB + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = m - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < m; ++k) v = v - L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    const double h0 = 0.5 * x[0], h1 = 0.5 * x[1], h2 = 0.5 * x[2];
    const double k = 1.0 / sqrt(((1.0 + h0 * h0) + h1 * h1) + h2 * h2);
    nr_rot(k, h0 * k, h1 * k, h2 * k, S.dR);
    S.ds = 1.0;
    if (m == 7) {
        S.ds = 1.0 + x[m - 1];
        if (!(S.ds > 0.0)) return false;
    }
    double yc[3];
    nr_mul(S.dR, c, yc);
#pragma unroll
    for (int i = 0; i < 3; ++i) S.dt[i] = (c[i] + x[3 + i]) - S.ds * yc[i];
    return true;
}

struct NrCentre {
    double c[3];
};

__global__ __launch_bounds__(64) void nfl_register_solve_kernel(const double* row, int mode, int with_scale, i64 min_pairs,
                                                                const NrCentre C, double* T, double* history, int iteration) {
    if (threadIdx.x != 0) return;
    const double count = row[NFL_REGISTER_COUNT];
    double* h = history + (size_t)iteration * NFL_REGISTER_HISTORY;
    h[0] = count;
    h[1] = sqrt(row[NFL_REGISTER_SUM_DD] / count);
    int status = NFL_REGISTER_OK;
    if (!(count >= (double)min_pairs)) {
        status = NFL_REGISTER_FEW;
    } else {
        NrStep S;
        bool ok;
        if (mode == NFL_REGISTER_POINT)
            ok = nr_solve_point(row, with_scale != 0, C.c, S);
        else
            ok = with_scale ? nr_solve_plane<7>(row, C.c, S) : nr_solve_plane<6>(row, C.c, S);
        double N[NFL_REGISTER_TRANSFORM];
        if (ok) {
            N[0] = S.ds * T[0];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    N[1 + 3 * i + j] = (S.dR[3 * i] * T[1 + j] + S.dR[3 * i + 1] * T[4 + j]) + S.dR[3 * i + 2] * T[7 + j];
            double y[3];
            nr_mul(S.dR, T + 10, y);
#pragma unroll
            for (int i = 0; i < 3; ++i) N[10 + i] = S.ds * y[i] + S.dt[i];
#pragma unroll
            for (int k = 0; k < NFL_REGISTER_TRANSFORM; ++k) ok = ok && ng_is_finite(N[k]);
        }
        if (ok) {
#pragma unroll
            for (int k = 0; k < NFL_REGISTER_TRANSFORM; ++k) T[k] = N[k];
        } else {
            status = NFL_REGISTER_SINGULAR;
        }
    }
    h[2] = (double)status;
    h[3] = T[0];
}

extern "C" int nfl_register_solve(const double* d_row, int32_t mode, int32_t with_scale, int64_t min_pairs, double cx, double cy,
                                  double cz, double* d_transform, double* d_history, int32_t iteration, void* stream) {
    if (mode != NFL_REGISTER_POINT && mode != NFL_REGISTER_PLANE) return NFL_EINVAL;
    if ((with_scale != 0 && with_scale != 1) || min_pairs < 1 || iteration < 0 || iteration > INT32_MAX / NFL_REGISTER_HISTORY)
        return NFL_EINVAL;
    if (!ng_finite(cx) || !ng_finite(cy) || !ng_finite(cz)) return NFL_EINVAL;
    if (ng_bad(d_row, 8) || ng_bad(d_transform, 8) || ng_bad(d_history, 8)) return NFL_EINVAL;
    const NrCentre C = {{cx, cy, cz}};
    hipLaunchKernelGGL(nfl_register_solve_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), d_row, (int)mode,
                       (int)with_scale, (i64)min_pairs, C, d_transform, d_history, (int)iteration);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
