// nfl_meshsmooth.hip -- smoothing an indexed triangle mesh on the device: vertex adjacency as two sorted CSR structures,
// Laplacian / Taubin steps over the neighbour rows, vertex normals from the triangles over the incident rows
// (include/nerf_fl_amd.h, "mesh smoothing").  DESIGN.md section 30.
//
//   count  zero      the two per-vertex counters, the two counters of d_totals = 0
//          corners   a thread per triangle: out of range -> counted; else one integer atomicAdd per corner
//          scan      exclusive scan of the counts (nm_scan of nfl_mesh_scan.hip): where every incident row starts; the total is I
//          fill      a thread per triangle: the entry 3 t + c goes to the row of tri[t][c] at the place its cursor hands out
//                    (the order of arrival: arbitrary)
//          rows      a thread per vertex SORTS its incident row, which is what makes every output reproducible, writes the
//                    candidates of the row (the other two corners of every entry, without v itself), sorts them and keeps
//                    the distinct ones: the neighbour row, its length, and the boundary flag (a candidate met exactly once).
//                    Rows of up to NFL_ADJ_SHORT_ROW entries are worked in a column of LDS by their own thread; a longer
//                    row (the hub of a fan, a heavily clustered mesh) is worked by the whole workgroup afterwards: a
//                    bitonic sort in LDS while it fits (8192 words), a rank sort through an LDS tile beyond that
//                    (d^2 / 256 comparisons a thread), then a scan that compacts the distinct values
//          scan      exclusive scan of the row lengths: where every neighbour row starts; the total is N
//   emit   the offsets (V + 1 of each), the flags, the incident entries (a straight copy: the scratch rows lie at the output's
//          offsets) and the neighbour rows (a thread per row; a long row is copied by the wave of its thread)
//   smooth a launch per step, a thread per vertex over a bounded grid: the sequential fp64 sum of the finite neighbours in
//          row order; the steps alternate between the scratch and the output so that the last one writes the output
//   normals  a thread per vertex over a bounded grid: the sequential fp64 sum of the triangle vectors in entry order
//
// Only integer atomics, and nothing that depends on their order leaves the count call.  Nothing here allocates, sets or
// copies memory through the runtime.
#include <math.h>

#include "nfl_geom.h"

#define NA_SHORT NFL_ADJ_SHORT_ROW                          // incident entries of a row that one thread sorts
#define NA_WS (2 * NA_SHORT)                                // LDS words of a thread: the candidates of such a row
#define NA_TILE (NA_WS * NM_THREADS)                        // the same LDS as the tile of a long row's rank sort: 12288 words
#define NA_BITONIC 8192                                     // words of a long row that are sorted in the LDS itself
#define NA_MAX_BLOCKS 2048                                  // grid of the smoothing and normal kernels

typedef NgLayout<NA_REGIONS> NaScratch;

extern "C" size_t nfl_mesh_adjacency_bytes(int64_t V, int64_t T) {
    if (!nm_sizes_ok(V, T)) return 0;
    return ng_bytes(na_layout(V, T));
}

extern "C" size_t nfl_mesh_smooth_bytes(int64_t V) {
    if (!nm_sizes_ok(V, 0)) return 0;
    return ng_bytes(na_smooth_layout(V));
}

// Checks shared by count and emit.  NFL_OK with V == 0 means: nothing to do.
static int na_carve(const nfl_mesh_adjacency_args* a, NaScratch& S) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    S = na_layout(a->n_vertices, a->n_triangles);
    if (a->n_triangles && !a->d_triangles) return NFL_EINVAL;
    if (a->n_vertices == 0) return NFL_OK;
    return ng_carve(S, a->d_scratch, a->scratch_bytes);
}

static inline unsigned na_bounded_grid(i64 n) {
    const i64 g = ng_cdiv(n, NM_THREADS);
    return (unsigned)(g < NA_MAX_BLOCKS ? g : NA_MAX_BLOCKS);
}

// --------------------------------------------------------------------------------------------------------------- count

__global__ __launch_bounds__(NM_THREADS) void nfl_adjacency_zero_kernel(int32_t* cnt, int32_t* cur, i64 V, i64* totals) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v < V) cnt[v] = cur[v] = 0;
    if (v == 0) totals[2] = totals[3] = 0;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_adjacency_corners_kernel(const int32_t* tri, i64 V, i64 T, int32_t* cnt,
                                                                           i64* n_out_of_range) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool bad = false;
    if (t < T) {
        const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        if (nm_in_range(a, b, c, V)) {
            atomicAdd(cnt + a, 1);
            atomicAdd(cnt + b, 1);
            atomicAdd(cnt + c, 1);
        } else {
            bad = true;
        }
    }
    ng_count_bad(bad, n_out_of_range);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_adjacency_fill_kernel(const int32_t* tri, i64 V, i64 T, const i64* toff,
                                                                        int32_t* cur, int32_t* inc) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (t >= T) return;
    const int32_t idx[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    if (!nm_in_range(idx[0], idx[1], idx[2], V)) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const i64 at = toff[idx[c]] + atomicAdd(cur + idx[c], 1);
        if (at >= 0 && at < 3 * T) inc[at] = (int32_t)(3 * t + c);          // the counts of this call put it there
    }
}

// the two corners of triangle e / 3 that are not corner e % 3, -1 in place of one that is u itself
__device__ __forceinline__ void na_others(const int32_t* tri, int32_t e, i64 u, int32_t& a, int32_t& b) {
    const i64 t = e / 3;
    const int c = e % 3;
    a = tri[3 * t + (c + 1) % 3];
    b = tri[3 * t + (c + 2) % 3];
    if (a == u) a = -1;
    if (b == u) b = -1;
}

// in-place insertion sort of n words of a thread's LDS column (word k at w[k * NM_THREADS])
__device__ __forceinline__ void na_sort_column(int32_t* w, int n) {
    for (int k = 1; k < n; ++k) {
        const int32_t x = w[k * NM_THREADS];
        int j = k;
        for (; j > 0 && w[(j - 1) * NM_THREADS] > x; --j) w[j * NM_THREADS] = w[(j - 1) * NM_THREADS];
        w[j * NM_THREADS] = x;
    }
}

// the power of two >= n, for 1 <= n <= NA_BITONIC
__device__ __forceinline__ int na_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// sorts tile[0 .. p) ascending, p a power of two in [2, NA_BITONIC]: the whole workgroup, a bitonic network in LDS
// (log2(p) (log2(p) + 1) / 2 stages of p / 2 compare-exchanges, a barrier a stage); the tile is filled before the call
__device__ void na_bitonic(int32_t* tile, int p) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= p; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < p / 2; t += NM_THREADS) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;          // the pair of this stage: bit j clear / set
                const bool up = (lo & k) == 0;
                const int32_t a = tile[lo], b = tile[hi];
                if ((a > b) == up) {
                    tile[lo] = b;
                    tile[hi] = a;
                }
            }
        }
    __syncthreads();
}

// dst[rank of src[i]] = src[i] for the n words of src, ranked by (value, place): the whole workgroup, through `tile`
// (NA_TILE words of LDS).  src and dst do not overlap.  A thread compares its words with all n: n^2 / NM_THREADS of them.
__device__ void na_rank_sort(const int32_t* src, i64 n, int32_t* dst, int32_t* tile) {
    const int tid = threadIdx.x;
    for (i64 ib = 0; ib < n; ib += NM_THREADS) {            // the same trips for every thread: there are barriers inside
        const i64 i = ib + tid;
        const bool mine = i < n;
        const int32_t x = mine ? src[i] : 0;
        i64 rank = 0;
        for (i64 base = 0; base < n; base += NA_TILE) {
            const int len = (int)(n - base < NA_TILE ? n - base : NA_TILE), len4 = (len + 3) / 4;
            __syncthreads();
            // filled up to whole int4s with a word no entry and no vertex index equals: it counts for nobody
            for (int k = tid; k < 4 * len4; k += NM_THREADS) tile[k] = k < len ? src[base + k] : INT32_MAX;
            __syncthreads();
            if (mine) {
                // the words before place `cut` of the tile come before src[i]
                const int cut = (int)(i - base < 0 ? 0 : i - base > NA_TILE ? NA_TILE : i - base);
                const int4* t4 = reinterpret_cast<const int4*>(tile);
                int c = 0;
#pragma unroll 4
                for (int q = 0; q < len4; ++q) {            // every lane reads the same words: four 16-byte broadcasts in flight
                    const int4 y = t4[q];
                    const int k = 4 * q;
                    c += (y.x < x) | ((y.x == x) & (k < cut));
                    c += (y.y < x) | ((y.y == x) & (k + 1 < cut));
                    c += (y.z < x) | ((y.z == x) & (k + 2 < cut));
                    c += (y.w < x) | ((y.w == x) & (k + 3 < cut));
                }
                rank += c;
            }
        }
        if (mine && rank < n) dst[rank] = x;
    }
}

// The row of vertex u, longer than NA_SHORT, by the whole workgroup: every thread calls with the same arguments.
__device__ void na_long_row(const int32_t* tri, i64 u, int n, i64 o, int32_t* inc, int32_t* cand, int32_t* tmp, int32_t* deg,
                            uint8_t* flag, i64* n_boundary, int32_t* tile, int32_t* wave_sum) {
    const int tid = threadIdx.x;
    int32_t *row = inc + o, *from = tmp + 2 * o, *nb = cand + 2 * o;
    const i64 m = 2 * (i64)n;
    if (n <= NA_BITONIC) {                                  // the entries fit the LDS: sorted there
        const int p = na_pow2(n);
        for (int k = tid; k < p; k += NM_THREADS) tile[k] = k < n ? row[k] : INT32_MAX;
        na_bitonic(tile, p);
        for (int k = tid; k < n; k += NM_THREADS) row[k] = tile[k];
    } else {
        na_rank_sort(row, n, from, tile);                   // entries are distinct: a permutation
        __syncthreads();
        for (i64 k = tid; k < n; k += NM_THREADS) row[k] = from[k];
    }
    __syncthreads();
    if (m <= NA_BITONIC) {                                  // so do the candidates
        const int p = na_pow2((int)m);
        for (int k = tid; k < p / 2; k += NM_THREADS) {
            int32_t a = INT32_MAX, b = INT32_MAX;
            if (k < n) na_others(tri, row[k], u, a, b);
            tile[2 * k] = a;
            tile[2 * k + 1] = b;
        }
        na_bitonic(tile, p);
        for (int k = tid; k < m; k += NM_THREADS) nb[k] = tile[k];
    } else {
        for (i64 k = tid; k < n; k += NM_THREADS) na_others(tri, row[k], u, from[2 * k], from[2 * k + 1]);
        __syncthreads();
        na_rank_sort(from, m, nb, tile);
    }
    __syncthreads();                                        // nb: the candidates ascending, the -1s first
    // the distinct values move to the front: a thread's value goes to a place at or before its own, and no place is read
    // after the chunk that owns it has written
    i64 run = 0;
    int single = 0;
    for (i64 ib = 0; ib < m; ib += NM_THREADS) {
        const i64 i = ib + tid;
        const bool mine = i < m;
        const int32_t x = mine ? nb[i] : -1;
        const bool first = mine && x >= 0 && (i == 0 || nb[i - 1] != x);
        single |= first && (i + 1 == m || nb[i + 1] != x);
        int32_t total;
        const int32_t before = ng_block_scan<int32_t, NM_THREADS>(first ? 1 : 0, wave_sum, total);
        if (first) nb[run + before] = x;
        run += total;
        __syncthreads();
    }
    const int any = __syncthreads_or(single);
    if (tid == 0) {
        deg[u] = (int32_t)run;
        flag[u] = any ? 1 : 0;
        if (any) atomicAdd(reinterpret_cast<unsigned long long*>(n_boundary), 1ull);
    }
}

__global__ __launch_bounds__(NM_THREADS) void nfl_adjacency_rows_kernel(const int32_t* tri, i64 V, i64 T, const int32_t* cnt,
                                                                        const i64* toff, int32_t* inc, int32_t* cand, int32_t* tmp,
                                                                        int32_t* deg, uint8_t* flag, i64* n_boundary) {
    __shared__ __attribute__((aligned(16))) int32_t ws[NA_TILE];
    __shared__ int32_t is_long[NM_THREADS];
    __shared__ int32_t wave_sum[NM_THREADS / 64];
    const int tid = threadIdx.x;
    const i64 v = (i64)blockIdx.x * NM_THREADS + tid;
    int n = 0;
    i64 o = 0;
    if (v < V) {
        n = cnt[v];
        o = toff[v];
        if (n < 0 || o < 0 || o + n > 3 * T) n = 0;         // the scan of this call's counts: never; an empty row if it were
    }
    bool boundary = false;
    if (v < V && n <= NA_SHORT) {
        int32_t* w = ws + tid;
        for (int k = 0; k < n; ++k) w[k * NM_THREADS] = inc[o + k];
        na_sort_column(w, n);
        int m = 0;
        for (int k = 0; k < n; ++k) {                       // the candidates pass through the sorting area: in the column
            const int32_t e = w[k * NM_THREADS];            // they would cover the entries still to come
            inc[o + k] = e;
            int32_t a, b;
            na_others(tri, e, v, a, b);
            if (a >= 0) tmp[2 * o + m++] = a;
            if (b >= 0) tmp[2 * o + m++] = b;
        }
        for (int k = 0; k < m; ++k) w[k * NM_THREADS] = tmp[2 * o + k];
        na_sort_column(w, m);
        int d = 0;
        for (int k = 0; k < m;) {
            const int32_t x = w[k * NM_THREADS];
            int r = 1;
            while (k + r < m && w[(k + r) * NM_THREADS] == x) ++r;
            cand[2 * o + d++] = x;
            boundary |= r == 1;
            k += r;
        }
        deg[v] = d;
        flag[v] = boundary ? 1 : 0;
    }
    ng_count_bad(boundary, n_boundary);
    is_long[tid] = v < V && n > NA_SHORT;
    __syncthreads();
    for (int r = 0; r < NM_THREADS; ++r) {
        if (!is_long[r]) continue;                          // the same for every thread
        const i64 u = (i64)blockIdx.x * NM_THREADS + r;
        na_long_row(tri, u, cnt[u], toff[u], inc, cand, tmp, deg, flag, n_boundary, ws, wave_sum);
    }
}

extern "C" int nfl_mesh_adjacency_count(const nfl_mesh_adjacency_args* a, void* stream) {
    NaScratch S;
    const int rc = na_carve(a, S);
    if (rc != NFL_OK) return rc;
    const i64 V = a->n_vertices, T = a->n_triangles;
    if (V == 0) return NFL_OK;
    if (!a->d_totals) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t *cnt = S.get<int32_t>(NA_CNT), *cur = S.get<int32_t>(NA_CUR), *deg = S.get<int32_t>(NA_DEG);
    int32_t *inc = S.get<int32_t>(NA_INC), *cand = S.get<int32_t>(NA_CAND), *tmp = S.get<int32_t>(NA_TMP);
    i64 *toff = S.get<i64>(NA_TOFF), *off = S.get<i64>(NA_OFF), *sums = S.get<i64>(NA_SUMS);
    uint8_t* flag = S.get<uint8_t>(NA_FLAG);
    hipLaunchKernelGGL(nfl_adjacency_zero_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, cnt, cur, V, a->d_totals);
    if (T)
        hipLaunchKernelGGL(nfl_adjacency_corners_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_triangles, V, T, cnt,
                           a->d_totals + 2);
    nm_scan(cnt, toff, V, sums, a->d_totals, s);
    if (T)
        hipLaunchKernelGGL(nfl_adjacency_fill_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_triangles, V, T, toff, cur, inc);
    hipLaunchKernelGGL(nfl_adjacency_rows_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_triangles, V, T, cnt, toff, inc,
                       cand, tmp, deg, flag, a->d_totals + 3);
    nm_scan(deg, off, V, sums, a->d_totals + 1, s);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------- emit

// thread v of V + 1: the two offsets (the totals at V), the flag
__global__ __launch_bounds__(NM_THREADS) void nfl_adjacency_emit_offsets_kernel(const i64* toff, const i64* off, const uint8_t* flag,
                                                                                i64 V, i64 I, i64 N, i64* out_toff, i64* out_off,
                                                                                uint8_t* out_flag) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v > V) return;
    const i64 a = v < V ? toff[v] : I, b = v < V ? off[v] : N;
    out_toff[v] = a < 0 ? 0 : a > I ? I : a;
    out_off[v] = b < 0 ? 0 : b > N ? N : b;
    if (v < V) out_flag[v] = flag[v] ? 1 : 0;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_adjacency_emit_incident_kernel(const int32_t* inc, i64 I, int32_t* out) {
    const i64 e = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (e < I) out[e] = inc[e];
}

__global__ __launch_bounds__(NM_THREADS) void nfl_adjacency_emit_neighbors_kernel(const i64* toff, const i64* off, const int32_t* deg,
                                                                                  const int32_t* cand, i64 V, i64 T, i64 N, int32_t* out) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    i64 src = 0, dst = 0;
    int d = 0;
    if (v < V) {
        src = 2 * toff[v];
        dst = off[v];
        d = deg[v];
        if (d < 0 || src < 0 || dst < 0 || src + d > 6 * T || dst + d > N) d = 0;
    }
    if (d <= NA_WS)
        for (int k = 0; k < d; ++k) out[dst + k] = cand[src + k];
    // a long row is copied by the wave of its thread, one row after the other
    const int lane = threadIdx.x & 63;
    for (unsigned long long m = __ballot(d > NA_WS); m; m &= m - 1) {
        const int l = __ffsll(m) - 1;
        const i64 rs = __shfl(src, l), rd = __shfl(dst, l);
        const int rn = __shfl(d, l);
        for (int k = lane; k < rn; k += 64) out[rd + k] = cand[rs + k];
    }
}

extern "C" int nfl_mesh_adjacency_emit(const nfl_mesh_adjacency_args* a, void* stream) {
    NaScratch S;
    const int rc = na_carve(a, S);
    if (rc != NFL_OK) return rc;
    const i64 V = a->n_vertices, T = a->n_triangles, I = a->n_incident, N = a->n_neighbors;
    if (V == 0) return NFL_OK;
    if (!na_totals_ok(T, I, N)) return NFL_EINVAL;
    if (!a->d_tri_offsets || !a->d_offsets || !a->d_boundary || (I && !a->d_incident) || (N && !a->d_neighbors)) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const i64 *toff = S.get<i64>(NA_TOFF), *off = S.get<i64>(NA_OFF);
    hipLaunchKernelGGL(nfl_adjacency_emit_offsets_kernel, dim3(nm_grid(V + 1)), dim3(NM_THREADS), 0, s, toff, off,
                       S.get<uint8_t>(NA_FLAG), V, I, N, a->d_tri_offsets, a->d_offsets, a->d_boundary);
    if (I)
        hipLaunchKernelGGL(nfl_adjacency_emit_incident_kernel, dim3(nm_grid(I)), dim3(NM_THREADS), 0, s, S.get<int32_t>(NA_INC), I,
                           a->d_incident);
    if (N)
        hipLaunchKernelGGL(nfl_adjacency_emit_neighbors_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, toff, off,
                           S.get<int32_t>(NA_DEG), S.get<int32_t>(NA_CAND), V, T, N, a->d_neighbors);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// -------------------------------------------------------------------------------------------------------------- smooth

__device__ __forceinline__ bool na_finite3(float x, float y, float z) { return ng_is_finite(x) && ng_is_finite(y) && ng_is_finite(z); }

__global__ __launch_bounds__(NM_THREADS) void nfl_smooth_copy_kernel(const float* in, i64 n, float* out) {
    for (i64 i = (i64)blockIdx.x * NM_THREADS + threadIdx.x; i < n; i += (i64)gridDim.x * NM_THREADS) out[i] = in[i];
}

// One Jacobi step.  A thread per vertex walks its row: the indices of a row are contiguous, the positions they name are
// gathered.  The sum is the definition's: fp64, in row order.
__global__ __launch_bounds__(NM_THREADS) void nfl_smooth_step_kernel(const float* __restrict__ in, const i64* __restrict__ off,
                                                                     const int32_t* __restrict__ nbr, i64 V, i64 N,
                                                                     const uint8_t* __restrict__ boundary,
                                                                     const uint8_t* __restrict__ pinned, double f,
                                                                     float* __restrict__ out) {
    for (i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x; v < V; v += (i64)gridDim.x * NM_THREADS) {
        const float px = in[3 * v], py = in[3 * v + 1], pz = in[3 * v + 2];
        float ox = px, oy = py, oz = pz;
        const bool stays = (pinned && pinned[v]) || (boundary && boundary[v]);
        if (!stays && na_finite3(px, py, pz)) {
            i64 a = off[v], b = off[v + 1];
            if (a < 0 || a > b || b > N) a = b = 0;
            double sx = 0.0, sy = 0.0, sz = 0.0;
            int d = 0;
#pragma unroll 4
            for (i64 j = a; j < b; ++j) {                   // no branch: the loads of several neighbours are in flight
                const int32_t w = nbr[j];
                const bool inside = w >= 0 && w < V;
                const i64 r = inside ? 3 * (i64)w : 0;
                const float qx = in[r], qy = in[r + 1], qz = in[r + 2];
                const bool ok = inside && na_finite3(qx, qy, qz);
                sx = ok ? sx + (double)qx : sx;
                sy = ok ? sy + (double)qy : sy;
                sz = ok ? sz + (double)qz : sz;
                d += ok ? 1 : 0;
            }
            if (d) {
                const double n = (double)d, x = (double)px, y = (double)py, z = (double)pz;
                ox = (float)(x + f * (sx / n - x));
                oy = (float)(y + f * (sy / n - y));
                oz = (float)(z + f * (sz / n - z));
            }
        }
        out[3 * v] = ox;
        out[3 * v + 1] = oy;
        out[3 * v + 2] = oz;
    }
}

extern "C" int nfl_mesh_smooth(const nfl_mesh_smooth_args* a, void* stream) {
    if (!a || !nm_sizes_ok(a->n_vertices, 0) || a->n_neighbors < 0) return NFL_EINVAL;
    if (a->n_steps < 0 || a->n_steps > NFL_SMOOTH_MAX_STEPS || (a->n_steps && !a->factors)) return NFL_EINVAL;
    for (int k = 0; k < a->n_steps; ++k)
        if (!isfinite(a->factors[k])) return NFL_EINVAL;
    const i64 V = a->n_vertices, N = a->n_neighbors;
    if (V == 0) return NFL_OK;
    if (!a->d_vertices || !a->d_offsets || !a->d_out_vertices || (N && !a->d_neighbors)) return NFL_EINVAL;
    if (a->d_out_vertices == a->d_vertices || (a->fix_boundary && !a->d_boundary)) return NFL_EINVAL;
    NgLayout<NA_S_REGIONS> S = na_smooth_layout(V);
    const int rc = ng_carve(S, a->d_scratch, a->scratch_bytes);
    if (rc != NFL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* buf[2] = {a->d_out_vertices, S.get<float>(NA_S_PING)};
    if (a->n_steps == 0)
        hipLaunchKernelGGL(nfl_smooth_copy_kernel, dim3(na_bounded_grid(3 * V)), dim3(NM_THREADS), 0, s, a->d_vertices, 3 * V, buf[0]);
    const float* in = a->d_vertices;
    for (int k = 0; k < a->n_steps; ++k) {
        float* out = buf[(a->n_steps - 1 - k) & 1];         // the last step writes the output
        hipLaunchKernelGGL(nfl_smooth_step_kernel, dim3(na_bounded_grid(V)), dim3(NM_THREADS), 0, s, in, a->d_offsets, a->d_neighbors,
                           V, N, a->fix_boundary ? a->d_boundary : nullptr, a->d_pinned, a->factors[k], out);
        in = out;
    }
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ------------------------------------------------------------------------------------------------------------- normals

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_normals_kernel(const float* __restrict__ pos, const int32_t* __restrict__ tri,
                                                                      i64 V, i64 T, const i64* __restrict__ toff,
                                                                      const int32_t* __restrict__ inc, i64 I, int uniform,
                                                                      const float* __restrict__ fallback, float* __restrict__ out) {
    for (i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x; v < V; v += (i64)gridDim.x * NM_THREADS) {
        i64 a = toff[v], b = toff[v + 1];
        if (a < 0 || a > b || b > I || T == 0) a = b = 0;
        double s[3] = {0.0, 0.0, 0.0};
#pragma unroll 2
        for (i64 j = a; j < b; ++j) {
            const int32_t e = inc[j];
            if (e < 0 || e >= 3 * T) continue;
            const i64 t = e / 3;
            const int32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
            if (!nm_in_range(i0, i1, i2, V)) continue;
            double p[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p[0][k] = (double)pos[3 * (i64)i0 + k];
                p[1][k] = (double)pos[3 * (i64)i1 + k];
                p[2][k] = (double)pos[3 * (i64)i2 + k];
            }
            const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            if (!(isfinite(cr[0]) && isfinite(cr[1]) && isfinite(cr[2])) || (cr[0] == 0.0 && cr[1] == 0.0 && cr[2] == 0.0)) continue;
            if (uniform) {
                const double len = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
                s[0] += cr[0] / len;
                s[1] += cr[1] / len;
                s[2] += cr[2] / len;
            } else {
                s[0] += cr[0];
                s[1] += cr[1];
                s[2] += cr[2];
            }
        }
        const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
        const bool ok = len > 0.0 && isfinite(len);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * v + k] = ok ? (float)(s[k] / len) : fallback ? fallback[3 * v + k] : 0.0f;
    }
}

extern "C" int nfl_mesh_normals(const nfl_mesh_normals_args* a, void* stream) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles) || a->n_incident < 0) return NFL_EINVAL;
    if (a->weighting != NFL_NORMALS_AREA && a->weighting != NFL_NORMALS_UNIFORM) return NFL_EINVAL;
    const i64 V = a->n_vertices, T = a->n_triangles, I = a->n_incident;
    if (T && !a->d_triangles) return NFL_EINVAL;
    if (V == 0) return NFL_OK;
    if (!a->d_vertices || !a->d_tri_offsets || !a->d_out_normals || (I && !a->d_incident)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_mesh_normals_kernel, dim3(na_bounded_grid(V)), dim3(NM_THREADS), 0, static_cast<hipStream_t>(stream),
                       a->d_vertices, a->d_triangles, V, T, a->d_tri_offsets, a->d_incident, I,
                       a->weighting == NFL_NORMALS_UNIFORM ? 1 : 0, a->d_fallback_normals, a->d_out_normals);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
