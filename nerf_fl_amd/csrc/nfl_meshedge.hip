// nfl_meshedge.hip -- the edges of an indexed triangle mesh on the device, its boundary loops, and the caps that close them
// (include/nerf_fl_amd.h, "mesh edges").  DESIGN.md section 39.
//
//   edges  count  zero      the per-edge counters and cursors, the totals = 0
//                 own       a thread per vertex a: the neighbours b > a of its sorted row (a binary search): the edges a owns
//                 scan      where the edges of every vertex start (nm_scan); the total is E
//                 halves    a thread per triangle: the edge of each of its three half-edges, by a binary search for the larger
//                           end in the row of the smaller one; one integer atomicAdd per half-edge on its edge's counter
//                 scan      where the row of every edge starts; the total is H
//                 fill      a thread per half-edge: into its edge's row at the place the cursor hands out (arbitrary order)
//                 rows      a thread per edge SORTS its row (rows of 1 or 2 on real meshes; up to NFL_EDGE_SHORT_ROW by the
//                           thread, a longer row -- a book of triangles on one edge -- by the wave of its thread, a rank sort)
//                           and classifies the edge
//                 finish    the totals, bounded
//          emit   a thread per half-edge (its edge, its twin, the edge's ends by the first half-edge of the row), a thread per
//                 edge (offset, kind), a copy of the rows
//   loops  count  succ      a thread per half-edge: the rotation about its end vertex through the twins
//                 double    ceil(log2 B) + 1 rounds of pointer doubling over succ between two buffers: the smallest half-edge
//                           ahead, and -1 once a dead end is ahead.  Alive at the end = on a cycle
//                 label     the root (smallest half-edge) of every loop; open chains counted
//                 scan      roots before h: the loop's number; the total is L
//                 fold      a thread per loop walks it from its root: positions, length, and the sequential fp64 sums
//                 scan      where every loop's row starts; the total is B'
//          emit   a thread per half-edge (loop_of, its place in loop_halves), a thread per loop (the table)
//   fill   count  a thread per loop: selected or not, its new vertices and triangles; two scans
//          emit   copies of the input rows, a thread per loop entry (its triangle), a thread per loop (its vertex: the
//                 sequential fp64 sums in walk order)
//
// Only integer atomics, and nothing that depends on their order leaves a count call.  Everything read from the scratch or from
// a caller's table is bounded before it is used as an index.  Nothing here allocates, sets or copies memory through the
// runtime.
#include <math.h>

#include "nfl_geom.h"

typedef NgLayout<NE_REGIONS> NeScratch;
typedef NgLayout<NL_REGIONS> NlScratch;
typedef NgLayout<NF_REGIONS> NfScratch;

// the half-edge after h in its triangle
__device__ __forceinline__ i64 ne_next(i64 h) {
    const i64 c = h % 3;
    return h - c + (c + 1) % 3;
}

// adds the wave's sum of n (a small count per lane) to *counter: one atomic per wave that has any.  Every lane must call it.
__device__ __forceinline__ void ne_count_add(int n, i64* counter) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)n);
}

extern "C" size_t nfl_mesh_edges_bytes(int64_t V, int64_t T) {
    if (!nm_sizes_ok(V, T)) return 0;
    return ng_bytes(ne_layout(V, T));
}

extern "C" size_t nfl_mesh_loops_bytes(int64_t T) {
    if (!nm_sizes_ok(0, T)) return 0;
    return ng_bytes(nl_layout(T));
}

extern "C" size_t nfl_mesh_fill_bytes(int64_t L) {
    if (L < 0 || L > INT32_MAX / 3) return 0;
    return ng_bytes(nf_layout(L));
}

// ======================================================================================================== edges: count

__global__ __launch_bounds__(NM_THREADS) void nfl_edges_zero_kernel(int32_t* cnt, int32_t* cur, i64 H3, i64* totals, i64* raw) {
    const i64 e = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (e < H3) cnt[e] = cur[e] = 0;
    if (e < NFL_EDGE_TOTALS) totals[e] = 0;
    if (e < 2) raw[e] = 0;
}

// the row of vertex v in a caller's adjacency, bounded: [o0, o1) inside [0, N), empty when the offsets are not in order
__device__ __forceinline__ void ne_row(const i64* off, i64 v, i64 N, i64& o0, i64& o1) {
    o0 = off[v];
    o1 = off[v + 1];
    if (o0 < 0 || o0 > o1 || o1 > N) o0 = o1 = 0;
}

// the first place in [lo, hi) whose value is not below x (hi when there is none): the row is ascending
__device__ __forceinline__ i64 ne_lower(const int32_t* row, i64 lo, i64 hi, int32_t x) {
    while (lo < hi) {
        const i64 mid = lo + (hi - lo) / 2;
        if (row[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_edges_own_kernel(const i64* off, const int32_t* nbr, i64 V, i64 N, int32_t* own) {
    const i64 a = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (a >= V) return;
    i64 o0, o1;
    ne_row(off, a, N, o0, o1);
    own[a] = a + 1 > INT32_MAX ? 0 : (int32_t)(o1 - ne_lower(nbr, o0, o1, (int32_t)(a + 1)));      // the neighbours above a
}

__global__ __launch_bounds__(NM_THREADS) void nfl_edges_halves_kernel(const int32_t* tri, i64 V, i64 T, const i64* off,
                                                                      const int32_t* nbr, i64 N, const int32_t* own, const i64* eoff,
                                                                      int32_t* he, int32_t* cnt, i64* totals) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool outside = false;
    int degenerate = 0;
    if (t < T) {
        const int32_t idx[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
        outside = !nm_in_range(idx[0], idx[1], idx[2], V);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int32_t a = idx[c], b = idx[(c + 1) % 3];
            int32_t e = -1;
            if (!outside && a == b) ++degenerate;
            if (!outside && a != b) {
                const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
                i64 o0, o1;
                ne_row(off, lo, N, o0, o1);
                const i64 n = own[lo];
                if (n >= 0 && n <= o1 - o0) {
                    const i64 first = o1 - n, p = ne_lower(nbr, first, o1, hi);
                    const i64 id = eoff[lo] + (p - first);
                    if (p < o1 && nbr[p] == hi && id >= 0 && id < 3 * T) e = (int32_t)id;       // an adjacency of this mesh: always
                }
            }
            he[3 * t + c] = e;
            if (e >= 0) atomicAdd(cnt + e, 1);
        }
    }
    ng_count_bad(outside, totals + 6);
    ne_count_add(degenerate, totals + 5);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_edges_fill_kernel(const int32_t* he, i64 H3, const i64* hoff, int32_t* cur,
                                                                    int32_t* tmp) {
    const i64 h = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (h >= H3) return;
    const int32_t e = he[h];
    if (e < 0 || e >= H3) return;
    const i64 at = hoff[e] + atomicAdd(cur + e, 1);
    if (at >= 0 && at < H3) tmp[at] = (int32_t)h;           // the counts of this call put it there
}

// whether half-edge h runs from the smaller to the larger of its ends
__device__ __forceinline__ bool ne_forward(const int32_t* tri, i64 h) { return tri[h] < tri[ne_next(h)]; }

__global__ __launch_bounds__(NM_THREADS) void nfl_edges_rows_kernel(const int32_t* tri, i64 H3, const int32_t* cnt, const i64* hoff,
                                                                    const int32_t* tmp, int32_t* eh, uint8_t* kind, i64* totals) {
    const i64 e = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    int n = 0;
    i64 o = 0;
    if (e < H3) {
        n = cnt[e];
        o = hoff[e];
        if (n < 0 || o < 0 || o + n > H3) n = 0;            // the scan of this call's counts: never; an empty row if it were
    }
    if (n <= NFL_EDGE_SHORT_ROW)
        for (int k = 0; k < n; ++k) {                       // the entries are distinct: the rank is the place
            const int32_t x = tmp[o + k];
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += tmp[o + j] < x;
            eh[o + rank] = x;
        }
    // a long row is sorted by the wave of its thread, one row after the other: n^2 / 64 comparisons a lane
    const int lane = threadIdx.x & 63;
    for (unsigned long long m = __ballot(n > NFL_EDGE_SHORT_ROW); m; m &= m - 1) {
        const int l = __ffsll(m) - 1;
        const i64 ro = __shfl(o, l);
        const int rn = __shfl(n, l);
        for (int k = lane; k < rn; k += 64) {
            const int32_t x = tmp[ro + k];
            int rank = 0;
            for (int j = 0; j < rn; ++j) rank += tmp[ro + j] < x;      // every lane reads the same word: a broadcast
            if (rank < rn) eh[ro + rank] = x;
        }
    }
    int k = NFL_EDGE_NONMANIFOLD;
    if (n == 1) k = NFL_EDGE_BOUNDARY;
    if (n == 2) {
        const i64 h0 = tmp[o], h1 = tmp[o + 1];
        if (h0 >= 0 && h0 < H3 && h1 >= 0 && h1 < H3) k = ne_forward(tri, h0) != ne_forward(tri, h1) ? NFL_EDGE_INTERIOR : NFL_EDGE_FLIPPED;
    }
    if (e < H3) kind[e] = (uint8_t)k;
    ng_count_bad(n > 0 && k == NFL_EDGE_BOUNDARY, totals + 2);
    ng_count_bad(n > 0 && k == NFL_EDGE_FLIPPED, totals + 3);
    ng_count_bad(n > 0 && k == NFL_EDGE_NONMANIFOLD, totals + 4);
}

__global__ __launch_bounds__(64) void nfl_edges_finish_kernel(const i64* raw, i64 H3, i64* totals) {
    if (threadIdx.x >= 2) return;
    const i64 v = raw[threadIdx.x];
    totals[threadIdx.x] = v < 0 ? 0 : v > H3 ? H3 : v;
}

extern "C" int nfl_mesh_edges_count(const int32_t* d_triangles, int64_t V, int64_t T, const int64_t* d_offsets,
                                    const int32_t* d_neighbors, int64_t N, void* d_scratch, size_t scratch_bytes,
                                    int64_t* d_totals, void* stream) {
    if (!nm_sizes_ok(V, T) || N < 0 || N > 6 * T) return NFL_EINVAL;
    if (ng_misaligned(d_triangles, 4) || ng_misaligned(d_offsets, 8) || ng_misaligned(d_neighbors, 4) || ng_misaligned(d_totals, 8))
        return NFL_EINVAL;
    if (V == 0 || T == 0) return NFL_OK;
    if (!d_triangles || !d_offsets || !d_totals || (N && !d_neighbors)) return NFL_EINVAL;
    NeScratch S = ne_layout(V, T);
    const int rc = ng_carve(S, d_scratch, scratch_bytes);
    if (rc != NFL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const i64 H3 = 3 * T;
    int32_t *own = S.get<int32_t>(NE_OWN), *he = S.get<int32_t>(NE_HE), *cnt = S.get<int32_t>(NE_CNT), *cur = S.get<int32_t>(NE_CUR);
    int32_t *tmp = S.get<int32_t>(NE_TMP), *eh = S.get<int32_t>(NE_EH);
    i64 *eoff = S.get<i64>(NE_EOFF), *hoff = S.get<i64>(NE_HOFF), *sums = S.get<i64>(NE_SUMS), *raw = S.get<i64>(NE_RAW);
    hipLaunchKernelGGL(nfl_edges_zero_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, cnt, cur, H3, d_totals, raw);
    hipLaunchKernelGGL(nfl_edges_own_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, d_offsets, d_neighbors, V, N, own);
    nm_scan(own, eoff, V, sums, raw, s);
    hipLaunchKernelGGL(nfl_edges_halves_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, d_triangles, V, T, d_offsets, d_neighbors, N,
                       own, eoff, he, cnt, d_totals);
    nm_scan(cnt, hoff, H3, sums, raw + 1, s);
    hipLaunchKernelGGL(nfl_edges_fill_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, he, H3, hoff, cur, tmp);
    hipLaunchKernelGGL(nfl_edges_rows_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, d_triangles, H3, cnt, hoff, tmp, eh,
                       S.get<uint8_t>(NE_KIND), d_totals);
    hipLaunchKernelGGL(nfl_edges_finish_kernel, dim3(1), dim3(64), 0, s, raw, H3, d_totals);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ========================================================================================================= edges: emit

__global__ __launch_bounds__(NM_THREADS) void nfl_edges_emit_halves_kernel(const int32_t* tri, i64 H3, const int32_t* he,
                                                                           const int32_t* cnt, const i64* hoff, const int32_t* eh,
                                                                           const uint8_t* kind, i64 E, i64 H, int32_t* out_he,
                                                                           int32_t* out_twin, int32_t* out_edges) {
    const i64 h = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (h >= H3) return;
    int32_t e = he[h], twin = -1;
    if (e < 0 || e >= E) e = -1;
    if (e >= 0) {
        const i64 o = hoff[e];
        const int n = cnt[e];
        if (o >= 0 && n >= 1 && o + n <= H) {
            const int32_t first = eh[o];
            if (first == h) {                               // the smallest half-edge of the row writes the edge's ends
                const int32_t a = tri[h], b = tri[ne_next(h)];
                out_edges[2 * (i64)e] = a < b ? a : b;
                out_edges[2 * (i64)e + 1] = a < b ? b : a;
            }
            if (n == 2 && kind[e] == NFL_EDGE_INTERIOR) {
                const int32_t other = first == h ? eh[o + 1] : first;
                if (other >= 0 && other < H3) twin = other;
            }
        }
    }
    out_he[h] = e;
    out_twin[h] = twin;
}

// thread e of E + 1: the offset (H at E), the kind
__global__ __launch_bounds__(NM_THREADS) void nfl_edges_emit_edges_kernel(const i64* hoff, const uint8_t* kind, i64 E, i64 H,
                                                                          i64* out_off, uint8_t* out_kind) {
    const i64 e = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (e > E) return;
    const i64 o = e < E ? hoff[e] : H;
    out_off[e] = o < 0 ? 0 : o > H ? H : o;
    if (e < E) out_kind[e] = kind[e] > NFL_EDGE_NONMANIFOLD ? (uint8_t)NFL_EDGE_NONMANIFOLD : kind[e];
}

__global__ __launch_bounds__(NM_THREADS) void nfl_edges_copy_kernel(const int32_t* in, i64 n, int32_t* out) {
    for (i64 i = (i64)blockIdx.x * NM_THREADS + threadIdx.x; i < n; i += (i64)gridDim.x * NM_THREADS) out[i] = in[i];
}

static inline unsigned ne_bounded_grid(i64 n) {
    const i64 g = ng_cdiv(n, NM_THREADS);
    return (unsigned)(g < 2048 ? g : 2048);
}

extern "C" int nfl_mesh_edges_emit(const int32_t* d_triangles, int64_t V, int64_t T, const void* d_scratch, size_t scratch_bytes,
                                   int64_t E, int64_t H, int32_t* d_edges, int32_t* d_half_edge, int64_t* d_edge_offsets,
                                   int32_t* d_edge_halves, void* d_kind, int32_t* d_twin, void* stream) {
    if (!nm_sizes_ok(V, T) || !ne_totals_ok(T, E, H)) return NFL_EINVAL;
    if (ng_misaligned(d_triangles, 4) || ng_misaligned(d_edges, 4) || ng_misaligned(d_half_edge, 4) || ng_misaligned(d_edge_offsets, 8)
        || ng_misaligned(d_edge_halves, 4) || ng_misaligned(d_twin, 4))
        return NFL_EINVAL;
    if (V == 0 || T == 0) return NFL_OK;
    if (!d_triangles || !d_half_edge || !d_edge_offsets || !d_twin || (E && (!d_edges || !d_kind)) || (H && !d_edge_halves))
        return NFL_EINVAL;
    NeScratch S = ne_layout(V, T);
    const int rc = ng_carve(S, const_cast<void*>(d_scratch), scratch_bytes);
    if (rc != NFL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const i64 H3 = 3 * T;
    const i64* hoff = S.get<i64>(NE_HOFF);
    const uint8_t* kind = S.get<uint8_t>(NE_KIND);
    hipLaunchKernelGGL(nfl_edges_emit_halves_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, d_triangles, H3, S.get<int32_t>(NE_HE),
                       S.get<int32_t>(NE_CNT), hoff, S.get<int32_t>(NE_EH), kind, E, H, d_half_edge, d_twin, d_edges);
    hipLaunchKernelGGL(nfl_edges_emit_edges_kernel, dim3(nm_grid(E + 1)), dim3(NM_THREADS), 0, s, hoff, kind, E, H, d_edge_offsets,
                       static_cast<uint8_t*>(d_kind));
    if (H)
        hipLaunchKernelGGL(nfl_edges_copy_kernel, dim3(ne_bounded_grid(H)), dim3(NM_THREADS), 0, s, S.get<int32_t>(NE_EH), H, d_edge_halves);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ======================================================================================================== loops: count

#define NL_INNER (-2)                                       // succ of a half-edge that is not on a BOUNDARY edge

__device__ __forceinline__ bool nl_is_boundary(const int32_t* he, const uint8_t* kind, i64 E, i64 h) {
    const int32_t e = he[h];
    return e >= 0 && e < E && kind[e] == NFL_EDGE_BOUNDARY;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_loops_succ_kernel(const int32_t* he, const int32_t* twin, const uint8_t* kind, i64 E,
                                                                    i64 T, int32_t* succ, int32_t* ptr, int32_t* mn, int32_t* len,
                                                                    i64* totals, i64* raw) {
    const i64 h = (i64)blockIdx.x * NM_THREADS + threadIdx.x, H3 = 3 * T;
    if (h < T) len[h] = 0;
    if (h < NFL_LOOP_TOTALS) totals[h] = 0;
    if (h < 2) raw[h] = 0;
    if (h >= H3) return;
    int32_t r = NL_INNER;
    if (nl_is_boundary(he, kind, E, h)) {
        r = -1;
        i64 g = ne_next(h);
        for (i64 steps = 0; steps <= H3; ++steps) {         // the rotation about the end of h
            const int32_t w = twin[g];
            if (w < 0 || w >= H3) {
                if (nl_is_boundary(he, kind, E, g)) r = (int32_t)g;
                break;
            }
            g = ne_next(w);
        }
    }
    succ[h] = r;
    ptr[h] = r < 0 ? -1 : r;
    mn[h] = (int32_t)h;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_loops_double_kernel(const int32_t* ptr, const int32_t* mn, i64 H3, int32_t* ptr2,
                                                                      int32_t* mn2) {
    const i64 h = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (h >= H3) return;
    int32_t p = ptr[h], m = mn[h];
    if (p >= 0 && p < H3) {
        const int32_t pm = mn[p];
        m = pm < m ? pm : m;
        p = ptr[p];
    } else {
        p = -1;
    }
    ptr2[h] = p;
    mn2[h] = m;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_loops_label_kernel(const int32_t* succ, const int32_t* ptr, const int32_t* mn, i64 H3,
                                                                     int32_t* root, int32_t* flag, i64* n_open) {
    const i64 h = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool open = false;
    if (h < H3) {
        int32_t r = -1;
        if (succ[h] != NL_INNER) {
            const int32_t p = ptr[h], m = mn[h];
            if (p >= 0 && p < H3 && m >= 0 && m < H3) r = m; else open = true;
        }
        root[h] = r;
        flag[h] = r == h ? 1 : 0;
    }
    ng_count_bad(open, n_open);
}

// A thread per loop walks it from its root, in order: the place of every half-edge, the length, the fp64 sums.
__global__ __launch_bounds__(NM_THREADS) void nfl_loops_fold_kernel(const float* ver, const int32_t* tri, i64 V, i64 T,
                                                                    const int32_t* succ, const int32_t* root, const int32_t* flag,
                                                                    const i64* rank, int32_t* pos, int32_t* len, float* per, float* cen) {
    const i64 h = (i64)blockIdx.x * NM_THREADS + threadIdx.x, H3 = 3 * T;
    if (h >= H3 || !flag[h]) return;
    const i64 id = rank[h];
    if (id < 0 || id >= T) return;
    double sum = 0.0, c[3] = {0.0, 0.0, 0.0};
    bool finite = true;
    i64 g = h, k = 0;
    for (;;) {
        pos[g] = (int32_t)k;
        const int32_t a = tri[g], b = tri[ne_next(g)];
        if (a >= 0 && a < V && b >= 0 && b < V) {
            double pa[3], d[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                pa[j] = (double)ver[3 * (i64)a + j];
                d[j] = (double)ver[3 * (i64)b + j] - pa[j];
                finite = finite && ng_is_finite(pa[j]);
                c[j] += pa[j];
            }
            sum += sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        } else {
            finite = false;
        }
        ++k;
        const int32_t nx = succ[g];
        if (nx == h || nx < 0 || nx >= H3 || root[nx] != h || k >= H3) break;
        g = nx;
    }
    len[id] = (int32_t)k;
    const double n = (double)k;
    per[id] = finite ? (float)sum : INFINITY;
#pragma unroll
    for (int j = 0; j < 3; ++j) cen[3 * id + j] = finite ? (float)(c[j] / n) : 0.0f;
}

__global__ __launch_bounds__(64) void nfl_loops_finish_kernel(const i64* raw, i64 T, i64* totals) {
    if (threadIdx.x >= 2) return;
    const i64 v = raw[threadIdx.x], top = threadIdx.x ? 3 * T : T;
    totals[threadIdx.x] = v < 0 ? 0 : v > top ? top : v;
}

extern "C" int nfl_mesh_loops_count(const float* d_vertices, const int32_t* d_triangles, int64_t V, int64_t T,
                                    const int32_t* d_half_edge, const int32_t* d_twin, const void* d_kind, int64_t E, int64_t B,
                                    void* d_scratch, size_t scratch_bytes, int64_t* d_totals, void* stream) {
    if (!nm_sizes_ok(V, T) || !ne_totals_ok(T, E, B)) return NFL_EINVAL;
    if (ng_misaligned(d_vertices, 4) || ng_misaligned(d_triangles, 4) || ng_misaligned(d_half_edge, 4) || ng_misaligned(d_twin, 4)
        || ng_misaligned(d_totals, 8))
        return NFL_EINVAL;
    if (V == 0 || T == 0) return NFL_OK;
    if (!d_vertices || !d_triangles || !d_half_edge || !d_twin || !d_totals || (E && !d_kind)) return NFL_EINVAL;
    NlScratch S = nl_layout(T);
    const int rc = ng_carve(S, d_scratch, scratch_bytes);
    if (rc != NFL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const i64 H3 = 3 * T;
    const uint8_t* kind = static_cast<const uint8_t*>(d_kind);
    int32_t *succ = S.get<int32_t>(NL_SUCC), *root = S.get<int32_t>(NL_ROOT), *flag = S.get<int32_t>(NL_FLAG);
    int32_t *pos = S.get<int32_t>(NL_POS), *len = S.get<int32_t>(NL_LEN);
    int32_t* ptr[2] = {S.get<int32_t>(NL_PTR0), S.get<int32_t>(NL_PTR1)};
    int32_t* mn[2] = {S.get<int32_t>(NL_MIN0), S.get<int32_t>(NL_MIN1)};
    i64 *rank = S.get<i64>(NL_RANK), *loff = S.get<i64>(NL_LOFF), *sums = S.get<i64>(NL_SUMS), *raw = S.get<i64>(NL_RAW);
    hipLaunchKernelGGL(nfl_loops_succ_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, d_half_edge, d_twin, kind, E, T, succ, ptr[0],
                       mn[0], len, d_totals, raw);
    const int rounds = nl_rounds(B);
    int at = 0;
    for (int r = 0; r < rounds; ++r, at ^= 1)
        hipLaunchKernelGGL(nfl_loops_double_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, ptr[at], mn[at], H3, ptr[at ^ 1], mn[at ^ 1]);
    hipLaunchKernelGGL(nfl_loops_label_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, succ, ptr[at], mn[at], H3, root, flag, d_totals + 2);
    nm_scan(flag, rank, H3, sums, raw, s);
    hipLaunchKernelGGL(nfl_loops_fold_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, d_vertices, d_triangles, V, T, succ, root, flag,
                       rank, pos, len, S.get<float>(NL_PER), S.get<float>(NL_CEN));
    nm_scan(len, loff, T, sums, raw + 1, s);
    hipLaunchKernelGGL(nfl_loops_finish_kernel, dim3(1), dim3(64), 0, s, raw, T, d_totals);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ========================================================================================================= loops: emit

__global__ __launch_bounds__(NM_THREADS) void nfl_loops_emit_halves_kernel(const int32_t* root, const i64* rank, const int32_t* pos,
                                                                           const int32_t* len, const i64* loff, i64 H3, i64 L, i64 B,
                                                                           int32_t* loop_of, int32_t* loop_halves) {
    const i64 h = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (h >= H3) return;
    int32_t id = -1;
    const int32_t r = root[h];
    if (r >= 0 && r < H3) {
        const i64 l = rank[r];
        if (l >= 0 && l < L) {
            const i64 o = loff[l], p = pos[h];
            if (o >= 0 && p >= 0 && p < len[l] && o + p < B) {
                id = (int32_t)l;
                loop_halves[o + p] = (int32_t)h;
            }
        }
    }
    loop_of[h] = id;
}

// thread l of L + 1: the offset (B at L), the table's row
__global__ __launch_bounds__(NM_THREADS) void nfl_loops_emit_table_kernel(const i64* loff, const int32_t* len, const float* per,
                                                                          const float* cen, i64 L, i64 B, i64* out_off, int32_t* out_len,
                                                                          float* out_per, float* out_cen) {
    const i64 l = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (l > L) return;
    const i64 o = l < L ? loff[l] : B;
    out_off[l] = o < 0 ? 0 : o > B ? B : o;
    if (l == L) return;
    out_len[l] = len[l];
    out_per[l] = per[l];
#pragma unroll
    for (int j = 0; j < 3; ++j) out_cen[3 * l + j] = cen[3 * l + j];
}

extern "C" int nfl_mesh_loops_emit(int64_t T, const void* d_scratch, size_t scratch_bytes, int64_t L, int64_t B,
                                   int64_t* d_loop_offsets, int32_t* d_loop_halves, int32_t* d_loop_of, int32_t* d_length,
                                   float* d_perimeter, float* d_centroid, void* stream) {
    if (!nm_sizes_ok(0, T) || !nl_totals_ok(T, L, B)) return NFL_EINVAL;
    if (ng_misaligned(d_loop_offsets, 8) || ng_misaligned(d_loop_halves, 4) || ng_misaligned(d_loop_of, 4) || ng_misaligned(d_length, 4)
        || ng_misaligned(d_perimeter, 4) || ng_misaligned(d_centroid, 4))
        return NFL_EINVAL;
    if (T == 0) return NFL_OK;
    if (!d_loop_offsets || !d_loop_of || (L && (!d_length || !d_perimeter || !d_centroid)) || (B && !d_loop_halves)) return NFL_EINVAL;
    NlScratch S = nl_layout(T);
    const int rc = ng_carve(S, const_cast<void*>(d_scratch), scratch_bytes);
    if (rc != NFL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const i64 H3 = 3 * T;
    const int32_t* len = S.get<int32_t>(NL_LEN);
    const i64* loff = S.get<i64>(NL_LOFF);
    hipLaunchKernelGGL(nfl_loops_emit_halves_kernel, dim3(nm_grid(H3)), dim3(NM_THREADS), 0, s, S.get<int32_t>(NL_ROOT),
                       S.get<i64>(NL_RANK), S.get<int32_t>(NL_POS), len, loff, H3, L, B, d_loop_of, d_loop_halves);
    hipLaunchKernelGGL(nfl_loops_emit_table_kernel, dim3(nm_grid(L + 1)), dim3(NM_THREADS), 0, s, loff, len, S.get<float>(NL_PER),
                       S.get<float>(NL_CEN), L, B, d_loop_offsets, d_length, d_perimeter, d_centroid);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ================================================================================================================= fill

__global__ __launch_bounds__(64) void nfl_fill_zero_kernel(i64* totals) {
    if (threadIdx.x < NFL_FILL_TOTALS) totals[threadIdx.x] = 0;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_fill_select_kernel(const int32_t* length, const float* perimeter, const uint8_t* keep,
                                                                     i64 L, i64 max_edges, float max_perimeter, int32_t* len,
                                                                     int32_t* nv, int32_t* nt, i64* n_filled) {
    const i64 l = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool sel = false;
    if (l < L) {
        const int32_t n = length[l];
        const float p = perimeter[l];
        sel = n >= 3 && n <= max_edges && ng_is_finite(p) && p <= max_perimeter && (!keep || keep[l]);
        len[l] = sel ? n : 0;
        nv[l] = sel && n > 3 ? 1 : 0;
        nt[l] = sel ? (n == 3 ? 1 : n) : 0;
    }
    ng_count_bad(sel, n_filled);
}

extern "C" int nfl_mesh_fill_count(int64_t L, const int32_t* d_length, const float* d_perimeter, const void* d_keep,
                                   int64_t max_edges, float max_perimeter, void* d_scratch, size_t scratch_bytes,
                                   int64_t* d_totals, void* stream) {
    if (L < 0 || L > INT32_MAX / 3 || max_edges < 3 || !(max_perimeter > 0.f)) return NFL_EINVAL;
    if (ng_misaligned(d_length, 4) || ng_misaligned(d_perimeter, 4) || ng_misaligned(d_totals, 8)) return NFL_EINVAL;
    if (L == 0) return NFL_OK;
    if (!d_length || !d_perimeter || !d_totals) return NFL_EINVAL;
    NfScratch S = nf_layout(L);
    const int rc = ng_carve(S, d_scratch, scratch_bytes);
    if (rc != NFL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t *nv = S.get<int32_t>(NF_NV), *nt = S.get<int32_t>(NF_NT);
    i64* sums = S.get<i64>(NF_SUMS);
    hipLaunchKernelGGL(nfl_fill_zero_kernel, dim3(1), dim3(64), 0, s, d_totals);
    hipLaunchKernelGGL(nfl_fill_select_kernel, dim3(nm_grid(L)), dim3(NM_THREADS), 0, s, d_length, d_perimeter,
                       static_cast<const uint8_t*>(d_keep), L, max_edges, max_perimeter, S.get<int32_t>(NF_LEN), nv, nt, d_totals);
    nm_scan(nv, S.get<i64>(NF_VOFF), L, sums, d_totals + 1, s);
    nm_scan(nt, S.get<i64>(NF_TOFF), L, sums, d_totals + 2, s);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// out[0 .. n) = in, out[n .. n + extra) left to the kernels below; flag = 0 for the old rows and 1 for the new ones
__global__ __launch_bounds__(NM_THREADS) void nfl_fill_copy_kernel(const int32_t* in, i64 words, int32_t* out, i64 rows, i64 extra,
                                                                   uint8_t* flag) {
    for (i64 i = (i64)blockIdx.x * NM_THREADS + threadIdx.x; i < words || i < rows + extra; i += (i64)gridDim.x * NM_THREADS) {
        if (i < words) out[i] = in[i];
        if (flag && i < rows + extra) flag[i] = i >= rows;
    }
}

// the start vertex of half-edge h of the caller's loop rows, -1 unless both are in range
__device__ __forceinline__ int32_t nf_start(const int32_t* tri, i64 V, i64 H3, int32_t h) {
    if (h < 0 || h >= H3) return -1;
    const int32_t a = tri[h];
    return a >= 0 && a < V ? a : -1;
}

// a thread per entry of loop_halves: the triangle that covers it
__global__ __launch_bounds__(NM_THREADS) void nfl_fill_triangles_kernel(const int32_t* tri, i64 V, i64 T, const i64* loff,
                                                                        const int32_t* halves, const int32_t* loop_of, i64 L, i64 B,
                                                                        const int32_t* len, const i64* voff, const i64* toff, i64 n_new_v,
                                                                        i64 n_new_t, int32_t* out) {
    const i64 j = (i64)blockIdx.x * NM_THREADS + threadIdx.x, H3 = 3 * T;
    if (j >= B) return;
    const int32_t h = halves[j];
    if (h < 0 || h >= H3) return;
    const int32_t l = loop_of[h];
    if (l < 0 || l >= L) return;
    const i64 n = len[l], o = loff[l], p = j - o, to = toff[l];
    if (n < 3 || o < 0 || o + n > B || p < 0 || p >= n || to < 0) return;
    const int32_t a = nf_start(tri, V, H3, h);
    int32_t b, c;
    i64 at;
    if (n == 3) {                                           // a -> b, b -> c, c -> a: the one triangle (b, a, c)
        if (p != 0) return;
        b = nf_start(tri, V, H3, halves[o + 1]);
        c = nf_start(tri, V, H3, halves[o + 2]);
        at = to;
    } else {                                                // a -> b: (b, a, z)
        const i64 z = voff[l];
        b = nf_start(tri, V, H3, (int32_t)ne_next(h));
        c = z >= 0 && z < n_new_v ? (int32_t)(V + z) : -1;
        at = to + p;
    }
    if (a < 0 || b < 0 || c < 0 || at >= n_new_t) return;
    out[3 * (T + at)] = b;
    out[3 * (T + at) + 1] = a;
    out[3 * (T + at) + 2] = c;
}

// a thread per loop of more than 3: its vertex.  The sums are fp64, in walk order.
__global__ __launch_bounds__(NM_THREADS) void nfl_fill_vertices_kernel(const float* ver, const float* col, const int32_t* tri, i64 V, i64 T,
                                                                       const i64* loff, const int32_t* halves, const float* centroid, i64 L,
                                                                       i64 B, const int32_t* len, const i64* voff, i64 n_new_v,
                                                                       float* out_ver, float* out_nrm, float* out_col) {
    const i64 l = (i64)blockIdx.x * NM_THREADS + threadIdx.x, H3 = 3 * T;
    if (l >= L) return;
    const i64 n = len[l], o = loff[l], z = voff[l];
    if (n <= 3 || o < 0 || o + n > B || z < 0 || z >= n_new_v) return;
    const float zf[3] = {centroid[3 * l], centroid[3 * l + 1], centroid[3 * l + 2]};
    const double p2[3] = {(double)zf[0], (double)zf[1], (double)zf[2]};
    double s[3] = {0.0, 0.0, 0.0}, cs[3] = {0.0, 0.0, 0.0};
    for (i64 k = 0; k < n; ++k) {
        const int32_t h = halves[o + k];
        const int32_t a = nf_start(tri, V, H3, h), b = h >= 0 && h < H3 ? nf_start(tri, V, H3, (int32_t)ne_next(h)) : -1;
        if (a < 0 || b < 0) continue;
        double p0[3], p1[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            p0[q] = (double)ver[3 * (i64)b + q];
            p1[q] = (double)ver[3 * (i64)a + q];
            if (col) cs[q] += (double)col[3 * (i64)a + q];
        }
        const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        s[0] += e1[1] * e2[2] - e1[2] * e2[1];
        s[1] += e1[2] * e2[0] - e1[0] * e2[2];
        s[2] += e1[0] * e2[1] - e1[1] * e2[0];
    }
    const double norm = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const bool ok = norm > 0.0 && ng_is_finite(norm);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        out_ver[3 * (V + z) + q] = zf[q];
        out_nrm[3 * (V + z) + q] = ok ? (float)(s[q] / norm) : 0.0f;
        if (col) out_col[3 * (V + z) + q] = (float)(cs[q] / (double)n);
    }
}

extern "C" int nfl_mesh_fill_emit(const float* d_vertices, const float* d_normals, const float* d_colors, const int32_t* d_triangles,
                                  int64_t V, int64_t T, const int64_t* d_loop_offsets, const int32_t* d_loop_halves,
                                  const int32_t* d_loop_of, const float* d_centroid, int64_t L, int64_t B, const void* d_scratch,
                                  size_t scratch_bytes, int64_t n_new_vertices, int64_t n_new_triangles, float* d_out_vertices,
                                  float* d_out_normals, float* d_out_colors, int32_t* d_out_triangles, void* d_new_vertices,
                                  void* d_new_triangles, void* stream) {
    if (!nm_sizes_ok(V, T) || !nl_totals_ok(T, L, B) || !nf_totals_ok(L, B, n_new_vertices, n_new_triangles)) return NFL_EINVAL;
    if (!nm_sizes_ok(V + n_new_vertices, T + n_new_triangles)) return NFL_EINVAL;
    const void* four[] = {d_vertices, d_normals, d_colors, d_triangles, d_loop_halves, d_loop_of, d_centroid, d_out_vertices,
                          d_out_normals, d_out_colors, d_out_triangles};
    for (const void* p : four)
        if (ng_misaligned(p, 4)) return NFL_EINVAL;
    if (ng_misaligned(d_loop_offsets, 8) || (d_colors == nullptr) != (d_out_colors == nullptr)) return NFL_EINVAL;
    if (V == 0 || T == 0 || L == 0) return NFL_OK;
    if (!d_vertices || !d_normals || !d_triangles || !d_loop_offsets || !d_loop_halves || !d_loop_of || !d_centroid) return NFL_EINVAL;
    if (!d_out_vertices || !d_out_normals || !d_out_triangles) return NFL_EINVAL;
    NfScratch S = nf_layout(L);
    const int rc = ng_carve(S, const_cast<void*>(d_scratch), scratch_bytes);
    if (rc != NFL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const i64 nv = n_new_vertices, nt = n_new_triangles;
    const int32_t* len = S.get<int32_t>(NF_LEN);
    const i64 *voff = S.get<i64>(NF_VOFF), *toff = S.get<i64>(NF_TOFF);
    const float* rows_in[3] = {d_vertices, d_normals, d_colors};
    float* rows_out[3] = {d_out_vertices, d_out_normals, d_out_colors};
    for (int k = 0; k < 3; ++k)
        if (rows_in[k])
            hipLaunchKernelGGL(nfl_fill_copy_kernel, dim3(ne_bounded_grid(3 * V)), dim3(NM_THREADS), 0, s,
                               reinterpret_cast<const int32_t*>(rows_in[k]), 3 * V, reinterpret_cast<int32_t*>(rows_out[k]), V, nv,
                               k == 0 ? static_cast<uint8_t*>(d_new_vertices) : nullptr);
    hipLaunchKernelGGL(nfl_fill_copy_kernel, dim3(ne_bounded_grid(3 * T)), dim3(NM_THREADS), 0, s, d_triangles, 3 * T, d_out_triangles, T, nt,
                       static_cast<uint8_t*>(d_new_triangles));
    if (nt && B)
        hipLaunchKernelGGL(nfl_fill_triangles_kernel, dim3(nm_grid(B)), dim3(NM_THREADS), 0, s, d_triangles, V, T, d_loop_offsets,
                           d_loop_halves, d_loop_of, L, B, len, voff, toff, nv, nt, d_out_triangles);
    if (nv)
        hipLaunchKernelGGL(nfl_fill_vertices_kernel, dim3(nm_grid(L)), dim3(NM_THREADS), 0, s, d_vertices, d_colors, d_triangles, V, T,
                           d_loop_offsets, d_loop_halves, d_centroid, L, B, len, voff, nv, d_out_vertices, d_out_normals, d_out_colors);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
