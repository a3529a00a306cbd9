// nfl_mesh.hip -- cleaning an indexed triangle mesh on the device (include/nerf_fl_amd.h, "mesh"): connected components,
// a per-component table, compaction under a per-component keep flag.  DESIGN.md section 19.
//
//   label    init     parent[v] = v; the ignored-triangle counter = 0
//            hook     one thread per triangle: lock-free union-find.  find() walks parent[] by agent-scope atomic loads
//                     and halves the path behind it (path splitting: a NON-root's parent is replaced by an ancestor, which
//                     can race with nothing but other such replacements); unite() points the LARGER root at the SMALLER by
//                     an agent-scope compare-and-swap on a word that still holds its own index, and starts over when it
//                     lost the race.  parent[x] <= x at all times, so a root is the smallest index of its tree, and when
//                     the launch ends a tree is a whole component: the roots do not depend on the order of arrival.
//            flatten  component[v] = find(v) (the same find: only path splitting races in this launch), flag[v] = root == v
//            scan     exclusive scan of the flags: rank of every root; the total is C
//            rank     component[v] = rank[component[v]]
//   stats    init, one pass over the vertices (count, min / max of the positions through the order-preserving integer map),
//            one over the triangles (count by the first index), decode of the bounds in place.  Equal ids of a wave are
//            combined (leader's id, ballot, popcount / butterfly min-max) before one atomic per distinct id.
//   compact  count: flags of kept vertices and kept triangles, two scans, the totals;  emit: kept rows in their order.
//
// The scan is one routine (nm_scan): tiles of NM_SCAN_TILE elements, a workgroup per tile, the tile sums scanned by the
// same kernel one level up until one tile is left (three levels cover 2^31 elements), then added back level by level:
// a fixed order, int32 in, int64 out.  Only integer adds, min and max are taken atomically, so every output is
// bit-reproducible.  Nothing here allocates, sets or copies memory through the runtime.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_mesh_scan.h"

#define NM_KEY_POS_INF 0xFF800000u                          // nm_key(+inf)
#define NM_KEY_NEG_INF 0x007FFFFFu                          // nm_key(-inf)

// ---------------------------------------------------------------------------------------------------------------- scan

// tile sums of all levels above the elements themselves, 8 B each
size_t nm_scan_bytes(i64 n) {
    size_t entries = 0;
    for (i64 m = nm_cdiv(n, NM_SCAN_TILE); m > 1; m = nm_cdiv(m, NM_SCAN_TILE)) entries += (size_t)m;
    return nm_pad(entries * 8);
}

// one tile: out[i] = sum of in[tile start .. i), sums[tile] = sum of the tile.  in == out is allowed (a thread reads its
// items before it writes them)
template <typename Tin>
__global__ __launch_bounds__(NM_SCAN_THREADS) void nfl_mesh_scan_tile_kernel(const Tin* in, i64* out, i64 n, i64* sums) {
    __shared__ i64 wave_sum[NM_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 i0 = (i64)blockIdx.x * NM_SCAN_TILE + (i64)tid * NM_SCAN_ITEMS;
    i64 v[NM_SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < NM_SCAN_ITEMS; ++j) {
        v[j] = i0 + j < n ? (i64)in[i0 + j] : 0;
        mine += v[j];
    }
    i64 incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const i64 up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    i64 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NM_SCAN_THREADS / 64; ++w) {
        const i64 s = wave_sum[w];
        if (w < wave) before += s;
        all += s;
    }
    i64 run = before + incl - mine;
#pragma unroll
    for (int j = 0; j < NM_SCAN_ITEMS; ++j) {
        if (i0 + j < n) out[i0 + j] = run;
        run += v[j];
    }
    if (tid == 0) sums[blockIdx.x] = all;
}

// out[i] += sums[tile of i]: the scanned level above, added back
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_scan_add_kernel(i64* out, i64 n, const i64* sums) {
    const i64 i = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (i < n) out[i] += sums[i / NM_SCAN_TILE];
}

__global__ __launch_bounds__(64) void nfl_mesh_zero_total_kernel(i64* total) {
    if (threadIdx.x == 0) *total = 0;
}

// out (n) int64 = exclusive prefix sums of in (n) int32, *total = their sum; `sums`: nm_scan_bytes(n) of scratch
void nm_scan(const int32_t* in, i64* out, i64 n, i64* sums, i64* total, hipStream_t s) {
    if (n == 0) {
        hipLaunchKernelGGL(nfl_mesh_zero_total_kernel, dim3(1), dim3(64), 0, s, total);
        return;
    }
    i64* buf[NM_SCAN_LEVELS + 1] = {out, nullptr, nullptr, nullptr};
    i64 len[NM_SCAN_LEVELS + 1] = {n, 0, 0, 0};
    int top = 0;
    for (;; ++top) {                                        // scan level `top`; its tile sums are level top + 1
        const i64 tiles = nm_cdiv(len[top], NM_SCAN_TILE);
        len[top + 1] = tiles;
        buf[top + 1] = tiles == 1 ? total : sums;
        if (top == 0)
            hipLaunchKernelGGL(nfl_mesh_scan_tile_kernel<int32_t>, dim3((unsigned)tiles), dim3(NM_SCAN_THREADS), 0, s, in,
                               buf[0], len[0], buf[1]);
        else
            hipLaunchKernelGGL(nfl_mesh_scan_tile_kernel<i64>, dim3((unsigned)tiles), dim3(NM_SCAN_THREADS), 0, s, buf[top],
                               buf[top], len[top], buf[top + 1]);
        if (tiles == 1) break;
        sums += tiles;
    }
    for (int k = top - 1; k >= 0; --k)
        hipLaunchKernelGGL(nfl_mesh_scan_add_kernel, dim3(nm_grid(len[k])), dim3(NM_THREADS), 0, s, buf[k], len[k], buf[k + 1]);
}

// --------------------------------------------------------------------------------------------------------------- label

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_init_kernel(int32_t* parent, i64 V, i64* ignored) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v < V) parent[v] = (int32_t)v;
    if (v == 0) *ignored = 0;
}

// the root of x's tree; every node passed on the way is pointed at its grandparent
__device__ __forceinline__ int32_t nm_find(int32_t* parent, int32_t x) {
    int32_t p = NM_LOAD(parent + x);
    while (p != x) {
        const int32_t g = NM_LOAD(parent + p);
        if (g != p) NM_STORE(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void nm_unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = nm_find(parent, a);
        b = nm_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        int32_t expected = a;                               // still a root: it becomes a child of the smaller one
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_hook_kernel(const int32_t* tri, i64 V, i64 T, int32_t* parent,
                                                                   i64* ignored) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    bool bad = false;
    if (t < T) {
        const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        if (nm_in_range(a, b, c, V)) {
            if (a != b) nm_unite(parent, a, b);
            if (b != c) nm_unite(parent, b, c);
        } else {
            bad = true;
        }
    }
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63) == __ffsll(m) - 1) atomicAdd(reinterpret_cast<unsigned long long*>(ignored), (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_flatten_kernel(int32_t* parent, i64 V, int32_t* root, int32_t* flag) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= V) return;
    const int32_t r = nm_find(parent, (int32_t)v);
    root[v] = r;
    flag[v] = r == v ? 1 : 0;
}

// component holds roots on entry; a thread touches its own element only
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_rank_kernel(int32_t* component, i64 V, const i64* rank) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v < V) component[v] = (int32_t)rank[component[v]];
}

extern "C" size_t nfl_mesh_label_bytes(int64_t V, int64_t T) {
    if (!nm_sizes_ok(V, T)) return 0;
    return nm_pad((size_t)V * 4) * 2 + nm_pad((size_t)V * 8) + nm_scan_bytes(V);        // parent, flag, rank, tile sums
}

extern "C" int nfl_mesh_label(const nfl_mesh_label_args* a, void* stream) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles) || !a->d_totals) return NFL_EINVAL;
    const i64 V = a->n_vertices, T = a->n_triangles;
    if (T && !a->d_triangles) return NFL_EINVAL;
    if (V == 0) return NFL_OK;
    if (!a->d_component || !a->d_scratch || reinterpret_cast<uintptr_t>(a->d_scratch) % 8) return NFL_EINVAL;
    if (a->scratch_bytes < nfl_mesh_label_bytes(V, T)) return NFL_ESMALL;
    char* p = static_cast<char*>(a->d_scratch);
    int32_t* parent = reinterpret_cast<int32_t*>(p);
    int32_t* flag = reinterpret_cast<int32_t*>(p + nm_pad((size_t)V * 4));
    i64* rank = reinterpret_cast<i64*>(p + 2 * nm_pad((size_t)V * 4));
    i64* sums = reinterpret_cast<i64*>(p + 2 * nm_pad((size_t)V * 4) + nm_pad((size_t)V * 8));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nfl_mesh_init_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, parent, V, a->d_totals + 1);
    if (T) hipLaunchKernelGGL(nfl_mesh_hook_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_triangles, V, T, parent, a->d_totals + 1);
    hipLaunchKernelGGL(nfl_mesh_flatten_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, parent, V, a->d_component, flag);
    nm_scan(flag, rank, V, sums, a->d_totals, s);
    hipLaunchKernelGGL(nfl_mesh_rank_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_component, V, rank);
    return nm_launched() ? NFL_OK : NFL_ELAUNCH;
}

// --------------------------------------------------------------------------------------------------------------- stats

// fp32 -> uint32 with the order of the floats (-0 below +0); NaN never gets here
__device__ __forceinline__ uint32_t nm_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float nm_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_stats_init_kernel(i64 C, int32_t* n_ver, int32_t* n_tri, uint32_t* keys) {
    const i64 c = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (c >= C) return;
    n_ver[c] = 0;
    n_tri[c] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        keys[6 * c + k] = NM_KEY_POS_INF;
        keys[6 * c + 3 + k] = NM_KEY_NEG_INF;
    }
}

// Adds 1 to count[id] for every lane with `valid`, one atomic per distinct id of the wave; with BOUNDS also folds
// the lane's six keys (min of lo[], max of hi[]) into the bounds of id.  Every lane of the wave must call it.
template <bool BOUNDS>
__device__ __forceinline__ void nm_wave_combine(bool valid, int32_t id, int32_t* count, uint32_t* keys, const uint32_t lo[3],
                                                const uint32_t hi[3]) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(valid);
    while (pending) {                                       // wave-uniform
        const int leader = __ffsll(pending) - 1;
        const int32_t lid = __shfl(id, leader);
        const bool member = valid && id == lid;
        const unsigned long long same = __ballot(member);
        if constexpr (BOUNDS) {
            uint32_t mn[3], mx[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mn[k] = member ? lo[k] : 0xFFFFFFFFu;
                mx[k] = member ? hi[k] : 0u;
            }
            if (same & (same - 1)) {                        // more than one member: butterfly over the wave
#pragma unroll
                for (int off = 32; off > 0; off >>= 1)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        mn[k] = min(mn[k], (uint32_t)__shfl_xor((int)mn[k], off));
                        mx[k] = max(mx[k], (uint32_t)__shfl_xor((int)mx[k], off));
                    }
            }
            if (lane == leader) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {               // lanes without a finite coordinate left the neutral key
                    if (mn[k] != 0xFFFFFFFFu) atomicMin(keys + 6 * (i64)lid + k, mn[k]);
                    if (mx[k] != 0u) atomicMax(keys + 6 * (i64)lid + 3 + k, mx[k]);
                }
            }
        }
        if (lane == leader) atomicAdd(count + lid, (int32_t)__popcll(same));
        pending &= ~same;
    }
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_stats_vertices_kernel(const int32_t* component, const float* pos, i64 V,
                                                                             i64 C, int32_t* n_ver, uint32_t* keys) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    int32_t id = -1;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (v < V) {
        id = component[v];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float f = pos[3 * v + k];
            if (isfinite(f)) lo[k] = hi[k] = nm_key(f);     // a finite key is neither 0 nor 0xFFFFFFFF
        }
    }
    nm_wave_combine<true>(id >= 0 && id < C, id, n_ver, keys, lo, hi);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_stats_triangles_kernel(const int32_t* component, const int32_t* tri, i64 V,
                                                                              i64 T, i64 C, int32_t* n_tri) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    int32_t id = -1;
    if (t < T) {
        const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        if (nm_in_range(a, b, c, V)) id = component[a];
    }
    nm_wave_combine<false>(id >= 0 && id < C, id, n_tri, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_stats_decode_kernel(i64 n, uint32_t* keys) {
    const i64 i = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (i < n) keys[i] = __float_as_uint(nm_unkey(keys[i]));
}

extern "C" int nfl_mesh_stats(const nfl_mesh_stats_args* a, void* stream) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    const i64 V = a->n_vertices, T = a->n_triangles, C = a->n_components;
    if (C < 0 || C > V) return NFL_EINVAL;
    if (C == 0) return NFL_OK;
    if (!a->d_component || !a->d_positions || (T && !a->d_triangles)) return NFL_EINVAL;
    if (!a->d_n_vertices || !a->d_n_triangles || !a->d_bounds) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* keys = reinterpret_cast<uint32_t*>(a->d_bounds);
    hipLaunchKernelGGL(nfl_mesh_stats_init_kernel, dim3(nm_grid(C)), dim3(NM_THREADS), 0, s, C, a->d_n_vertices, a->d_n_triangles, keys);
    hipLaunchKernelGGL(nfl_mesh_stats_vertices_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_component, a->d_positions, V, C,
                       a->d_n_vertices, keys);
    if (T) hipLaunchKernelGGL(nfl_mesh_stats_triangles_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_component, a->d_triangles,
                              V, T, C, a->d_n_triangles);
    hipLaunchKernelGGL(nfl_mesh_stats_decode_kernel, dim3(nm_grid(6 * C)), dim3(NM_THREADS), 0, s, 6 * C, keys);
    return nm_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ------------------------------------------------------------------------------------------------------------- compact

// The scratch of count and emit, in this order, every part padded to 16 B: the flags and offsets of the vertices
// (4 + 8 B each), those of the triangles (4 + 8 B each), then ONE region of tile sums, sized for the longer of the two
// scans: the vertex scan has finished with it (its sums are added back) before the triangle scan, next in the stream, starts.
struct NmCompact {
    int32_t* flag_v;        // (V) 1 = kept
    i64* off_v;             // (V) kept vertices before v
    int32_t* flag_t;        // (T)
    i64* off_t;             // (T)
    i64* sums;              // tile sums of the larger of the two scans (they run one after the other)
};

extern "C" size_t nfl_mesh_compact_bytes(int64_t V, int64_t T) {
    if (!nm_sizes_ok(V, T)) return 0;
    return nm_pad((size_t)V * 4) + nm_pad((size_t)V * 8) + nm_pad((size_t)T * 4) + nm_pad((size_t)T * 8)
           + nm_max(nm_scan_bytes(V), nm_scan_bytes(T));
}

// Checks shared by count and emit.  emit reads neither d_component nor d_keep, but takes the arguments of the count call
// unchanged, so both calls refuse the same ones.
static int nm_carve(const nfl_mesh_compact_args* a, NmCompact& S) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    const i64 V = a->n_vertices, T = a->n_triangles, C = a->n_components;
    if (C < 0 || C > V) return NFL_EINVAL;
    if (V && (!a->d_component || !a->d_keep)) return NFL_EINVAL;
    if (T && !a->d_triangles) return NFL_EINVAL;
    if (V + T == 0) return NFL_OK;
    if (!a->d_scratch || reinterpret_cast<uintptr_t>(a->d_scratch) % 8) return NFL_EINVAL;
    if (a->scratch_bytes < nfl_mesh_compact_bytes(V, T)) return NFL_ESMALL;
    char* p = static_cast<char*>(a->d_scratch);
    S.flag_v = reinterpret_cast<int32_t*>(p);   p += nm_pad((size_t)V * 4);
    S.off_v = reinterpret_cast<i64*>(p);        p += nm_pad((size_t)V * 8);
    S.flag_t = reinterpret_cast<int32_t*>(p);   p += nm_pad((size_t)T * 4);
    S.off_t = reinterpret_cast<i64*>(p);        p += nm_pad((size_t)T * 8);
    S.sums = reinterpret_cast<i64*>(p);
    return NFL_OK;
}

__device__ __forceinline__ bool nm_kept(const int32_t* component, const uint8_t* keep, i64 C, int32_t v) {
    const int32_t id = component[v];
    return id >= 0 && id < C && keep[id] != 0;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_keep_vertices_kernel(const int32_t* component, const uint8_t* keep, i64 V, i64 C,
                                                                            int32_t* flag) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v < V) flag[v] = nm_kept(component, keep, C, (int32_t)v) ? 1 : 0;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_keep_triangles_kernel(const int32_t* component, const uint8_t* keep,
                                                                             const int32_t* tri, i64 V, i64 T, i64 C, int32_t* flag) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (t >= T) return;
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    // all three, so that a component array which is not the labelling of THESE triangles cannot leave a dangling index
    flag[t] = (nm_in_range(a, b, c, V) && nm_kept(component, keep, C, a) && nm_kept(component, keep, C, b)
               && nm_kept(component, keep, C, c)) ? 1 : 0;
}

extern "C" int nfl_mesh_compact_count(const nfl_mesh_compact_args* a, void* stream) {
    NmCompact S;
    const int rc = nm_carve(a, S);
    if (rc != NFL_OK) return rc;
    if (!a->d_totals) return NFL_EINVAL;
    const i64 V = a->n_vertices, T = a->n_triangles, C = a->n_components;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (V) hipLaunchKernelGGL(nfl_mesh_keep_vertices_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_component, a->d_keep, V, C, S.flag_v);
    if (T) hipLaunchKernelGGL(nfl_mesh_keep_triangles_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_component, a->d_keep,
                              a->d_triangles, V, T, C, S.flag_t);
    nm_scan(S.flag_v, S.off_v, V, S.sums, a->d_totals, s);
    nm_scan(S.flag_t, S.off_t, T, S.sums, a->d_totals + 1, s);
    return nm_launched() ? NFL_OK : NFL_ELAUNCH;
}

struct NmRows {
    const float* in[3];
    float* out[3];
};

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_emit_vertices_kernel(const int32_t* flag, const i64* off, i64 V, i64 n_kept,
                                                                            const NmRows R) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= V || !flag[v]) return;
    const i64 o = off[v];
    if (o < 0 || o >= n_kept) return;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (!R.in[r]) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) R.out[r][3 * o + k] = R.in[r][3 * v + k];
    }
}

// The scratch is the caller's: should it not be what the count call left, the indices and offsets read from it are
// checked like any others and the triangle is skipped, so nothing is read or written out of range.
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_emit_triangles_kernel(const int32_t* flag, const i64* off, const int32_t* tri,
                                                                             const i64* off_v, i64 V, i64 T, i64 n_kept_v, i64 n_kept,
                                                                             int32_t* out) {
    const i64 t = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (t >= T || !flag[t]) return;                         // a flagged triangle has its three indices in range and kept
    const i64 o = off[t];
    if (o < 0 || o >= n_kept) return;
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (!nm_in_range(a, b, c, V)) return;
    const i64 na = off_v[a], nb = off_v[b], nc = off_v[c];
    if (na < 0 || nb < 0 || nc < 0 || na >= n_kept_v || nb >= n_kept_v || nc >= n_kept_v) return;
    out[3 * o] = (int32_t)na;
    out[3 * o + 1] = (int32_t)nb;
    out[3 * o + 2] = (int32_t)nc;
}

extern "C" int nfl_mesh_compact_emit(const nfl_mesh_compact_args* a, void* stream) {
    NmCompact S;
    const int rc = nm_carve(a, S);
    if (rc != NFL_OK) return rc;
    const i64 V = a->n_vertices, T = a->n_triangles, Vk = a->n_kept_vertices, Tk = a->n_kept_triangles;
    if (Vk < 0 || Tk < 0 || Vk > V || Tk > T) return NFL_EINVAL;
    if (Vk == 0 && Tk == 0) return NFL_OK;
    NmRows R = {{a->d_vertices, a->d_normals, a->d_colors}, {a->d_out_vertices, a->d_out_normals, a->d_out_colors}};
    for (int r = 0; r < 3; ++r)
        if (Vk && R.in[r] && !R.out[r]) return NFL_EINVAL;
    if (Tk && !a->d_out_triangles) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Vk && (R.in[0] || R.in[1] || R.in[2]))
        hipLaunchKernelGGL(nfl_mesh_emit_vertices_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, S.flag_v, S.off_v, V, Vk, R);
    if (Tk) hipLaunchKernelGGL(nfl_mesh_emit_triangles_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, S.flag_t, S.off_t,
                               a->d_triangles, S.off_v, V, T, Vk, Tk, a->d_out_triangles);
    return nm_launched() ? NFL_OK : NFL_ELAUNCH;
}
