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
// The scans are nm_scan (nfl_mesh_scan.hip): a fixed order, int32 in, int64 out.  Only integer adds, min and max are taken
// atomically, so every output is bit-reproducible.  Nothing here allocates, sets or copies memory through the runtime.
#include <math.h>

#include "nfl_geom.h"

#define NM_KEY_POS_INF 0xFF800000u                          // nm_key(+inf)
#define NM_KEY_NEG_INF 0x007FFFFFu                          // nm_key(-inf)

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
    ng_count_bad(bad, ignored);
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_flatten_kernel(int32_t* parent, i64 V, int32_t* root, int32_t* flag) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= V) return;
    const int32_t r = nm_find(parent, (int32_t)v);
    root[v] = r;
    flag[v] = r == v ? 1 : 0;
}

extern "C" size_t nfl_mesh_label_bytes(int64_t V, int64_t T) {
    if (!nm_sizes_ok(V, T)) return 0;
    return ng_bytes(nm_label_layout(V));
}

extern "C" int nfl_mesh_label(const nfl_mesh_label_args* a, void* stream) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles) || !a->d_totals) return NFL_EINVAL;
    const i64 V = a->n_vertices, T = a->n_triangles;
    if (T && !a->d_triangles) return NFL_EINVAL;
    if (V == 0) return NFL_OK;
    if (!a->d_component) return NFL_EINVAL;
    auto L = nm_label_layout(V);
    const int rc = ng_carve(L, a->d_scratch, a->scratch_bytes);
    if (rc != NFL_OK) return rc;
    int32_t *parent = L.get<int32_t>(NM_L_PARENT), *flag = L.get<int32_t>(NM_L_FLAG);
    i64 *rank = L.get<i64>(NM_L_RANK), *sums = L.get<i64>(NM_L_SUMS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nfl_mesh_init_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, parent, V, a->d_totals + 1);
    if (T) hipLaunchKernelGGL(nfl_mesh_hook_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_triangles, V, T, parent, a->d_totals + 1);
    hipLaunchKernelGGL(nfl_mesh_flatten_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, parent, V, a->d_component, flag);
    nm_scan(flag, rank, V, sums, a->d_totals, s);
    nm_rank(a->d_component, V, rank, s);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
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
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ------------------------------------------------------------------------------------------------------------- compact

// the scratch of count and emit: nm_compact_layout (nfl_geom_layout.h)
typedef NgLayout<NM_C_REGIONS> NmCompact;

extern "C" size_t nfl_mesh_compact_bytes(int64_t V, int64_t T) {
    if (!nm_sizes_ok(V, T)) return 0;
    return ng_bytes(nm_compact_layout(V, T));
}

// Checks shared by count and emit.  emit reads neither d_component nor d_keep, but takes the arguments of the count call
// unchanged, so both calls refuse the same ones.
static int nm_carve(const nfl_mesh_compact_args* a, NmCompact& S) {
    if (!a || !nm_sizes_ok(a->n_vertices, a->n_triangles)) return NFL_EINVAL;
    const i64 V = a->n_vertices, T = a->n_triangles, C = a->n_components;
    if (C < 0 || C > V) return NFL_EINVAL;
    if (V && (!a->d_component || !a->d_keep)) return NFL_EINVAL;
    if (T && !a->d_triangles) return NFL_EINVAL;
    S = nm_compact_layout(V, T);
    if (V + T == 0) return NFL_OK;
    return ng_carve(S, a->d_scratch, a->scratch_bytes);
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
    int32_t *flag_v = S.get<int32_t>(NM_C_FLAG_V), *flag_t = S.get<int32_t>(NM_C_FLAG_T);
    i64* sums = S.get<i64>(NM_C_SUMS);
    if (V) hipLaunchKernelGGL(nfl_mesh_keep_vertices_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, a->d_component, a->d_keep, V, C, flag_v);
    if (T) hipLaunchKernelGGL(nfl_mesh_keep_triangles_kernel, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, a->d_component, a->d_keep,
                              a->d_triangles, V, T, C, flag_t);
    nm_scan(flag_v, S.get<i64>(NM_C_OFF_V), V, sums, a->d_totals, s);
    nm_scan(flag_t, S.get<i64>(NM_C_OFF_T), T, sums, a->d_totals + 1, s);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_emit_vertices_kernel(const int32_t* flag, const i64* off, i64 V, i64 n_kept,
                                                                            const NgRows R) {
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

extern "C" int nfl_mesh_compact_emit(const nfl_mesh_compact_args* a, void* stream) {
    NmCompact S;
    const int rc = nm_carve(a, S);
    if (rc != NFL_OK) return rc;
    const i64 V = a->n_vertices, T = a->n_triangles, Vk = a->n_kept_vertices, Tk = a->n_kept_triangles;
    if (Vk < 0 || Tk < 0 || Vk > V || Tk > T) return NFL_EINVAL;
    if (Vk == 0 && Tk == 0) return NFL_OK;
    NgRows R = {{a->d_vertices, a->d_normals, a->d_colors}, {a->d_out_vertices, a->d_out_normals, a->d_out_colors}};
    for (int r = 0; r < 3; ++r)
        if (Vk && R.in[r] && !R.out[r]) return NFL_EINVAL;
    if (Tk && !a->d_out_triangles) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (Vk && (R.in[0] || R.in[1] || R.in[2]))
        hipLaunchKernelGGL(nfl_mesh_emit_vertices_kernel, dim3(nm_grid(V)), dim3(NM_THREADS), 0, s, S.get<int32_t>(NM_C_FLAG_V),
                           S.get<i64>(NM_C_OFF_V), V, Vk, R);
    if (Tk) hipLaunchKernelGGL(nfl_mesh_emit_triangles_kernel<i64>, dim3(nm_grid(T)), dim3(NM_THREADS), 0, s, S.get<int32_t>(NM_C_FLAG_T),
                               S.get<i64>(NM_C_OFF_T), a->d_triangles, S.get<i64>(NM_C_OFF_V), V, T, Vk, Tk, a->d_out_triangles);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
