// nfl_mesh_scan.hip -- the library's prefix sum over a device array (nm_scan) and its companion nm_rank; nfl_mesh.hip and
// nfl_simplify.hip run on them.  Tiles of NM_SCAN_TILE elements, a workgroup per tile, the tile sums scanned by the same
// kernel one level up until one tile is left (three levels cover 2^31 elements), then added back level by level: a fixed
// order, int32 in, int64 out, only integer adds, so every output is bit-reproducible.  Nothing here allocates, sets or
// copies memory through the runtime.
#include "nfl_geom.h"

// one tile: out[i] = sum of in[tile start .. i), sums[tile] = sum of the tile.  in == out is allowed (a thread reads its
// items before it writes them)
template <typename Tin>
__global__ __launch_bounds__(NM_SCAN_THREADS) void nfl_mesh_scan_tile_kernel(const Tin* in, i64* out, i64 n, i64* sums) {
    __shared__ i64 wave_sum[NM_SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    const i64 i0 = (i64)blockIdx.x * NM_SCAN_TILE + (i64)tid * NM_SCAN_ITEMS;
    i64 v[NM_SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int j = 0; j < NM_SCAN_ITEMS; ++j) {
        v[j] = i0 + j < n ? (i64)in[i0 + j] : 0;
        mine += v[j];
    }
    i64 all;
    i64 run = ng_block_scan<i64, NM_SCAN_THREADS>(mine, wave_sum, all);
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

void nm_scan(const int32_t* in, i64* out, i64 n, i64* sums, i64* total, hipStream_t s) {
    if (n == 0) {
        hipLaunchKernelGGL(nfl_mesh_zero_total_kernel, dim3(1), dim3(64), 0, s, total);
        return;
    }
    i64* buf[NM_SCAN_LEVELS + 1] = {out, nullptr, nullptr, nullptr};
    i64 len[NM_SCAN_LEVELS + 1] = {n, 0, 0, 0};
    int top = 0;
    for (;; ++top) {                                        // scan level `top`; its tile sums are level top + 1
        const i64 tiles = ng_cdiv(len[top], NM_SCAN_TILE);
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

// ids holds group representatives (or -1: in no group) on entry; a thread touches its own element only
__global__ __launch_bounds__(NM_THREADS) void nfl_mesh_rank_kernel(int32_t* ids, i64 n, const i64* rank) {
    const i64 v = (i64)blockIdx.x * NM_THREADS + threadIdx.x;
    if (v >= n) return;
    const int32_t r = ids[v];
    if (r >= 0) ids[v] = (int32_t)rank[r];
}

void nm_rank(int32_t* ids, i64 n, const i64* rank, hipStream_t s) {
    hipLaunchKernelGGL(nfl_mesh_rank_kernel, dim3(nm_grid(n)), dim3(NM_THREADS), 0, s, ids, n, rank);
}
