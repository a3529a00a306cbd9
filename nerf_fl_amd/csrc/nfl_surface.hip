// nfl_surface.hip -- the iso-surface of a regular fp32 lattice as an indexed triangle mesh (include/nerf_fl_amd.h,
// "surface"): marching tetrahedra, welded, bit-reproducible, no atomics.  DESIGN.md section 18.
//
// Split.  A corner of a cell is the bit mask c = dx | dy << 1 | dz << 2.  Every cell is cut into the six Kuhn tetrahedra
// (0, a, a | b, 7), (a, b, c) running over the permutations of the axis bits in lexicographic order; all six share the
// body diagonal 0-7, and the cut of a cell face is the same seen from either cell, so the surface is closed across cells
// without a case analysis.  Every edge of a tetrahedron joins corners lo and hi with lo a subset of hi: it points towards
// +, belongs to the LATTICE POINT at corner lo and has one of seven types m = hi ^ lo (three axis edges, three face
// diagonals, the body diagonal).  A crossing edge (one end >= iso, the other not; NaN is not) carries exactly one vertex,
// whichever of the up to six tetrahedra around it asks: that is the weld.
//
// One workgroup owns a slab of NS_TILE points of one x-row and stages the 2 x 2 x (NS_TILE + 1) values around it in LDS
// once; a thread owns one lattice point (its seven edges) and the cell whose corner 0 that point is (its six tetrahedra).
//   count   per thread: the 7-bit mask of crossing edges and the number of triangles; a workgroup scan turns them into
//           offsets inside the slab.  One uint32 per point goes to the scratch (mask << 16 | vertex offset in the slab),
//           one (vertices, triangles) pair per slab.
//   scan    one workgroup turns the slab pairs into exclusive int64 prefix sums in place and writes the two totals.
//   emit    stages the same values plus the point records of the four rows; a vertex id is
//           slab offset + offset in the slab + rank of the edge type in the owner's mask,
//           for the thread's own edges and for the edges its tetrahedra borrow from the seven neighbouring points alike.
// Vertices come out ordered by (owner point, edge type), triangles by (cell, tetrahedron, place in the table).  Every
// result is written by a plain vector store; nothing is zeroed (every scratch element that is read was written first).
#include <math.h>

#include "nfl_geom.h"

#define NS_SCAN_THREADS 1024
#define NS_SCAN_ITEMS 4

// corners (0, a, a | b, 7) of the six tetrahedra
__constant__ uint8_t NS_TET[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// [tetrahedron][case: bit j = corner j inside][2 triangles x 3 edges], an edge as lo << 3 | m; the winding makes the
// triangle normal point from inside to outside.  Printed by tests/geometry_ref.py, which builds it from geometry.
__constant__ uint8_t NS_TRI[6][16][6] = {
    {{ 0, 0, 0, 0, 0, 0}, { 1, 3, 7, 0, 0, 0}, { 1,14,10, 0, 0, 0}, { 3, 7,14, 3,14,10}, { 3,10,28, 0, 0, 0}, { 1,28, 7, 1,10,28}, { 1,14,28, 1,28, 3}, { 7,14,28, 0, 0, 0},
     { 7,28,14, 0, 0, 0}, { 1, 3,28, 1,28,14}, { 1,28,10, 1, 7,28}, { 3,28,10, 0, 0, 0}, { 3,10,14, 3,14, 7}, { 1,10,14, 0, 0, 0}, { 1, 7, 3, 0, 0, 0}, { 0, 0, 0, 0, 0, 0}},
    {{ 0, 0, 0, 0, 0, 0}, { 1, 7, 5, 0, 0, 0}, { 1,12,14, 0, 0, 0}, { 5,14, 7, 5,12,14}, { 5,42,12, 0, 0, 0}, { 1, 7,42, 1,42,12}, { 1,42,14, 1, 5,42}, { 7,42,14, 0, 0, 0},
     { 7,14,42, 0, 0, 0}, { 1,42, 5, 1,14,42}, { 1,12,42, 1,42, 7}, { 5,12,42, 0, 0, 0}, { 5,14,12, 5, 7,14}, { 1,14,12, 0, 0, 0}, { 1, 5, 7, 0, 0, 0}, { 0, 0, 0, 0, 0, 0}},
    {{ 0, 0, 0, 0, 0, 0}, { 2, 7, 3, 0, 0, 0}, { 2,17,21, 0, 0, 0}, { 3,21, 7, 3,17,21}, { 3,28,17, 0, 0, 0}, { 2, 7,28, 2,28,17}, { 2,28,21, 2, 3,28}, { 7,28,21, 0, 0, 0},
     { 7,21,28, 0, 0, 0}, { 2,28, 3, 2,21,28}, { 2,17,28, 2,28, 7}, { 3,17,28, 0, 0, 0}, { 3,21,17, 3, 7,21}, { 2,21,17, 0, 0, 0}, { 2, 3, 7, 0, 0, 0}, { 0, 0, 0, 0, 0, 0}},
    {{ 0, 0, 0, 0, 0, 0}, { 2, 6, 7, 0, 0, 0}, { 2,21,20, 0, 0, 0}, { 6, 7,21, 6,21,20}, { 6,20,49, 0, 0, 0}, { 2,49, 7, 2,20,49}, { 2,21,49, 2,49, 6}, { 7,21,49, 0, 0, 0},
     { 7,49,21, 0, 0, 0}, { 2, 6,49, 2,49,21}, { 2,49,20, 2, 7,49}, { 6,49,20, 0, 0, 0}, { 6,20,21, 6,21, 7}, { 2,20,21, 0, 0, 0}, { 2, 7, 6, 0, 0, 0}, { 0, 0, 0, 0, 0, 0}},
    {{ 0, 0, 0, 0, 0, 0}, { 4, 5, 7, 0, 0, 0}, { 4,35,33, 0, 0, 0}, { 5, 7,35, 5,35,33}, { 5,33,42, 0, 0, 0}, { 4,42, 7, 4,33,42}, { 4,35,42, 4,42, 5}, { 7,35,42, 0, 0, 0},
     { 7,42,35, 0, 0, 0}, { 4, 5,42, 4,42,35}, { 4,42,33, 4, 7,42}, { 5,42,33, 0, 0, 0}, { 5,33,35, 5,35, 7}, { 4,33,35, 0, 0, 0}, { 4, 7, 5, 0, 0, 0}, { 0, 0, 0, 0, 0, 0}},
    {{ 0, 0, 0, 0, 0, 0}, { 4, 7, 6, 0, 0, 0}, { 4,34,35, 0, 0, 0}, { 6,35, 7, 6,34,35}, { 6,49,34, 0, 0, 0}, { 4, 7,49, 4,49,34}, { 4,49,35, 4, 6,49}, { 7,49,35, 0, 0, 0},
     { 7,35,49, 0, 0, 0}, { 4,49, 6, 4,35,49}, { 4,34,49, 4,49, 7}, { 6,34,49, 0, 0, 0}, { 6,35,34, 6, 7,35}, { 4,35,34, 0, 0, 0}, { 4, 6, 7, 0, 0, 0}, { 0, 0, 0, 0, 0, 0}}};

// (vertices, triangles) of a slab, as they lie in NsArgs::sums: what the scan kernel sums
struct NsPair { long long v, t; };
__device__ __forceinline__ NsPair operator+(NsPair a, NsPair b) { return {a.v + b.v, a.t + b.t}; }
__device__ __forceinline__ NsPair operator-(NsPair a, NsPair b) { return {a.v - b.v, a.t - b.t}; }
__device__ __forceinline__ NsPair ng_shfl_up(NsPair p, int off) { return {__shfl_up(p.v, off), __shfl_up(p.t, off)}; }

// what the kernels get: the caller's arguments and the scratch (ns_layout of nfl_geom_layout.h), carved up
struct NsArgs {
    nfl_surface_args a;
    uint32_t* rec;          // (points) mask << 16 | vertex offset inside the slab
    long long* sums;        // (slabs, 2) vertices, triangles per slab; after the scan their exclusive prefix sums
    int ntx;                // slabs per x-row
    long long n_slabs;
};

// the 2 x 2 rows (y + dy, z + dz), row r = dy + 2 dz, of NS_TILE + 1 values from x0 on; 0 where the lattice ends
__device__ __forceinline__ void ns_stage(const NsArgs& A, int x0, int y, int z, float (*val)[NS_TILE + 1]) {
    const int nx = A.a.nx, ny = A.a.ny, nz = A.a.nz;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = y + (r & 1), zz = z + (r >> 1);
        const bool row_ok = yy < ny && zz < nz;
        const float* row = A.a.d_lattice + ((size_t)zz * ny + yy) * nx;
        for (int i = threadIdx.x; i < NS_TILE + 1; i += NS_TILE) val[r][i] = (row_ok && x0 + i < nx) ? row[x0 + i] : 0.f;
    }
}

// the thread's point (x, y, z): inside bits of the 8 corners of its cell, mask of its crossing edges, triangles of its cell
__device__ __forceinline__ void ns_classify(const NsArgs& A, int x, int y, int z, const float (*val)[NS_TILE + 1],
                                            uint32_t& corners, uint32_t& edges, uint32_t& n_tri) {
    corners = edges = n_tri = 0;
    if (x >= A.a.nx) return;
    const int i = threadIdx.x;
    const float iso = A.a.iso;
#pragma unroll
    for (int c = 0; c < 8; ++c) corners |= (val[c >> 1][i + (c & 1)] >= iso ? 1u : 0u) << c;
    // axes along which the lattice goes on: an edge or a cell needs all of its own
    const uint32_t axes = (x + 1 < A.a.nx ? 1u : 0u) | (y + 1 < A.a.ny ? 2u : 0u) | (z + 1 < A.a.nz ? 4u : 0u);
#pragma unroll
    for (uint32_t m = 1; m < 8; ++m)
        if ((m & ~axes) == 0 && (((corners >> m) ^ corners) & 1u)) edges |= 1u << (m - 1);
    if (axes == 7u) {
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const uint32_t k = (corners & 1u) + ((corners >> NS_TET[t][1]) & 1u) + ((corners >> NS_TET[t][2]) & 1u) + (corners >> 7);
            n_tri += k == 2 ? 2u : (k & 1u);
        }
    }
}

__global__ __launch_bounds__(NS_TILE) void nfl_surface_count_kernel(const NsArgs A) {
    __shared__ float val[4][NS_TILE + 1];
    __shared__ uint32_t wave_sum[NS_TILE / 64];
    const int x0 = blockIdx.x * NS_TILE, y = blockIdx.y, z = blockIdx.z, x = x0 + threadIdx.x;
    ns_stage(A, x0, y, z, val);
    __syncthreads();
    uint32_t corners, edges, n_tri, total;
    ns_classify(A, x, y, z, val, corners, edges, n_tri);
    // vertices in the low half, triangles in the high half: at most 7 * 256 and 12 * 256 per slab
    const uint32_t excl = ng_block_scan<uint32_t, NS_TILE>((n_tri << 16) | __popc(edges), wave_sum, total);
    if (x < A.a.nx) A.rec[((size_t)z * A.a.ny + y) * A.a.nx + x] = (edges << 16) | (excl & 0xFFFFu);
    if (threadIdx.x == 0) {
        long long* s = A.sums + 2 * (((size_t)z * A.a.ny + y) * A.ntx + blockIdx.x);
        s[0] = total & 0xFFFFu;
        s[1] = total >> 16;
    }
}

// one workgroup: sums (n, 2) -> exclusive prefix sums in place, the two totals to d_totals
__global__ __launch_bounds__(NS_SCAN_THREADS) void nfl_surface_scan_kernel(const NsArgs A) {
    __shared__ NsPair wave_sum[NS_SCAN_THREADS / 64];
    NsPair* sums = reinterpret_cast<NsPair*>(A.sums);
    const int tid = threadIdx.x;
    NsPair carry = {0, 0};
    for (long long base = 0; base < A.n_slabs; base += NS_SCAN_THREADS * NS_SCAN_ITEMS) {
        const long long i0 = base + (long long)tid * NS_SCAN_ITEMS;
        NsPair v[NS_SCAN_ITEMS], mine = {0, 0}, all;
#pragma unroll
        for (int j = 0; j < NS_SCAN_ITEMS; ++j) {
            v[j] = i0 + j < A.n_slabs ? sums[i0 + j] : NsPair{0, 0};
            mine = mine + v[j];
        }
        __syncthreads();                                    // the previous round's wave_sum has been read
        NsPair run = carry + ng_block_scan<NsPair, NS_SCAN_THREADS>(mine, wave_sum, all);
#pragma unroll
        for (int j = 0; j < NS_SCAN_ITEMS; ++j) {
            if (i0 + j < A.n_slabs) sums[i0 + j] = run;
            run = run + v[j];
        }
        carry = carry + all;
    }
    if (tid == 0) {
        A.a.d_totals[0] = carry.v;
        A.a.d_totals[1] = carry.t;
    }
}

// -grad of the lattice at point (x, y, z): central differences, one-sided at the border
__device__ __forceinline__ void ns_gradient(const nfl_surface_args& a, int x, int y, int z, float g[3]) {
    const int n[3] = {a.nx, a.ny, a.nz}, p[3] = {x, y, z};
    const size_t stride[3] = {1, (size_t)a.nx, (size_t)a.nx * a.ny};
    const float* c = a.d_lattice + ((size_t)z * a.ny + y) * a.nx + x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float s = a.spacing[k];
        if (p[k] == 0) g[k] = (c[stride[k]] - c[0]) / s;
        else if (p[k] == n[k] - 1) g[k] = (c[0] - *(c - stride[k])) / s;
        else g[k] = (c[stride[k]] - *(c - stride[k])) / (2.f * s);
    }
}

__global__ __launch_bounds__(NS_TILE) void nfl_surface_emit_kernel(const NsArgs A) {
    __shared__ float val[4][NS_TILE + 1];
    __shared__ uint32_t rec[4][NS_TILE + 1];
    __shared__ long long slab_v[4][2];       // vertex offset of the slab of row r, and of the next slab of that row
    __shared__ uint32_t wave_sum[NS_TILE / 64];
    const nfl_surface_args& a = A.a;
    const int tid = threadIdx.x, x0 = blockIdx.x * NS_TILE, y = blockIdx.y, z = blockIdx.z, x = x0 + tid;
    ns_stage(A, x0, y, z, val);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int yy = y + (r & 1), zz = z + (r >> 1);
        const bool row_ok = yy < a.ny && zz < a.nz;
        const size_t row = (size_t)zz * a.ny + yy;
        for (int i = tid; i < NS_TILE + 1; i += NS_TILE) rec[r][i] = (row_ok && x0 + i < a.nx) ? A.rec[row * a.nx + x0 + i] : 0u;
        if (tid < 2) slab_v[r][tid] = (row_ok && (int)blockIdx.x + tid < A.ntx) ? A.sums[2 * (row * A.ntx + blockIdx.x + tid)] : 0;
    }
    __syncthreads();
    uint32_t corners, edges, n_tri, total;
    ns_classify(A, x, y, z, val, corners, edges, n_tri);
    const uint32_t tri_excl = ng_block_scan<uint32_t, NS_TILE>(n_tri, wave_sum, total);

    // ---- the vertices of this point's crossing edges
    if (edges) {
        long long v = slab_v[0][0] + (rec[0][tid] & 0xFFFFu);
        const float va = val[0][tid];
        const int pa[3] = {x, y, z};
        float ga[3];
        ns_gradient(a, x, y, z, ga);
        for (uint32_t m = 1; m < 8; ++m) {
            if (!((edges >> (m - 1)) & 1u)) continue;
            const int d[3] = {(int)(m & 1u), (int)((m >> 1) & 1u), (int)(m >> 2)};
            const float vb = val[m >> 1][tid + d[0]];
            float t = (a.iso - va) / (vb - va);
            t = fminf(fmaxf(t, 0.f), 1.f);                  // a NaN (an infinite or NaN end) becomes 0: the owner's end
            float gb[3], nrm[3];
            ns_gradient(a, x + d[0], y + d[1], z + d[2], gb);
            if (v < a.n_vertices) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float qa = a.lo[k] + (float)pa[k] * a.spacing[k];
                    const float qb = a.lo[k] + (float)(pa[k] + d[k]) * a.spacing[k];
                    a.d_vertices[3 * v + k] = qa + t * (qb - qa);
                    nrm[k] = -(ga[k] + t * (gb[k] - ga[k]));
                }
                const float len = sqrtf((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) a.d_normals[3 * v + k] = len > 0.f ? nrm[k] / len : 0.f;
            }
            ++v;
        }
    }

    // ---- the triangles of this point's cell
    if (n_tri) {
        long long tri = A.sums[2 * (((size_t)z * a.ny + y) * A.ntx + blockIdx.x) + 1] + tri_excl;
        for (int t = 0; t < 6; ++t) {
            uint32_t k = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) k |= ((corners >> NS_TET[t][j]) & 1u) << j;
            const int n = __popc(k) == 2 ? 2 : (__popc(k) & 1);
            for (int j = 0; j < n; ++j, ++tri) {
                if (tri >= a.n_triangles) continue;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const uint32_t code = NS_TRI[t][k][3 * j + e], lo = code >> 3, m = code & 7u;
                    const int i = tid + (lo & 1u);
                    const uint32_t r = rec[lo >> 1][i];
                    const long long id = slab_v[lo >> 1][i >= NS_TILE ? 1 : 0] + (r & 0xFFFFu) + __popc((r >> 16) & ((1u << (m - 1)) - 1u));
                    a.d_triangles[3 * tri + e] = (int32_t)id;
                }
            }
        }
    }
}

static int ns_carve(const nfl_surface_args* a, NsArgs& A) {
    if (!a || !a->d_lattice || !a->d_scratch) return NFL_EINVAL;
    if (!ng_dims_ok(a->nx, a->ny, a->nz)) return NFL_EINVAL;
    auto L = ns_layout(a->nx, a->ny, a->nz);
    const int rc = ng_carve(L, a->d_scratch, a->scratch_bytes, true);
    if (rc != NFL_OK) return rc;
    A.a = *a;
    A.ntx = ns_ntx(a->nx);
    A.n_slabs = (long long)A.ntx * a->ny * a->nz;
    A.rec = L.get<uint32_t>(NS_REC);
    A.sums = L.get<long long>(NS_SUMS);
    return NFL_OK;
}

extern "C" size_t nfl_surface_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!ng_dims_ok(nx, ny, nz)) return 0;
    return ng_bytes(ns_layout(nx, ny, nz));
}

extern "C" int nfl_surface_count(const nfl_surface_args* args, void* stream) {
    NsArgs A;
    const int rc = ns_carve(args, A);
    if (rc != NFL_OK) return rc;
    if (!args->d_totals) return NFL_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nfl_surface_count_kernel, dim3(A.ntx, args->ny, args->nz), dim3(NS_TILE), 0, s, A);
    hipLaunchKernelGGL(nfl_surface_scan_kernel, dim3(1), dim3(NS_SCAN_THREADS), 0, s, A);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

extern "C" int nfl_surface_emit(const nfl_surface_args* args, void* stream) {
    NsArgs A;
    const int rc = ns_carve(args, A);
    if (rc != NFL_OK) return rc;
    if (args->n_vertices < 0 || args->n_triangles < 0) return NFL_EINVAL;
    if (args->n_vertices > INT32_MAX || args->n_triangles > INT32_MAX / 3) return NFL_EINVAL;     // indices are int32
    if (args->n_vertices == 0 && args->n_triangles == 0) return NFL_OK;
    if (!args->d_vertices || !args->d_normals || (args->n_triangles && !args->d_triangles)) return NFL_EINVAL;
    hipLaunchKernelGGL(nfl_surface_emit_kernel, dim3(A.ntx, args->ny, args->nz), dim3(NS_TILE), 0,
                       static_cast<hipStream_t>(stream), A);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
