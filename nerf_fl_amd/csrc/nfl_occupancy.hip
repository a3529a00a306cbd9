// nfl_occupancy.hip -- empty-space skipping (include/nerf_fl_amd.h, "occupancy"): a one-bit-per-cell grid built from a
// regular fp32 lattice, and a kernel that walks rays through it and tightens their [near, far].  DESIGN.md section 20.
//
// Build.  Cell (i, j, k) at dilation d is occupied when an inside cell lies within Chebyshev distance d, and a cell is
// inside when one of its 8 corners is; cells outside the grid do not exist.  Both ORs together are ONE box-OR over the
// point flags: cell i sees the points max(i - d, 0) .. min(i + d, cx - 1) + 1 of its axis, i.e. the window
// [i - d, i + d + 1] cut to the lattice.  A box-OR is separable, so the build is four launches in bit space:
//   flags   a thread per lattice point; the wave's ballot is two words of point flags (bit x & 31 of word x >> 5)
//   x       a thread per output word: the window is d + 2 shifts of the word with carries from its two neighbours
//           (d + 1 <= 9 < 32, so one neighbour each side is enough); the bits past cx are cleared here
//   y, z    a thread per output word: whole words ORed over the window of rows, then of planes
// Each launch writes every word the next one reads; nothing is zeroed and nothing is accumulated into.
//
// Clip.  A thread per ray: slab test, entry cell, Amanatides-Woo walk with the plane parameters recomputed from integer
// plane indices.  The walk of a wave is as long as its longest ray (neighbouring pixels of a frame walk alike); the last
// fetched word stays in a register while the walk moves along x inside it.
#include <math.h>

#include "nfl_geom.h"

#define NO_TILE 256
#define NO_MAX_DILATE 8

// what the build kernels get
struct NoBuild {
    const float* lattice;
    int nx, ny, nz, d;
    int wpx, wx;            // words per row of points, of cells
    float threshold;
    uint32_t* P;            // (nz, ny, wpx) point flags; after the y pass (nz, cy, wx)
    uint32_t* X;            // (nz, ny, wx)
    uint32_t* bits;         // (cz, cy, wx)
};

__global__ __launch_bounds__(NO_TILE) void nfl_occ_flags_kernel(const NoBuild A) {
    const int x = blockIdx.x * NO_TILE + threadIdx.x;
    const size_t row = (size_t)blockIdx.z * A.ny + blockIdx.y;
    const bool inside = x < A.nx && A.lattice[row * A.nx + x] >= A.threshold;      // NaN compares false: outside
    const unsigned long long b = __ballot(inside);
    if ((threadIdx.x & 31) == 0) {
        const int w = x >> 5;
        if (w < A.wpx) A.P[row * A.wpx + w] = (threadIdx.x & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
    }
}

__global__ __launch_bounds__(NO_TILE) void nfl_occ_x_kernel(const NoBuild A) {
    const long long total = (long long)A.nz * A.ny * A.wx;
    const long long t = (long long)blockIdx.x * NO_TILE + threadIdx.x;
    if (t >= total) return;
    const long long row = t / A.wx;
    const int w = (int)(t - row * A.wx);
    const uint32_t* p = A.P + row * A.wpx;
    const uint64_t cur = p[w];
    const uint64_t up = (w + 1 < A.wpx ? (uint64_t)p[w + 1] << 32 : 0ull) | cur;       // bits w * 32 .. w * 32 + 63
    const uint64_t down = (cur << 32) | (w > 0 ? p[w - 1] : 0u);                         // bits w * 32 - 32 .. w * 32 + 31
    uint32_t out = 0;
    for (int s = 0; s <= A.d + 1; ++s) out |= (uint32_t)(up >> s);                       // points i .. i + d + 1
    for (int s = 1; s <= A.d; ++s) out |= (uint32_t)((down << s) >> 32);                 // points i - d .. i - 1
    const int cx = A.nx - 1;
    if (w == A.wx - 1 && (cx & 31)) out &= (1u << (cx & 31)) - 1u;
    A.X[t] = out;
}

// out (n_outer, n_out, wx): word (o, j, w) = OR of in (o, max(j - d, 0) .. min(j + d + 1, n_in - 1), w); n_out = n_in - 1.
// The y pass runs it with outer = planes and inner = wx, the z pass with outer = 1 and inner = cy * wx.
__global__ __launch_bounds__(NO_TILE) void nfl_occ_or_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                              long long n_outer, int n_in, long long inner, int d) {
    const int n_out = n_in - 1;
    const long long total = n_outer * n_out * inner;
    const long long t = (long long)blockIdx.x * NO_TILE + threadIdx.x;
    if (t >= total) return;
    const long long o = t / (n_out * inner), r = t - o * (n_out * inner);
    const int j = (int)(r / inner);
    const long long w = r - (long long)j * inner;
    const int a = j - d > 0 ? j - d : 0, b = j + d + 1 < n_in - 1 ? j + d + 1 : n_in - 1;
    const uint32_t* src = in + (o * n_in) * inner + w;
    uint32_t v = 0;
    for (int y = a; y <= b; ++y) v |= src[(long long)y * inner];
    out[t] = v;
}

extern "C" size_t nfl_occ_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (!ng_dims_ok(nx, ny, nz)) return 0;
    return (size_t)(nz - 1) * (ny - 1) * no_words(nx - 1) * 4;
}

extern "C" size_t nfl_occ_build_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t dilate) {
    if (!ng_dims_ok(nx, ny, nz) || dilate < 0 || dilate > NO_MAX_DILATE) return 0;
    return ng_bytes(no_layout(nx, ny, nz));
}

extern "C" int nfl_occ_build(const nfl_occ_build_args* a, void* stream) {
    if (!a || !a->d_lattice || !a->d_scratch || !a->d_bits) return NFL_EINVAL;
    if (!ng_dims_ok(a->nx, a->ny, a->nz) || a->dilate < 0 || a->dilate > NO_MAX_DILATE) return NFL_EINVAL;
    if (ng_misaligned(a->d_lattice, 4) || ng_misaligned(a->d_bits, 4)) return NFL_EINVAL;
    auto L = no_layout(a->nx, a->ny, a->nz);
    const int rc = ng_carve(L, a->d_scratch, a->scratch_bytes);
    if (rc != NFL_OK) return rc;
    NoBuild A;
    A.lattice = a->d_lattice;
    A.nx = a->nx, A.ny = a->ny, A.nz = a->nz, A.d = a->dilate;
    A.wpx = no_words(a->nx), A.wx = no_words(a->nx - 1);
    A.threshold = a->threshold;
    A.P = L.get<uint32_t>(NO_P);
    A.X = L.get<uint32_t>(NO_X);
    A.bits = a->d_bits;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cy = a->ny - 1, cz = a->nz - 1;
    auto blocks = [](long long n) { return dim3((unsigned)((n + NO_TILE - 1) / NO_TILE)); };
    hipLaunchKernelGGL(nfl_occ_flags_kernel, dim3((a->nx + NO_TILE - 1) / NO_TILE, a->ny, a->nz), dim3(NO_TILE), 0, s, A);
    hipLaunchKernelGGL(nfl_occ_x_kernel, blocks((long long)a->nz * a->ny * A.wx), dim3(NO_TILE), 0, s, A);
    // y: X (nz, ny, wx) -> P reused as (nz, cy, wx), which is no larger than the point flags it held
    hipLaunchKernelGGL(nfl_occ_or_kernel, blocks((long long)a->nz * cy * A.wx), dim3(NO_TILE), 0, s,
                       (const uint32_t*)A.X, A.P, (long long)a->nz, a->ny, (long long)A.wx, A.d);
    // z: (nz, cy * wx) -> bits (cz, cy * wx)
    hipLaunchKernelGGL(nfl_occ_or_kernel, blocks((long long)cz * cy * A.wx), dim3(NO_TILE), 0, s,
                       (const uint32_t*)A.P, A.bits, 1ll, a->nz, (long long)cy * A.wx, A.d);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}

// ---- clip ----------------------------------------------------------------------------------------------------------------

// parameter of plane b of an axis: the plane position is rebuilt from the integer index every time (no accumulation)
__device__ __forceinline__ float no_plane_t(float lo, float sp, int b, float o, float inv) {
    return ((lo + (float)b * sp) - o) * inv;
}

__global__ __launch_bounds__(NO_TILE) void nfl_occ_clip_kernel(const nfl_occ_clip_args a) {
    const long long r = (long long)blockIdx.x * NO_TILE + threadIdx.x;
    if (r >= a.n_rays) return;
    const float4 q0 = reinterpret_cast<const float4*>(a.d_rays)[2 * r];
    const float4 q1 = reinterpret_cast<const float4*>(a.d_rays)[2 * r + 1];
    const float ox = q0.x, oy = q0.y, oz = q0.z, dx = q0.w, dy = q1.x, dz = q1.y, near = q1.z, far = q1.w;
    const int cx = a.nx - 1, cy = a.ny - 1, cz = a.nz - 1;
    const int wx = (cx + 31) >> 5;
    const float lox = a.lo[0], loy = a.lo[1], loz = a.lo[2], sx = a.spacing[0], sy = a.spacing[1], sz = a.spacing[2];
    const float INF = __builtin_huge_valf();

    // a NaN anywhere: a miss (fminf / fmaxf below would drop it silently)
    bool miss = !(ox == ox && oy == oy && oz == oz && dx == dx && dy == dy && dz == dz && near == near && far == far);
    float t0 = near, t1 = far, ix = 0.f, iy = 0.f, iz = 0.f;
#define NO_SLAB(o, d, inv, lo, sp, c)                                                   \
    {                                                                                   \
        const float hi = lo + (float)(c) * sp;                                          \
        if (d != 0.f) {                                                                 \
            inv = 1.f / d;                                                              \
            const float ta = (lo - o) * inv, tb = (hi - o) * inv;                       \
            t0 = fmaxf(t0, fminf(ta, tb));                                              \
            t1 = fminf(t1, fmaxf(ta, tb));                                              \
        } else if (!(o >= lo && o <= hi)) miss = true;                                  \
    }
    NO_SLAB(ox, dx, ix, lox, sx, cx)
    NO_SLAB(oy, dy, iy, loy, sy, cy)
    NO_SLAB(oz, dz, iz, loz, sz, cz)
#undef NO_SLAB
    float out_near = near, out_far = far;
    uint8_t hit = 0;
    if (!miss && t0 < t1) {
        // entry cell: floor((o + t0 d - lo) / spacing), clamped in fp32 (a NaN or an infinity lands inside the grid too)
        int i = (int)fminf(fmaxf(floorf(((ox + t0 * dx) - lox) / sx), 0.f), (float)(cx - 1));
        int j = (int)fminf(fmaxf(floorf(((oy + t0 * dy) - loy) / sy), 0.f), (float)(cy - 1));
        int k = (int)fminf(fmaxf(floorf(((oz + t0 * dz) - loz) / sz), 0.f), (float)(cz - 1));
        const int stx = dx > 0.f ? 1 : -1, sty = dy > 0.f ? 1 : -1, stz = dz > 0.f ? 1 : -1;
        int bx = i + (dx > 0.f ? 1 : 0), by = j + (dy > 0.f ? 1 : 0), bz = k + (dz > 0.f ? 1 : 0);
        float tx = dx != 0.f ? no_plane_t(lox, sx, bx, ox, ix) : INF;
        float ty = dy != 0.f ? no_plane_t(loy, sy, by, oy, iy) : INF;
        float tz = dz != 0.f ? no_plane_t(loz, sz, bz, oz, iz) : INF;
        float t_in = t0, t_first = 0.f, t_last = 0.f;
        bool found = false;
        long long have = -1;
        uint32_t word = 0;
        const int max_cells = cx + cy + cz + 1;
        for (int n = 0; n < max_cells; ++n) {
            const long long wi = ((long long)k * cy + j) * wx + (i >> 5);
            if (wi != have) { word = a.d_bits[wi]; have = wi; }
            int axis = 0;
            float t_out = tx;
            if (ty < t_out) { axis = 1; t_out = ty; }
            if (tz < t_out) { axis = 2; t_out = tz; }
            if ((word >> (i & 31)) & 1u) {
                if (!found) { t_first = t_in; found = true; }
                t_last = fminf(t_out, t1);
            }
            if (!(t_out < t1)) break;
            if (axis == 0) {
                i += stx; bx += stx;
                if (i < 0 || i >= cx) break;
                tx = no_plane_t(lox, sx, bx, ox, ix);
            } else if (axis == 1) {
                j += sty; by += sty;
                if (j < 0 || j >= cy) break;
                ty = no_plane_t(loy, sy, by, oy, iy);
            } else {
                k += stz; bz += stz;
                if (k < 0 || k >= cz) break;
                tz = no_plane_t(loz, sz, bz, oz, iz);
            }
            t_in = t_out;
        }
        if (found && t_last > t_first) { hit = 1; out_near = t_first; out_far = t_last; }
    }
    reinterpret_cast<float2*>(a.d_near_far)[r] = make_float2(out_near, out_far);
    a.d_hit[r] = hit;
}

extern "C" int nfl_occ_clip_rays(const nfl_occ_clip_args* a, void* stream) {
    if (!a || a->n_rays < 0 || a->n_rays > INT32_MAX) return NFL_EINVAL;
    if (!ng_dims_ok(a->nx, a->ny, a->nz)) return NFL_EINVAL;
    for (int k = 0; k < 3; ++k)
        if (!(a->spacing[k] > 0.f) || !(a->spacing[k] < __builtin_huge_valf()) || !ng_finite(a->lo[k])) return NFL_EINVAL;
    if (a->n_rays == 0) return NFL_OK;
    if (ng_bad(a->d_rays, 16) || ng_bad(a->d_bits, 4) || ng_bad(a->d_near_far, 8) || !a->d_hit) return NFL_EINVAL;
    const unsigned blocks = (unsigned)((a->n_rays + NO_TILE - 1) / NO_TILE);
    hipLaunchKernelGGL(nfl_occ_clip_kernel, dim3(blocks), dim3(NO_TILE), 0, static_cast<hipStream_t>(stream), *a);
    return ng_launched() ? NFL_OK : NFL_ELAUNCH;
}
