// nfl_wgrad.hip -- weight / bias gradients of the field MLP as streaming fp16 GEMMs.
//
//   dW_l[out, in] = sum over samples  delta_l[sample, out] * h_{l-1}[sample, in]
//   db_l[out]     = sum over samples  delta_l[sample, out]
// (what autograd's Linear backward does per point chunk in the reference, models/nerf.py
// 153-212).  Both operands come from the stashes the forward / dgrad kernels wrote: per
// 32-sample segment, per layer, MFMA-fragment-ordered fp16 with the SAMPLE on the lane (the
// gradients carry the pass' power-of-two loss scale, divided out by the reduction).
// The contraction index here is the sample, so both operands have to be presented with
// the FEATURE on the lane and 8 consecutive samples in registers: the 1 KiB k-step images
// are DMA'd verbatim into LDS and read back with ds_read_b64_tr_b16 (hardware 4x16
// transpose), two reads per MFMA operand, no extra pass over the data.
//
// Composed through xyz_encoding_final.  That layer is linear (feat = W_fin h8 + b_fin, no activation), and its
// output is read by the direction layer and the first transient layer only, so
//     delta_feat = Wd^T delta_dirh (+ Wt^T delta_g1)        Wd = W_dir[:, :256], Wt = W_t0[:, :256]
// and with G = sum_s delta_dirh (x) h8  (128 x 256; Gt the same from delta_g1):
//     dW_fin        = Wd^T G (+ Wt^T Gt)            db_fin = Wd^T db_dir (+ Wt^T db_t0)
//     dW_dir[:, :256] = G W_fin^T + db_dir (x) b_fin    (dW_t0[:, :256] likewise from Gt)
// Neither `feat` nor `delta_feat` is ever stashed (16 KiB per 32-sample segment less written by the forward, 16 less
// by dgrad, 24 less read here); the stream accumulates G | Gt into a 256 x 256 scratch like any other job and
// nfl_wgrad_compose_kernel (nfl_compose.hip; the task list: nfl_compose.cpp) finishes the four products in fp32 (34-67 MFLOP, one launch).
//
// Roofline: HBM.  A 256x256 layer reads 32 KiB per segment for 2 x 64 MFMAs, 128 FLOP/B,
// far under the MFMA ridge, so the kernel is a stream (wg_body_rs below), with fp32 accumulators
// for the whole (<=256 x <=352) tile of dW in registers.  Every workgroup stores its accumulators once, as they are, and
// nfl_wgrad_reduce_kernel adds the parts up in a fixed order and divides the loss scale out: no atomics.
//
// The job list of a field, the launch schedule of a call, the entry point's checks and the table of instantiations are host
// code: nfl_wgrad_plan.h / .cpp.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_compose.h"
#include "nfl_dev.h"
#include "nfl_diag.h"
#include "nfl_wgrad_plan.h"

typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float wg_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int wg_orig(int kind, int i) {
    return kind == NFL_SEG_ACT ? 16 * (i >> 4) + 8 * ((i & 7) >> 2) + 4 * ((i >> 3) & 1) + (i & 3) : i;
}

// feature-on-lane MFMA operand of MFMA k-step m (samples 16m..16m+15) from a tile image (2 k-step pieces)
__device__ __forceinline__ h8 wg_operand(const char* tile, int lane, int m) {
    // stash k-step image: [sample c][lane half h][8 values] = 32 B per sample.  A 16-lane group reads 4
    // samples x 16 features = 128 contiguous bytes; the two groups of a 32-lane half take the two k-steps of
    // the tile (pieces WG_PSTRIDE apart, 32 B off the 1 KiB grid): every read is bank-conflict free.
    const int g = lane >> 4, ip = lane & 15, q = ip >> 2, p = ip & 3;
    const int c = 16 * m + 8 * (g >> 1) + q;
    const char* ad = tile + (g & 1) * WG_PSTRIDE + c * 32 + p * 8;
    typedef __fp16 hf4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    const h4 lo = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hf4*)(ad)));
    const h4 hi = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hf4*)(ad + 4 * 32)));
    h8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
}

template <int NITW>
__device__ __forceinline__ void wg_flush(const WgArgs& A, const int j, const int part, f16v (&acc)[WG_NOT][NITW], float (&bsum)[WG_NOT],
                                         const int wave, const int lane) {
    // flush: every workgroup stores its accumulators (still carrying the loss scale) as they are, 64 B per lane and tile; the
    // reduction kernel below knows which gradient element each of them is.  (Until round 3 this was 64 MB of fp32 atomics into
    // the gradient tensors at the end of the launch, 55 us during which the HBM idled, a zeroing and an unscaling launch around
    // it -- and a summation order that changed from run to run.)
    float* P = A.partial + (size_t)A.part_off[j] + (size_t)part * A.part_len[j];
#pragma unroll
    for (int a = 0; a < WG_NOT; ++a) {
#pragma unroll
        for (int b = 0; b < NITW; ++b) {
            // [tile][q][lane][4]: a store instruction (and a wave of the reduction) covers 1 KiB of contiguous memory
            float* dst = P + (size_t)((wave * WG_NOT + a) * NITW + b) * 1024 + lane * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<wg_f4*>(dst + q * 256) = wg_f4{acc[a][b][4 * q], acc[a][b][4 * q + 1], acc[a][b][4 * q + 2], acc[a][b][4 * q + 3]};
        }
        P[(size_t)4 * WG_NOT * NITW * 1024 + (wave * WG_NOT + a) * 64 + lane] = bsum[a];
    }
}

// One block per (job, wave, a, b) accumulator tile: sums the job's parts in order, unscales, and writes the elements the tile
// owns -- each gradient element is owned by exactly one tile of one job, so these are plain stores into tensors nobody zeroed.
__global__ __launch_bounds__(256) void nfl_wgrad_reduce_kernel(const WgArgs A, const float* gmax) {
    const WgPlan& P = *A.plan;
    int j = 0;
    while (j + 1 < P.n_jobs && (int)blockIdx.x >= A.red_start[j + 1]) ++j;
    const WgJob& J = P.job[j];
    const int nitw = A.part_nitw[j], t = blockIdx.x - A.red_start[j];
    const int b = t % nitw, wa = t / nitw, a = wa % WG_NOT, wave = wa / WG_NOT;
    const int wo = wave % J.n_wo, wi = wave / J.n_wo;
    const int lane = threadIdx.x & 63, rq = threadIdx.x >> 6;
    const int nparts = A.wg_start[j + 1] - A.wg_start[j];
    const int live = A.n_seg < nparts ? A.n_seg : nparts;        // workgroups beyond the segment count returned before their flush
    float inv;
    {   // nfl_gmax_bits and its nfl_wave_max (nfl_dev.h) written out: through the helpers the compiler schedules this kernel differently
        unsigned v = 0u;
        for (int i = lane; i < NFL_GMAX_SLOTS; i += 64) {
            const unsigned o = reinterpret_cast<const unsigned*>(gmax)[i];
            v = o > v ? o : v;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned o = __shfl_xor(v, d);
            v = o > v ? o : v;
        }
        inv = 1.0f / nfl_loss_scale_from_bits(__builtin_amdgcn_readfirstlane(v));
    }
    const int ot = wo * WG_NOT + a;
    if (ot >= J.n_ot) return;
    const WgTile TO = J.ot[ot];
    const int layer = J.bias_layer_of_ot[ot] >= 0 ? J.bias_layer_of_ot[ot] : J.layer;
    const float* base = A.partial + (size_t)A.part_off[j];
    const int n = lane & 31, hh = lane >> 5;
    float* W = layer == WG_SCRATCH ? A.scratch : A.g.weight[layer];
    if (wi + b * J.n_wi < J.n_it && W != nullptr) {
        const WgTile TI = J.it[wi + b * J.n_wi];
        const int on = wg_orig(TI.kind, n);
        wg_f4 sum = {0.f, 0.f, 0.f, 0.f};
        const float* src = base + (size_t)((wave * WG_NOT + a) * nitw + b) * 1024 + rq * 256 + lane * 4;
        // eight parts in flight at a time (a dependent chain of ~20 loads would cost the launch their latencies); the order is fixed
        const size_t pl = (size_t)A.part_len[j];
        int p = 0;
        for (; p + 8 <= live; p += 8) {
            wg_f4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const wg_f4*>(src + (size_t)(p + u) * pl);
            sum += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
        for (; p < live; ++p) sum += *reinterpret_cast<const wg_f4*>(src + (size_t)p * pl);
        if (on < TI.nvalid) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = 4 * rq + k;
                const int oi = wg_orig(TO.kind, (r & 3) + 8 * (r >> 2) + 4 * hh);
                if (oi < TO.nvalid) W[(size_t)(TO.idx0 + oi) * J.ld + TI.idx0 + on] = sum[k] * inv;
            }
        }
    }
    if (b == 0 && rq == 0 && J.do_bias && wi == 0 && layer != WG_SCRATCH && A.g.bias[layer] != nullptr) {
        const float* src = base + (size_t)4 * WG_NOT * nitw * 1024 + (wave * WG_NOT + a) * 64 + lane;
        float sb = 0.f;
        for (int p = 0; p < live; ++p) sb += src[(size_t)p * A.part_len[j]];
        const float tot = sb + __shfl_xor(sb, 32);
        const int oi = wg_orig(TO.kind, n);
        if (hh == 0 && oi < TO.nvalid) A.g.bias[layer][TO.idx0 + oi] = tot * inv;
    }
}

typedef unsigned wg_u4 __attribute__((ext_vector_type(4)));
// scalar base (the segment's record, uniform) + 32-bit per-lane offset: one VGPR of address per piece instead of two
__device__ __forceinline__ void wg_gload(wg_u4& dst, unsigned voff, const char* sbase) {
    asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(dst) : "v"(voff), "s"(sbase));
}
// wait until at most N vector-memory operations are outstanding; the register set rides through so its users stay below
template <int N, int PW>
__device__ __forceinline__ void wg_landed(wg_u4 (&r)[PW]) {
    static_assert(N < 64, "vmcnt is a 6-bit counter");
    static_assert(PW == 4 || PW == 5 || PW == 6 || PW == 8 || PW == 12 || PW == 16, "piece counts the dispatcher uses");
    if constexpr (PW == 4)
        asm volatile("s_waitcnt vmcnt(%4)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : "n"(N));
    else if constexpr (PW == 5)
        asm volatile("s_waitcnt vmcnt(%5)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]) : "n"(N));
    else if constexpr (PW == 6)
        asm volatile("s_waitcnt vmcnt(%6)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]) : "n"(N));
    else if constexpr (PW == 8)
        asm volatile("s_waitcnt vmcnt(%8)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]),
                     "+v"(r[6]), "+v"(r[7]) : "n"(N));
    else if constexpr (PW == 12)
        asm volatile("s_waitcnt vmcnt(%12)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]),
                     "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]) : "n"(N));
    else
        asm volatile("s_waitcnt vmcnt(%16)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]),
                     "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]),
                     "+v"(r[14]), "+v"(r[15]) : "n"(N));
}

// The stream is staged through REGISTERS.  An LDS-DMA ring (the first design: 4 slots of 32-40 KiB, 1.43 ms per
// fine pass) caps the bytes a workgroup keeps outstanding at what fits in the 160 KB of LDS, and this kernel waits
// for HBM ~60 % of the time, so bytes in flight are what counts.  Here every wave keeps D segments of its own
// 1 KiB pieces in flight in registers (nontemporal global_load_dwordx4, 4 VGPRs per piece; PW = pieces per wave
// per segment, NITW = in tiles per wave), copies the oldest set into a 2-slot LDS double buffer with
// ds_write_b128 when its turn comes, and re-issues loads into the freed registers at once: 1.13 ms = 5.7 TB/s.
// One barrier per segment; no branch inside a segment: a wave whose share is short works on a clamped
// (duplicate) tile and drops it at the flush.
// SPLIT (three-product weight gradient, NFL_PREC_F16X3): the residual images of every tile travel with the hi images (twice
// the pieces per segment, the lo pieces behind the hi pieces in the LDS slot) and every accumulator gets
// d_hi (x) h_hi + d_lo (x) h_hi + d_hi (x) h_lo -- one pass over hi + lo instead of three passes of the one-product GEMM.
template <int PW, int NITW, int D, bool SPLIT = false>
__device__ __forceinline__ void wg_body_rs(const WgArgs& A, const WgJob& J, const int act_slots, const int grd_slots,
                                           const int seg0, const int seg1, const int seg_first, const int seg_step, const int jidx, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave % J.n_wo, wi = wave / J.n_wo;
    const int n_hi = 2 * (J.n_ot + J.n_it);
    const int n_pieces = SPLIT ? 2 * n_hi : n_hi;

    unsigned poff[PW];          // byte offset of this lane's 16 B of the piece inside its segment record
    unsigned outmask = 0u;      // bit pp: piece pp comes from the gradient stash (else: activation stash)
    int pdst[PW];
#pragma unroll
    for (int pp = 0; pp < PW; ++pp) {
        int p = wave + 4 * pp;           // (wave * PW + pp, a wave's pieces contiguous in the record, runs at the same speed: measured)
        p = p < n_pieces ? p : n_pieces - 1;
        const bool lo = p >= n_hi;
        const int q = lo ? p - n_hi : p;
        const int t = q >> 1;
        const bool is_out = t < J.n_ot;
        const int slot = (is_out ? J.ot[t].slot : J.it[t - J.n_ot].slot) + (q & 1);
        poff[pp] = (unsigned)slot * 1024u + lane * 16u + (lo ? (unsigned)(is_out ? A.grd_lo : A.act_lo) : 0u);
        outmask |= is_out ? (1u << pp) : 0u;
        pdst[pp] = p * WG_PSTRIDE + lane * 16;
    }
    outmask = __builtin_amdgcn_readfirstlane(outmask);
    const size_t grd_stride = (size_t)grd_slots * 1024, act_stride = (size_t)act_slots * 1024;
    // The loads and their waits are hand-issued: left to hipcc the loop header gets an s_waitcnt vmcnt(0), which
    // drains all D segments once per trip.  VMEM operations return in order, so "all but the (D-1)*PW youngest"
    // is exactly "the oldest register set has landed"; nothing else in the loop touches vector memory.
    wg_u4 R[D][PW];
    auto gload = [&](int seg, auto DD) __attribute__((always_inline)) {
        constexpr int d = decltype(DD)::value;
        // logical segment `seg` of this workgroup is record seg_first + seg * seg_step of the stashes (see the kernel below)
        const int sg = seg_first + (seg < seg1 ? seg : seg1 - 1) * seg_step;          // surplus loads re-read the last segment
        const char* bo = A.grd + (size_t)sg * grd_stride;
        const char* bi = A.act + (size_t)sg * act_stride;
#pragma unroll
        for (int pp = 0; pp < PW; ++pp) wg_gload(R[d][pp], poff[pp], ((outmask >> pp) & 1u) ? bo : bi);
    };

    int my_ot[WG_NOT], my_it[NITW];
#pragma unroll
    for (int a = 0; a < WG_NOT; ++a) my_ot[a] = wo * WG_NOT + a < J.n_ot ? wo * WG_NOT + a : J.n_ot - 1;
#pragma unroll
    for (int b = 0; b < NITW; ++b) my_it[b] = wi + b * J.n_wi < J.n_it ? wi + b * J.n_wi : J.n_it - 1;

    f16v acc[WG_NOT][NITW];
#pragma unroll
    for (int a = 0; a < WG_NOT; ++a)
#pragma unroll
        for (int b = 0; b < NITW; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    float bsum[WG_NOT] = {0.f, 0.f};
    // tile offsets inside a slot, in registers: J lives in global memory and the asm memory clobbers below would
    // otherwise make the loop re-load J.n_ot (a vmcnt(0) wait per segment)
    int ot_off[WG_NOT], it_off[NITW];
#pragma unroll
    for (int a = 0; a < WG_NOT; ++a) ot_off[a] = my_ot[a] * WG_TSTRIDE;
#pragma unroll
    for (int b = 0; b < NITW; ++b) it_off[b] = (J.n_ot + my_it[b]) * WG_TSTRIDE;

#ifdef NFL_DIAG_WGRAD_LDSDMA
    // timing ablation (nfl_diag.h): the same pieces of the same segments, fetched by LDS-DMA (global_load_lds, 16 B per lane) straight
    // into the two LDS slots instead of through registers; nothing consumes them, nothing is flushed -- what does THAT stream sustain?
    if (A.n_seg >= 0) {
        auto dma = [&](int seg) __attribute__((always_inline)) {
            const int sg = seg_first + (seg < seg1 ? seg : seg1 - 1) * seg_step;
            const char* bo = A.grd + (size_t)sg * grd_stride;
            const char* bi = A.act + (size_t)sg * act_stride;
            char* slot = smem + ((seg - seg0) & 1) * A.slot_bytes;
#pragma unroll
            for (int pp = 0; pp < PW; ++pp) {
                const char* src = (((outmask >> pp) & 1u) ? bo : bi) + poff[pp];
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(slot + (pdst[pp] - lane * 16)), 16, 0, 0);
            }
        };
        dma(seg0);
        dma(seg0 + 1);
        for (int seg = seg0; seg < seg1; ++seg) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PW) : "memory");      // all but the youngest segment's pieces: `seg` has landed
            dma(seg + 2);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }
#endif
    nfl_static_for<0, D>([&](auto DD) __attribute__((always_inline)) { gload(seg0 + decltype(DD)::value, DD); });
    for (int base = seg0; base < seg1; base += D) {
        nfl_static_for<0, D>([&](auto DD) __attribute__((always_inline)) {
            constexpr int d = decltype(DD)::value;
            const int seg = base + d;
            if (seg < seg1) {                                     // uniform
                char* slot = smem + ((seg - seg0) & 1) * A.slot_bytes;
                wg_landed<(D - 1) * PW, PW>(R[d]);
#ifdef NFL_DIAG_WGRAD_LOADS_ONLY
                // timing ablation (nfl_diag.h): the load stream alone -- no LDS round trip, no barrier, no MFMA; results wrong by construction
                if (A.n_seg >= 0) {
#pragma unroll
                    for (int pp = 0; pp < PW; ++pp) bsum[0] += __uint_as_float(R[d][pp].x ^ R[d][pp].y ^ R[d][pp].z ^ R[d][pp].w);
                    gload(seg + D, DD);
                    return;
                }
#endif
#pragma unroll
                for (int pp = 0; pp < PW; ++pp) *reinterpret_cast<wg_u4*>(slot + pdst[pp]) = R[d][pp];
                gload(seg + D, DD);
                __builtin_amdgcn_sched_barrier(0);
                // raw barrier: __syncthreads() carries a fence that hipcc lowers to s_waitcnt vmcnt(0), which would
                // drain the D segments in flight; only the LDS writes have to be complete here
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                const char* base_l = slot;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    h8 av[WG_NOT], bv[NITW];
#pragma unroll
                    for (int a = 0; a < WG_NOT; ++a) av[a] = wg_operand(base_l + ot_off[a], lane, m);
#pragma unroll
                    for (int b = 0; b < NITW; ++b) bv[b] = wg_operand(base_l + it_off[b], lane, m);
#pragma unroll
                    for (int a = 0; a < WG_NOT; ++a) {
                        float sacc = 0.f;
#pragma unroll
                        for (int j = 0; j < 8; ++j) sacc += (float)av[a][j];
                        bsum[a] += sacc;
                    }
#pragma unroll
                    for (int b = 0; b < NITW; ++b)
#pragma unroll
                        for (int a = 0; a < WG_NOT; ++a)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[a], bv[b], acc[a][b], 0, 0, 0);
                    if constexpr (SPLIT) {
                        const char* base_lo = base_l + n_hi * WG_PSTRIDE;        // the lo pieces follow the hi pieces
                        h8 al[WG_NOT];
#pragma unroll
                        for (int a = 0; a < WG_NOT; ++a) {
                            al[a] = wg_operand(base_lo + ot_off[a], lane, m);
                            float sacc = 0.f;
#pragma unroll
                            for (int j = 0; j < 8; ++j) sacc += (float)al[a][j];
                            bsum[a] += sacc;                              // db = sum_s (d_hi + d_lo)
                        }
#pragma unroll
                        for (int b = 0; b < NITW; ++b)
#pragma unroll
                            for (int a = 0; a < WG_NOT; ++a)
                                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[a], bv[b], acc[a][b], 0, 0, 0);
#pragma unroll
                        for (int b = 0; b < NITW; ++b) {
                            const h8 bl = wg_operand(base_lo + it_off[b], lane, m);
#pragma unroll
                            for (int a = 0; a < WG_NOT; ++a)
                                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[a], bl, acc[a][b], 0, 0, 0);
                        }
                    }
                }
            }
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the surplus loads still target live registers
    wg_flush<NITW>(A, jidx, (int)blockIdx.x - A.wg_start[jidx], acc, bsum, wave, lane);
}

// wg_body_rs in the instantiation of row I of WG_INST (nfl_wgrad_plan.h)
template <bool SPLIT, int I>
__device__ __forceinline__ void wg_row(const WgArgs& A, const WgJob& J, const int seg0, const int seg1, const int seg_first,
                                       const int seg_step, const int j, char* smem) {
    constexpr WgInst T = WG_INST[SPLIT][I];
    static_assert(T.cost == WG_INST[0][I].cost && T.nitw == WG_INST[0][I].nitw, "the split kernel's rows are the one-product kernel's");
    static_assert(T.pw >= (SPLIT ? 2 : 1) * T.cost, "the four waves hold every piece of the class");
    wg_body_rs<T.pw, T.nitw, T.d, SPLIT>(A, J, A.act_rec, A.grd_rec, seg0, seg1, seg_first, seg_step, j, smem);
}

template <bool SPLIT>
__global__ __launch_bounds__(256, 1) void nfl_wgrad_kernel(const WgArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const WgPlan& P = *A.plan;
    int j = 0;
    while (j + 1 < P.n_jobs && (int)blockIdx.x >= A.wg_start[j + 1]) ++j;
    const int part = blockIdx.x - A.wg_start[j], nparts = A.wg_start[j + 1] - A.wg_start[j];
    // The job's workgroups take its segments ROUND-ROBIN (workgroup `part` of `nparts`: records part, part + nparts, ...), not one
    // contiguous range each: every job crosses the stashes at the same pace (that is what the dealing equalises), so all 256
    // workgroups then read the same neighbourhood of memory at any time.  Same-box A/B against contiguous ranges
    // (-DWG_SEGMENTS_CONTIGUOUS): 0.918 vs 0.934 ms per fine pass, the split kernel of f16x3 2.10 vs 2.21
#ifdef WG_SEGMENTS_CONTIGUOUS
    const int seg_first = (int)((long long)A.n_seg * part / nparts), seg_step = 1;
    const int seg0 = 0, seg1 = (int)((long long)A.n_seg * (part + 1) / nparts) - seg_first;
#else
    const int seg_first = part, seg_step = nparts;
    const int seg0 = 0, seg1 = part < A.n_seg ? (A.n_seg - part + nparts - 1) / nparts : 0;
#endif
    if (seg0 >= seg1) return;
    const WgJob& J = P.job[j];
    const int pw = P.cost[j];
    const int nitw = (J.n_it + J.n_wi - 1) / J.n_wi;       // in tiles per wave
    // wg_inst_row(pw, nitw) as a ladder: every rung runs the row that the table gives for the largest (pw, nitw) it admits
    // (the planner rejects a job without a row, so the last rung of a class does not compare nitw, nor the last class pw)
#define WG_RUN(PW_, NITW_) wg_row<SPLIT, wg_inst_row(PW_, NITW_)>(A, J, seg0, seg1, seg_first, seg_step, j, smem)
    if (pw <= 4) {
        if (nitw <= 1) WG_RUN(4, 1);
        else WG_RUN(4, 2);
    } else if (pw <= 5) {
        WG_RUN(5, 2);
    } else if (pw <= 6) {          // layers 1 / 5a of a field with 11..15 position frequencies: 8 out x 3 in tiles
        WG_RUN(6, 4);
    } else {
        if (nitw <= 5) WG_RUN(8, 5);
        else if (nitw <= 6) WG_RUN(8, 6);
        else WG_RUN(8, 8);
    }
#undef WG_RUN
}

// Zeroes the gradient tensors and the composition scratch before the stream: the reduction stores only the elements a job owns.
// blockIdx.y = tensor, blockIdx.x strides over its elements.
__global__ __launch_bounds__(256) void nfl_wgrad_zero_kernel(const WgTensors T) {
    float* p = T.ptr[blockIdx.y];
    if (p == nullptr) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < T.n[blockIdx.y]; i += gridDim.x * 256) p[i] = 0.f;
}

void nfl_compose_launch(const WgCompose& Cc, hipStream_t s);      // nfl_compose.hip

// Every refusal (nfl_wgrad_check, the schedule, the composition's task list) comes before the first launch: a refused call
// leaves the gradient tensors as they were.
extern "C" int nfl_mlp_wgrad(const void* h_wplan, const void* d_wplan, const char* d_act_stash,
                             const char* d_grad_stash, const float* d_gmax, int32_t n_rays, int32_t n_samples,
                             int32_t bwd_prec, const nfl_field_params* params, float* d_scratch,
                             const nfl_field_grads* grads, void* stream) {
    int rc = nfl_wgrad_check(h_wplan, d_wplan, d_act_stash, d_grad_stash, d_gmax, n_rays, n_samples, bwd_prec, params, d_scratch, grads);
    if (rc != NFL_OK) return rc;
    const WgPlan* hp = static_cast<const WgPlan*>(h_wplan);
    const int mult = bwd_prec == NFL_PREC_F16X3 ? 2 : 1;       // split stashes: [hi record | lo record] per segment
    int n_wg = 0, red_blocks = 0;
    const NflDevice dev = nfl_device();
    WgArgs A;
    memset(&A, 0, sizeof(A));
    rc = nfl_wgrad_schedule(hp, n_rays * ((n_samples + 31) / 32), dev.n_cu, mult, &A, &n_wg, &red_blocks);
    if (rc != NFL_OK) return rc;
    WgTensors T;
    nfl_wgrad_fill(hp, d_wplan, d_act_stash, d_grad_stash, grads, d_scratch, &A, &T);
    WgCompose Cc;      // the composition through xyz_encoding_final (file header)
    rc = nfl_compose_backward_tasks(hp, params, grads, d_scratch, &Cc);
    if (rc != NFL_OK) return rc;
    if (nfl_lds_attr<&nfl_wgrad_kernel<false>>(dev.ordinal, 2 * WG_SLOT) != NFL_OK ||
        nfl_lds_attr<&nfl_wgrad_kernel<true>>(dev.ordinal, 4 * WG_SLOT) != NFL_OK)
        return NFL_ENODEV;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nfl_wgrad_zero_kernel, dim3(16, WG_NTENS), dim3(256), 0, s, T);
    if (n_rays == 0) return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
    // NFL_PREC_F16X3: dW = sum_s (d_hi + d_lo) (x) (h_hi + h_lo) without the lo x lo term, in ONE pass over the hi and lo
    // records (fp16 x fp16 products are exact in the fp32 accumulators, so what is left is the 2^-22 lo x lo term and the
    // summation order); the bias gradients are sum_s (d_hi + d_lo).
    if (mult == 2) hipLaunchKernelGGL(nfl_wgrad_kernel<true>, dim3(n_wg), dim3(256), 2 * A.slot_bytes, s, A);
    else hipLaunchKernelGGL(nfl_wgrad_kernel<false>, dim3(n_wg), dim3(256), 2 * A.slot_bytes, s, A);
    // parts -> gradient tensors and G, summed in a fixed order and divided by the loss scale (what the tensors' zeroing above
    // still covers: elements no job owns, i.e. the heads a call leaves out)
    hipLaunchKernelGGL(nfl_wgrad_reduce_kernel, dim3(red_blocks), dim3(256), 0, s, A, d_gmax);
    if (Cc.n_wg > 0) nfl_compose_launch(Cc, s);      // G, db_dir, db_t0 are final (unscaled) by now
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
