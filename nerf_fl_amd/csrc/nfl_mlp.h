// nfl_mlp.h -- the register-resident MLP engine that the forward kernel (nfl_render_impl.h) and the dgrad kernel
// (nfl_dgrad.hip) share: weight ring, MFMA row tile, activation epilogue, dense layer and head.  Mapping onto CDNA4:
//   * the MLP is evaluated transposed, H^T[out,sample] = W[out,in] . H^T[in,sample] with v_mfma_f32_32x32x16_f16.
//     Activations live in registers for the whole network: the 32x32 fp32 accumulator tile of one layer, converted to
//     fp16, IS the B operand of the next layer (column = sample stays on the lane; the k-slot permutation this implies
//     is folded into the packed weights, nfl_plan.h).
//   * W streams global(L2) -> LDS through a 3-slot ring with global_load_lds (16 B per lane, lane-linear = exactly the
//     fragment image), one raw s_barrier per chunk and a counted vmcnt so two chunks stay in flight across barriers;
//     all four waves read every fragment with conflict-free ds_read_b128.
//   * NSPLIT == 3: operands are split hi+lo in fp16 and three products are accumulated (w_lo*x_hi + w_hi*x_lo +
//     w_hi*x_hi): ~2^-21 relative error per product instead of 2^-11, at 3x the MFMA issue.  NSPLIT == 1 is the fast mode.
#pragma once
#include "nfl_dev.h"
#include "nfl_diag.h"
#include "nfl_math.h"
#include "nfl_plan.h"
#include "nfl_prods.h"

__device__ __forceinline__ f16v nfl_mfma(h8 a, h8 b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// stash stores are streaming (nt): A/B on one box, training forward 1.69 ms with nt, 1.74 with plain stores (step 5.20 / 5.36 ms)
#define NFL_STREAM_STORE(v, p) __builtin_nontemporal_store(v, p)

// 8 values -> fp16 -> this lane's 16 B of a stash k-step (dst already includes lane*16); LO != 0: the fp16 residuals
// x - fp16(x) go LO bytes behind (split stashes of the three-product backward, nfl_plan.h)
template <int LO = 0>
NFL_DEV void nfl_stash8(const float (&v)[8], char* dst) {
    h8 t, tl;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        if constexpr (LO != 0) {
            float l0, l1;
            reinterpret_cast<unsigned(&)[4]>(t)[j / 2] = nfl_split_pair<_Float16>(v[j], v[j + 1], l0, l1);
            reinterpret_cast<unsigned(&)[4]>(tl)[j / 2] = nfl_pack2<_Float16>(l0, l1);
        } else {
            reinterpret_cast<unsigned(&)[4]>(t)[j / 2] = nfl_pack2<_Float16>(v[j], v[j + 1]);
        }
    }
    NFL_STREAM_STORE(t, reinterpret_cast<h8*>(dst));
    if constexpr (LO != 0) NFL_STREAM_STORE(tl, reinterpret_cast<h8*>(dst + LO));
}

// natural-order B operand of one k-step of a positional encoding: lane half h holds
// features 16*ks + 8*h + j.  Both candidates are evaluated per-lane via selects so the
// instruction stream is uniform.
template <int N, int NP, int LO = 0>
NFL_DEV void nfl_pe_kstep(int ks, int h, const float (&raw)[3], const float (&th)[3], const float (&tl)[3],
                          const float* pw, h8 (&dst)[NP], char* stash = nullptr) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int f0 = 16 * ks + j, f1 = f0 + 8;
        // select the feature descriptor by lane half, then evaluate once
        if (f0 < 3 || f0 >= 6 * N + 3 || f1 >= 6 * N + 3) {
            const float v0 = nfl_pe_feature<N>(f0, raw, th, tl, pw);
            const float v1 = nfl_pe_feature<N>(f1, raw, th, tl, pw);
            v[j] = h ? v1 : v0;
        } else {
            const int g0 = f0 - 3, g1 = f1 - 3;
            const int k0 = g0 / 6, k1 = g1 / 6, t0 = (g0 % 6) / 3, t1 = (g1 % 6) / 3, c0 = g0 % 3, c1 = g1 % 3;
            const float sc = h ? (float)(1 << k1) : (float)(1 << k0);
            const float thc = h ? th[c1] : th[c0];
            const float tlc = h ? tl[c1] : tl[c0];
            const float ph = h ? 0.25f * t1 : 0.25f * t0;
            const float r = __builtin_amdgcn_fractf(thc * sc) + tlc * sc + ph;
            v[j] = (h ? pw[k1] : pw[k0]) * nfl_sin_rev(r);
        }
    }
    nfl_split8<NP>(v, dst);
    if (stash) {        // the operand images ARE the stash (hi; with LO the residuals too)
        NFL_STREAM_STORE(dst[0], reinterpret_cast<h8*>(stash));
        if constexpr (LO != 0 && NP == 2) NFL_STREAM_STORE(dst[NP - 1], reinterpret_cast<h8*>(stash + LO));
    }
}

// ---------------------------------------------------------------------------------
// weight ring: global -> LDS by LDS-DMA, 3 slots, prefetch distance 2
// ---------------------------------------------------------------------------------
template <int SLOT_BYTES, int MAXP_>
struct NflRing {
    static constexpr int MAXP = MAXP_;     // DMA pieces (1 KiB per wave-instruction) every wave issues per chunk
    const char* gsrc;
    const int* chunk_off;
    char* lds;          // ring base (LDS)
    int n_chunks;
    int c_issue;        // next chunk (index within the per-tile stream) to issue
    int s_issue;        // slot it goes to
    int s_read;         // slot of the next chunk to consume
    int wave, lane;
    // chunk currently being issued (pieces are spread over the MFMA loop of the chunk being consumed)
    const char* i_src;
    char* i_dst;
    int i_nbytes;

#ifdef NFL_STAMPS
    unsigned long long t_wait = 0, t_bar = 0;   // cycles in consume(): DMA wait / workgroup barrier
#endif
    int n_off0, n_off1;   // table entries of chunk c_issue, fetched one step ahead (no LDS latency after the barrier)
    // Not ring state, but it travels with the ring through every layer: per-lane running maximum (packed u16 pair) of
    // the |fp16 bit patterns| the activation epilogues have formed.  >= 0x7c00 at the end of the kernel means an
    // activation left fp16's range (the conversion gave inf); reported through nfl_pass_args::d_status.
    unsigned ovf = 0;

    NFL_DEV void begin_issue() {
        i_nbytes = n_off1 - n_off0;
        i_src = gsrc + n_off0;               // wave-uniform; the lane offset is added per piece (keeps no 64-bit VGPR live)
        i_dst = lds + s_issue * SLOT_BYTES;
        c_issue = c_issue + 1 == n_chunks ? 0 : c_issue + 1;
        s_issue = s_issue == 2 ? 0 : s_issue + 1;
        n_off0 = __builtin_amdgcn_readfirstlane(chunk_off[c_issue]);
        n_off1 = __builtin_amdgcn_readfirstlane(chunk_off[c_issue + 1]);
    }
    template <int P>
    NFL_DEV void piece() {
        if constexpr (P < MAXP) {
            // uniform byte offset (SALU min), one VALU add for the lane: SGPR base + 32-bit VGPR offset
            unsigned byte = (unsigned)(wave + 4 * P) * 1024u;
            const unsigned last = (unsigned)i_nbytes - 1024u;
            byte = byte < last ? byte : last;                      // surplus pieces re-copy the last KiB
            const unsigned vo = byte + (threadIdx.x & 63) * 16u;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(i_src + vo),
                (__attribute__((address_space(3))) void*)(i_dst + byte), 16, 0, 0);
        }
    }
    template <int P0, int P1>
    NFL_DEV void pieces() {                 // pieces [P0, P1)
        nfl_static_for<P0, P1>([&](auto P) __attribute__((always_inline)) { piece<decltype(P)::value>(); });
    }
    NFL_DEV void prime() {
        n_off0 = __builtin_amdgcn_readfirstlane(chunk_off[c_issue]);
        n_off1 = __builtin_amdgcn_readfirstlane(chunk_off[c_issue + 1]);
        begin_issue();
        pieces<0, MAXP>();
        begin_issue();
        pieces<0, MAXP>();
    }
    // Wait for the oldest chunk in flight, make it visible to all waves and return this lane's
    // read base; the caller then issues the MAXP pieces of the next chunk (piece<P>()) while it
    // computes, into the slot everybody has just finished reading.
    // EXTRA: VMEM ops (stash stores) known to have been issued after the pieces of the chunk waited for,
    // besides the MAXP pieces of the next one -- without it the wait would also sit on those stores.
    template <int EXTRA = 0>
    NFL_DEV const char* consume() {
#if defined(NFL_STAMPS) && NFL_STAMPS >= 2
        const unsigned long long c0 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(MAXP + EXTRA) : "memory");
        const unsigned long long c1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_barrier();
        t_wait += c1 - c0;
        t_bar += __builtin_amdgcn_s_memtime() - c1;
#else
        // all but the MAXP (+EXTRA) youngest VMEM ops (= the younger chunk's pieces) are done
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(MAXP + EXTRA) : "memory");
        __builtin_amdgcn_s_barrier();
#endif
        asm volatile("" ::: "memory");
        begin_issue();
        const char* base = lds + s_read * SLOT_BYTES + (threadIdx.x & 63) * 16;
        s_read = s_read == 2 ? 0 : s_read + 1;
        return base;
    }
};

// ---------------------------------------------------------------------------------
// MFMA building blocks
// ---------------------------------------------------------------------------------
template <int NP, int NCB>
NFL_DEV void nfl_bias_init(f16v (&acc)[NCB], const float* bias_rt, int h) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f4v b = *reinterpret_cast<const f4v*>(bias_rt + 8 * q + 4 * h);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            acc[cb][4 * q + 0] = b[0];
            acc[cb][4 * q + 1] = b[1];
            acc[cb][4 * q + 2] = b[2];
            acc[cb][4 * q + 3] = b[3];
        }
    }
}

// One row tile, software-pipelined in source order.  Every MFMA is followed by a few
// "fillers" that fit in the issue slots it leaves free (an MFMA holds the issue port for 8 of
// its 32 cycles): the LDS reads of k-step k+2, one LDS-DMA piece of the chunk being prefetched,
// and a slice of the PREVIOUS tile's VALU epilogue.  sched_barrier(0) after each micro-slice
// pins that order (hipcc otherwise emits the DMA pieces and the epilogue back to back after
// the barrier, with the matrix pipe idle).
//   getb(K, cb, part) -> B operand of k-step K;  epi.template step<K, NK>() runs the epilogue
//   work assigned to k-step K;  pieces P0+k are issued at k-step k.
// The weight fragments are read with hand-issued ds_read_b128 and hand-counted s_waitcnt lgkmcnt(N): left to
// hipcc, every third k-step got an `s_waitcnt lgkmcnt(0)` that also waits for the reads issued one instruction
// earlier for k+2, so the full LDS latency was exposed once per three k-steps (1.4x the MFMA time with three
// products per k-step, 2x with one).  LDS operations return in order, so "all but the N youngest" is exact: N =
// the reads of k-step k+1.  Any LDS operation the compiler adds in between only makes the wait stricter.
typedef unsigned nfl_u4 __attribute__((ext_vector_type(4)));
template <int OFF>
NFL_DEV nfl_u4 nfl_lds_read128(unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field is 16 bits");
    nfl_u4 r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
    return r;
}
// wait until at most N LDS operations are outstanding; the operands ride through so that their users stay below
template <int N, int NREAD, int NWP>
NFL_DEV void nfl_lds_wait(nfl_u4 (&w)[NWP]) {
    if constexpr (NREAD == 2) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(w[0]), "+v"(w[1]) : "n"(N));
    else asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(w[0]) : "n"(N));
}

// DEPTH = how many k-steps ahead the fragments are read (DEPTH + 1 register sets).  Two k-steps are 6 MFMAs with
// three products per k-step but only 2 with one: the single-product kernels read 4 ahead, or every k-step waits
// out most of the LDS latency (in-kernel stamps: 3.3 k cycles per 32-MFMA row tile with DEPTH 2).
#ifndef NFL_DEPTH_X3
#define NFL_DEPTH_X3 2
#endif
// PRODS (three-product mode only): which of the two correction products a layer issues besides w_hi x_hi --
// bit 0: w_lo x_hi (the weights' fp16 residuals; without it the layer's weights are fp16-rounded and their lo fragments
// are not even read from LDS), bit 1: w_hi x_lo (the activations' residuals).  3 = the full f16x3 product.  The per-layer
// plan is NFL_PRODS (nfl_prods.h), chosen by measurement against the parity bar (tests/report_parity.py).
// bit 2 (NP == 1 only): the stream carries hi + lo WEIGHT fragments although the B operands are single fp16 images -- the
// default dgrad (nfl_dgrad.hip): W_hi d_hi + W_lo d_hi, the weights to fp32 class, the gradients fp16.
template <int PRODS, int NP, int NCB, int NK, int P0, class V8, class GetB, class Epi, class Ring,
          int DEPTH = ((NP == 1 && (PRODS & 4) == 0) ? 4 : NFL_DEPTH_X3)>
NFL_DEV void nfl_tile_p(f16v (&acc)[NCB], const char* wl, const int frag0, GetB&& getb, Epi&& epi, Ring& ring) {
    constexpr int NWP = (NP == 2 || (PRODS & 4) != 0) ? 2 : 1;          // weight fragments per k-step: hi (+ lo)
    constexpr int KSB = 1024 * NWP;
    constexpr int NW = DEPTH + 1;
    constexpr bool W_LO = NWP == 2 && (PRODS & 1) != 0, X_LO = NP == 2 && (PRODS & 2) != 0;
    constexpr int NREAD = W_LO ? 2 : 1;     // LDS reads per k-step
    (void)frag0;                          // == P0 (kept in the signature for the callers' readability)
    nfl_u4 w[NW][NWP];
    const unsigned wa = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)wl;
    auto load = [&](auto K) __attribute__((always_inline)) {
        constexpr int k = decltype(K)::value;
        w[k % NW][0] = nfl_lds_read128<(P0 + k) * KSB>(wa);
        if constexpr (W_LO) w[k % NW][NWP - 1] = nfl_lds_read128<(P0 + k) * KSB + 1024>(wa);
    };
    nfl_static_for<0, (DEPTH < NK ? DEPTH : NK)>([&](auto K) __attribute__((always_inline)) { load(K); });
    epi.early();                         // VALU work that hides the latency of the first LDS reads
    __builtin_amdgcn_sched_barrier(0);
    nfl_static_for<0, NK>([&](auto K) __attribute__((always_inline)) {
        constexpr int k = decltype(K)::value;
        // k-step k has landed; the reads of k+1 .. k+DEPTH-1 (already issued) may still be in flight
        constexpr int younger = (NK - 1 - k) < (DEPTH - 1) ? (NK - 1 - k) : (DEPTH - 1);
        nfl_lds_wait<younger * NREAD, NREAD>(w[k % NW]);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            // fillers of the k-step (the LDS reads of k + DEPTH, one DMA piece) ride behind its first two MFMAs
            if constexpr (W_LO) {
                acc[cb] = nfl_mfma(__builtin_bit_cast(V8, w[k % NW][NWP - 1]), getb(K, cb, 0), acc[cb]);
                if (cb == 0) {
                    if constexpr (k + DEPTH < NK) load(std::integral_constant<int, k + DEPTH>{});
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (X_LO) {
                acc[cb] = nfl_mfma(__builtin_bit_cast(V8, w[k % NW][0]), getb(K, cb, NP - 1), acc[cb]);
                if (cb == 0) {
                    if constexpr (!W_LO && k + DEPTH < NK) load(std::integral_constant<int, k + DEPTH>{});
                    ring.template piece<P0 + k>();
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            acc[cb] = nfl_mfma(__builtin_bit_cast(V8, w[k % NW][0]), getb(K, cb, 0), acc[cb]);
            if (cb == 0) {
                if constexpr (!W_LO && !X_LO && k + DEPTH < NK) load(std::integral_constant<int, k + DEPTH>{});
                if constexpr (!X_LO) ring.template piece<P0 + k>();
            }
            if (cb == NCB - 1) epi.template step<k, NK>();
            __builtin_amdgcn_sched_barrier(0);
        }
    });
}
template <int NP, int NCB, int NK, int P0, class V8, class GetB, class Epi, class Ring>
NFL_DEV void nfl_tile(f16v (&acc)[NCB], const char* wl, const int frag0, GetB&& getb, Epi&& epi, Ring& ring) {
    nfl_tile_p<3, NP, NCB, NK, P0, V8>(acc, wl, frag0, getb, epi, ring);
}

struct NflNoEpi {
    template <int K, int NK> NFL_DEV void step() {}
    NFL_DEV void early() {}
};
#ifndef NFL_EPI_EARLY
#define NFL_EPI_EARLY 2      // pair-ops done before the first MFMA of the following tile
#endif

// Epilogue of an accumulator tile -> the two k-steps (ks, ks+1) of the next layer's B operand
// (and, in the training forward, the fp16 activation stash), cut into 8 pair-ops per column
// block so it can be spread over the k-steps of the following tile.
template <int NP, int NCB, bool RELU, bool STASH, int NOUT, int MSLOT, int LO = 0, bool ZST = false>
struct NflActEpi {
    const f16v (&acc)[NCB];
    h8 (&out)[NOUT][NCB][NP];
    const int ks;
    char* const (&stash)[NCB];
    const int slot;
    char* const (&mstash)[NCB];      // relu-mask records of the lane's segments (training forward)
    const int mword;                 // mask word of this tile
    unsigned (&mq)[NCB][4];          // the words of the current group of four tiles: one dwordx4 store per group
    unsigned& ovf;                   // NflRing::ovf
    float* const* zc;                // ZST: per segment, the lane's sample column of its ray's appearance cache
    const int zpad;                  // ZST: sample stride of the cache
    h8 tmp[NCB];
    h8 tmpl[LO != 0 ? NCB : 1];      // residual halves for the split stash (LO: their byte offset behind the hi image)
    unsigned m32[NCB];

    template <int OP>
    NFL_DEV void pair() {                      // OP 0..7: elements 2*OP, 2*OP+1 of the 16 accumulators
        constexpr int s = OP / 4, j = 2 * (OP % 4);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            float x0 = acc[cb][8 * s + j], x1 = acc[cb][8 * s + j + 1];
            if constexpr (ZST) {        // NFL_MODE_ZCACHE: the fp32 pre-activation of features f, f + 1 (NFL_SEG_ACT)
                const int f = 16 * (ks + s) + 8 * (j >> 2) + 4 * (int)((threadIdx.x & 63) >> 5) + (j & 3);
                zc[cb][(size_t)f * zpad] = x0;
                zc[cb][(size_t)(f + 1) * zpad] = x1;
            }
            if (RELU) {
                x0 = nfl_relu(x0);
                x1 = nfl_relu(x1);
            }
            unsigned hi;
            if constexpr (NP == 2) {
                float l0, l1;
                hi = nfl_split_pair<_Float16>(x0, x1, l0, l1);
                const unsigned lo = nfl_pack2<_Float16>(l0, l1);
                reinterpret_cast<unsigned(&)[4]>(out[ks + s][cb][NP - 1])[j / 2] = lo;
                if constexpr (STASH && LO != 0) {
                    reinterpret_cast<unsigned(&)[4]>(tmpl[cb])[j / 2] = lo;
                    if (OP % 4 == 3) NFL_STREAM_STORE(tmpl[cb], reinterpret_cast<h8*>(stash[cb] + LO + (slot + s) * 1024));
                }
            } else {
                hi = nfl_pack2<_Float16>(x0, x1);
            }
            reinterpret_cast<unsigned(&)[4]>(out[ks + s][cb][0])[j / 2] = hi;
            {   // range tracking: after relu the halves are non-negative, so their bit patterns order like the values
                const unsigned mag = RELU ? hi : (hi & 0x7fff7fffu);
                asm("v_pk_max_u16 %0, %0, %1" : "+v"(ovf) : "v"(mag));
            }
            if (STASH) {        // the fp16 hi operand IS the stashed activation
                reinterpret_cast<unsigned(&)[4]>(tmp[cb])[j / 2] = hi;
                if (OP % 4 == 3) NFL_STREAM_STORE(tmp[cb], reinterpret_cast<h8*>(stash[cb] + (slot + s) * 1024));
                if (RELU) {     // relu mask of the pair for the dgrad kernel: bit 2*OP / 16 + 2*OP (nfl_plan.h)
                    unsigned on;
                    asm("v_pk_min_u16 %0, %1, %2" : "=v"(on) : "v"(hi), "s"(0x00010001u));
                    m32[cb] = OP == 0 ? on : ((on << (2 * OP)) | m32[cb]);
                    if (OP == 7) {
                        // mask words are grouped by four tiles (mw0 is a multiple of 4 for every layer): lane l keeps
                        // words 4g..4g+3 in 16 contiguous bytes, record layout [group][lane][4]
                        mq[cb][MSLOT] = m32[cb];              // MSLOT = mword & 3, known at compile time
                        if (MSLOT == 3) {
                            typedef unsigned nfl_mq4 __attribute__((ext_vector_type(4)));
                            const nfl_mq4 v = {mq[cb][0], mq[cb][1], mq[cb][2], mq[cb][3]};
                            NFL_STREAM_STORE(v, reinterpret_cast<nfl_mq4*>(mstash[cb] + (mword >> 2) * 1024));
                        }
                    }
                }
            }
        }
    }
    template <int K, int NK>
    NFL_DEV void step() {                      // the remaining pair-ops, spread evenly over the k-steps
        constexpr int R = 8 - NFL_EPI_EARLY;
        nfl_static_for<NFL_EPI_EARLY + (R * K) / NK, NFL_EPI_EARLY + (R * (K + 1)) / NK>([&](auto O) __attribute__((always_inline)) {
            pair<decltype(O)::value>();
        });
    }
    NFL_DEV void early() {
        nfl_static_for<0, NFL_EPI_EARLY>([&](auto O) __attribute__((always_inline)) { pair<decltype(O)::value>(); });
    }
    NFL_DEV void all() {
        nfl_static_for<0, 8>([&](auto O) __attribute__((always_inline)) { pair<decltype(O)::value>(); });
    }
};

// A dense layer of NRT row tiles reading inA[ksA0..+NKA) then inB[ksB0..+NKB), TPC tiles per
// ring chunk.  The epilogue of tile i-1 rides in the MFMA shadows of tile i.
// ZST (NFL_MODE_ZCACHE, a layer whose output starts at k-step 0): the epilogue also stores the fp32 pre-activations to
// zc[cb][f * zpad] (the appearance cache, nfl_appearance_cache).
template <int NP, int NCB, int NKA, int NKB, bool RELU, int NRT, int TPC, bool STASH, int LO = 0, int PRODS = 3, bool ZST = false, int NINA, int NINB, int NOUT, class Ring>
NFL_DEV void nfl_dense(Ring& ring, const float* bias_lds, int& rt, int h,
                       const h8 (&inA)[NINA][NCB][NP], int ksA0,
                       const h8 (&inB)[NINB][NCB][NP], int ksB0,
                       h8 (&out)[NOUT][NCB][NP], int out_ks0, char* const (&stash)[NCB], int slot0,
                       char* const (&mstash)[NCB], int mw0, float* const* zc = nullptr, int zpad = 0) {
    constexpr int NK = NKA + NKB;
    constexpr int NST = 2 * NCB * (LO != 0 ? 2 : 1);     // activation-stash stores of one tile's epilogue (the mask
                                                         // words go out once per four tiles: not counted, the wait is only stricter)
    unsigned mq[NCB][4];
    f16v acc[2][NCB];
    const char* wl = nullptr;
    auto getb = [&](auto K, int cb, int part) __attribute__((always_inline)) -> const h8& {
        constexpr int k = decltype(K)::value;
        if constexpr (k < NKA) return inA[ksA0 + k][cb][part];
        else return inB[ksB0 + k - NKA][cb][part];
    };
    nfl_static_for<0, NRT>([&](auto I) __attribute__((always_inline)) {
        constexpr int i = decltype(I)::value;
        // tile i-1 carried the stash stores of tile i-2's epilogue, issued after this chunk's pieces
        if (i % TPC == 0) wl = ring.template consume<(STASH && TPC == 1 && i >= 2) ? NST : 0>();
        constexpr int frag0 = (i % TPC) * NK;
        nfl_bias_init<NP, NCB>(acc[i & 1], bias_lds + (rt + i) * 32, h);
        if constexpr (i > 0) {
            NflActEpi<NP, NCB, RELU, STASH, NOUT, (i - 1) & 3, LO, ZST> epi{acc[(i - 1) & 1], out, out_ks0 + 2 * (i - 1), stash, slot0 + 2 * (i - 1), mstash, mw0 + i - 1, mq, ring.ovf, zc, zpad};
            nfl_tile_p<PRODS, NP, NCB, NK, frag0, h8>(acc[i & 1], wl, frag0, getb, epi, ring);
        } else {
            NflNoEpi epi;
            nfl_tile_p<PRODS, NP, NCB, NK, frag0, h8>(acc[i & 1], wl, frag0, getb, epi, ring);
        }
        // pieces the k-loop of this chunk did not get to
        if (i % TPC == TPC - 1 || i == NRT - 1) ring.template pieces<((i % TPC) + 1) * NK, Ring::MAXP>();
    });
    NflActEpi<NP, NCB, RELU, STASH, NOUT, (NRT - 1) & 3, LO, ZST> last{acc[(NRT - 1) & 1], out, out_ks0 + 2 * (NRT - 1), stash, slot0 + 2 * (NRT - 1), mstash, mw0 + NRT - 1, mq, ring.ovf, zc, zpad};
    last.all();
    rt += NRT;
}

// a single head tile (own chunk); the caller interprets the accumulator rows
template <int NP, int NCB, int NK, int PRODS = 3, int NIN, class Ring>
NFL_DEV void nfl_head(Ring& ring, const float* bias_lds, int& rt, int h,
                      const h8 (&in)[NIN][NCB][NP], int ks0, f16v (&acc)[NCB]) {
    const char* wl = ring.consume();
    nfl_bias_init<NP, NCB>(acc, bias_lds + rt * 32, h);
    auto getb = [&](auto K, int cb, int part) __attribute__((always_inline)) -> const h8& {
        return in[ks0 + decltype(K)::value][cb][part];
    };
    NflNoEpi epi;
    nfl_tile_p<PRODS, NP, NCB, NK, 0, h8>(acc, wl, 0, getb, epi, ring);
    ring.template pieces<NK, Ring::MAXP>();
    rt += 1;
}
