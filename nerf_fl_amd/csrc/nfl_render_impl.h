// nfl_render_impl.h -- the fused per-ray-chunk forward kernel.
//
// Replaces, for one pass (coarse or fine) of the reference's render_rays:
//   models/rendering.py:243-261  depth generation + o + d*z
//   models/nerf.py:19-32         positional encoding (in registers, never stored)
//   models/rendering.py:98-139   the point-chunk loop and all repeat/cat glue
//   models/nerf.py:153-212       the 8x256 MLP + heads   (MFMA, fp16 operands, fp32 accumulate)
//   models/rendering.py:141-226  alpha compositing       (wave scans, fp32)
//
// Mapping onto CDNA4
//   * workgroup = 4 waves, one per SIMD, up to 512 VGPR/AGPR each.  A workgroup owns a
//     contiguous range of rays and walks their samples in "segments" of 32 samples
//     (= one MFMA column block); a wave carries NCB segments at a time.
//   * the MLP itself -- transposed MFMA tiles, activations in registers, the weight ring, the
//     three-product arithmetic -- is the engine of nfl_mlp.h, shared with the dgrad kernel.
//   * compositing: per segment, an exclusive product scan of (1-alpha) over 32 lanes
//     gives the local transmittance; partial sums are linear in the incoming
//     transmittance, so segments (and tiles) of one ray are folded through a tiny LDS
//     record.  Nothing per-sample except the API's own (R,N) outputs is written.
#pragma once
#include "nfl_launch.h"
#include "nfl_mlp.h"

#define NFL_NST 20            // floats in a segment / ray compositing record
#define NFL_REC 32            // record stride (floats)

// ---------------------------------------------------------------------------------
// depths (reference models/rendering.py:243-259); every operation separately rounded
// ---------------------------------------------------------------------------------
template <class PA>
NFL_DEV float nfl_z_plain(const PA& a, float near, float far, int i) {
    const float s = a.d_lin[i];
    const float oms = 1.0f - s;
    if (!a.use_disp) return near * oms + far * s;
    return 1.0f / (1.0f / near * oms + 1.0f / far * s);
}
template <class PA>
NFL_DEV float nfl_z_at(const PA& a, int ray, float near, float far, int i) {
    const int N = a.n_samples;
    if (a.d_z) return a.d_z[(size_t)ray * N + i];
    float z = nfl_z_plain(a, near, far, i);
    if (a.perturb > 0.f) {
        const float zm = nfl_z_plain(a, near, far, i > 0 ? i - 1 : 0);
        const float zp = nfl_z_plain(a, near, far, i < N - 1 ? i + 1 : N - 1);
        const float upper = i < N - 1 ? 0.5f * (z + zp) : z;
        const float lower = i > 0 ? 0.5f * (zm + z) : z;
        const float pr = a.perturb * a.d_perturb_rand[(size_t)ray * N + i];
        z = lower + (upper - lower) * pr;
    }
    return z;
}

// ---------------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------------
template <int NSPLIT, int NCB, int NFX>
struct NflRenderCfg {
    static constexpr int NP = NSPLIT == 3 ? 2 : 1;
    static constexpr int NKP = (6 * NFX + 3 + 15) / 16;
    static constexpr int KSB = 1024 * NP;
    static constexpr int MAXKS = 16 + (NKP > 5 ? NKP : 5);
    static constexpr int SLOT = MAXKS * KSB;
    static constexpr int MAXP = (SLOT + 4095) / 4096;
    static constexpr int NSLOT = 4 * NCB;
    static constexpr int LDS_RING = 3 * SLOT;
    static constexpr int LDS_BIAS = NFL_MAX_RT * 32 * 4;
    static constexpr int LDS_REC = (NSLOT + 2) * NFL_REC * 4;
    static constexpr int LDS_CHK = (NFL_MAX_CHUNKS + 8 + 32 + 8) * 4; // chunk offsets + 32 positional-encoding weights + 4 loss partials
    static constexpr int LDS_BYTES = LDS_RING + LDS_BIAS + LDS_REC + LDS_CHK;
};

// Diagnostic build only (make diag, -DNFL_STAMPS): per-phase s_memtime totals of every wave, written to the buffer of
// nfl_stamps.h.  No stamp code exists in the product build.
#ifdef NFL_STAMPS
#include "nfl_stamps.h"
#define NFL_STAMP(i)                                                      \
    do {                                                                  \
        const unsigned long long t_now = __builtin_amdgcn_s_memtime();    \
        t_acc[i] += t_now - t_last;                                       \
        t_last = t_now;                                                   \
    } while (0)
#else
#define NFL_STAMP(i) do {} while (0)
#endif

#define NFL_LOSS_ON(a) ((a).d_loss_target != nullptr)
// the kernel's argument block, re-read from the kernarg segment where it is used (nfl_dev.h: nfl_kernarg)
typedef NflKernarg<RenderArgs> NflKArgs;
NFL_DEV NflKArgs nfl_kargs() { return nfl_kernarg<RenderArgs>(); }

// the camera of a ray-generating pass: in the kernarg segment (copied from nfl_pass_args::h_cam at launch) or, when the
// caller keeps it in device memory (d_cam: graph replays), behind that pointer -- read with scalar loads either way
typedef const __attribute__((address_space(4))) nfl_camera* NflKCam;
NFL_DEV NflKCam nfl_kcam(NflKArgs K) {
    return K->a.d_cam ? (NflKCam)(unsigned long long)K->a.d_cam : &K->cam;
}

template <int NSPLIT, int NCB, int NFX, int MODE>
__global__ __launch_bounds__(256, 1) void nfl_render_kernel(const RenderArgs A) {
    constexpr bool STASH = MODE == NFL_MODE_STASH || MODE == NFL_MODE_STASH2, EMBED = MODE == NFL_MODE_EMBED;
    constexpr bool ZC = MODE == NFL_MODE_ZCACHE;
    using C = NflRenderCfg<NSPLIT, NCB, NFX>;
    constexpr int NP = C::NP, NKP = C::NKP, NSLOT = C::NSLOT;
    constexpr int SMULT = MODE == NFL_MODE_STASH2 ? 2 : 1;                              // records per segment: hi (+ lo)
    constexpr int LO = MODE == NFL_MODE_STASH2 ? nfl_act_slots(NKP) * 1024 : 0;         // byte offset of the lo record
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // small tables first (so ds_read immediates reach them from one base register), ring last
    float* const bias_lds = reinterpret_cast<float*>(smem);
    float* const rec_lds = reinterpret_cast<float*>(smem + C::LDS_BIAS);   // [NSLOT] segment records, then carry[2]
    int* const chk_lds = reinterpret_cast<int*>(smem + C::LDS_BIAS + C::LDS_REC);
    float* const pw_lds = reinterpret_cast<float*>(chk_lds + NFL_MAX_CHUNKS + 8);   // [0,16): xyz freqs, [16,32): dir freqs
    float* const loss_lds = pw_lds + 32;                                            // [4] fused-loss partial sums of this workgroup

    const nfl_pass_args& a = A.a;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c = lane & 31;
    const int N = a.n_samples, SPR = A.spr;

    const int ray0 = blockIdx.x * A.rays_per_wg;
    int ray1 = ray0 + A.rays_per_wg;
    if (ray1 > a.n_rays) ray1 = a.n_rays;
    if (ray0 >= ray1) return;
    const int seg_end = (ray1 - ray0) * SPR;
    const int ntiles = (seg_end + NSLOT - 1) / NSLOT;

    {   // bias table and chunk offsets -> LDS (LDS reads keep the VMEM queue free for the ring)
        const float* bg = reinterpret_cast<const float*>(A.packed + A.bias_off);
        for (int i = tid; i < A.n_rt * 32; i += 256) bias_lds[i] = bg[i];
        for (int i = tid; i <= A.n_chunks; i += 256) chk_lds[i] = A.plan->chunk_off[i];
        if (tid < 16) pw_lds[tid] = (a.d_pe_w_xyz && tid < A.nfx_rt) ? a.d_pe_w_xyz[tid] : 1.f;
        else if (tid < 32) pw_lds[tid] = (a.d_pe_w_dir && tid - 16 < A.ndir_rt) ? a.d_pe_w_dir[tid - 16] : 1.f;
        else if (tid < 36) loss_lds[tid - 32] = 0.f;
    }
    __syncthreads();

    NflRing<C::SLOT, C::MAXP> ring;
    ring.gsrc = A.packed;
    ring.chunk_off = chk_lds;
    ring.lds = smem + C::LDS_BIAS + C::LDS_REC + C::LDS_CHK;
    ring.n_chunks = A.n_chunks;
    ring.c_issue = 0;
    ring.s_issue = 0;
    ring.s_read = 0;
    ring.wave = wave;
    ring.lane = lane;
    ring.prime();

#ifdef NFL_STAMPS
    unsigned long long t_acc[NFL_NSTAMP] = {};
    unsigned long long t_last = __builtin_amdgcn_s_memtime();
#endif
    for (int tile = 0; tile < ntiles; ++tile) {
        NflKArgs K = nfl_kargs();          // ray set-up: arguments loaded here, not carried through the MLP
        // ------------------------------------------------------------ per-sample setup
        int s_ray[NCB], s_idx[NCB];
        bool s_ok[NCB];
        float s_z[NCB], s_dl[NCB];
        h8 P[NKP][NCB][NP];
        h8 X[16][NCB][NP], Y[16][NCB][NP];
        char* st[NCB];        // this lane's slice of the segment's activation record (training forward) or null
        char* mst[NCB];       // ... and of its relu-mask record
        float* zc[NCB];       // NFL_MODE_ZCACHE: the sample column of the segment's ray in the appearance cache
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int g = tile * NSLOT + wave * NCB + cb;        // segment index inside this workgroup
            const bool seg_ok = g < seg_end;
            const int gg = seg_ok ? g : seg_end - 1;
            const int ray = ray0 + gg / SPR;
            const int i = (gg % SPR) * 32 + c;
            const bool ok = seg_ok && i < N;
            const int ii = i < N ? i : N - 1;
            if constexpr (EMBED) {
                // point b = 32 * segment + c of an (n_points, row) matrix [xyz enc | dir enc (+a) | tau]
                const int b = ray * 32 + c;
                const bool pok = seg_ok && b < K->n_points;
                const float* xr = K->a.d_embedded + (size_t)(b < K->n_points ? b : K->n_points - 1) * K->emb_stride;
                st[cb] = nullptr;
                mst[cb] = nullptr;
                s_ray[cb] = ray;
                s_idx[cb] = c;
                s_ok[cb] = pok;
                s_z[cb] = 0.f;
                s_dl[cb] = 0.f;
#pragma unroll
                for (int ks = 0; ks < NKP; ++ks) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int f = 16 * ks + 8 * h + j;
                        v[j] = f < K->cx ? xr[f] : 0.f;
                    }
                    nfl_split8<NP>(v, P[ks][cb]);
                }
                continue;
            }
            f4v r0, r1;
            if (K->gen_rays) {
                const NflKCam cam = nfl_kcam(K);
                nfl_cam_ray(*cam, cam->pix0 + ray, r0, r1);
            } else
            {
                const float* rp = K->a.d_rays + (size_t)ray * 8;
                r0 = *reinterpret_cast<const f4v*>(rp);
                r1 = *reinterpret_cast<const f4v*>(rp + 4);
            }
            const float near = r1[2], far = r1[3];
            const float z = nfl_z_at(K->a, ray, near, far, ii);
            const float zn = ii + 1 < N ? nfl_z_at(K->a, ray, near, far, ii + 1) : z;
            // padded segments recompute (and re-store) the last real one: identical bytes, no branch
            // stash k-step image = [sample c][lane half h][8 values]: a sample's 16 features are 32 contiguous
            // bytes, which makes the weight-gradient kernel's transposed LDS reads conflict-free
            st[cb] = STASH ? K->a.d_act_stash + ((size_t)(ray0 * SPR + gg) * nfl_act_rec(NKP, SMULT)) * 1024 + (2 * c + h) * 16
                           : nullptr;
            mst[cb] = STASH ? K->a.d_act_stash + nfl_msk_offset((size_t)K->a.n_rays * SPR, NKP, SMULT)
                                  + (size_t)(ray0 * SPR + gg) * (NFL_MSK_WORDS * 256) + lane * 16
                            : nullptr;
            s_ray[cb] = ray;
            s_idx[cb] = ii;
            s_ok[cb] = ok;
            // padded samples (ii clamped to N - 1) re-store the last real sample's values: identical bytes, no branch
            zc[cb] = ZC ? K->zcache + (size_t)ray * 128 * K->zpad + ii : nullptr;
            s_z[cb] = z;
            s_dl[cb] = ii + 1 < N ? zn - z : 1e2f;
            if (K->a.d_z_out && ok && h == 0) K->a.d_z_out[(size_t)ray * N + ii] = z;
            float raw[3], th[3], tl[3];
            raw[0] = r0[0] + r0[3] * z;
            raw[1] = r0[1] + r1[0] * z;
            raw[2] = r0[2] + r1[1] * z;
#pragma unroll
            for (int k = 0; k < 3; ++k) nfl_turns(raw[k], th[k], tl[k]);
#pragma unroll
            for (int ks = 0; ks < NKP; ++ks) {
                nfl_pe_kstep<NFX, NP, LO>(ks, h, raw, th, tl, pw_lds, P[ks][cb], STASH ? st[cb] + ks * 1024 : nullptr);
                __builtin_amdgcn_sched_barrier(0);      // bound the register pressure of the encoder
            }
        }

        // ------------------------------------------------------------ the field
        K = nfl_kargs();
        int rt = 0;
        // raw head outputs of sample c (lane half 0); extracted at once so the 16-register
        // accumulator tiles die immediately
        float o_sig[NCB], o_rgb[NCB][3], o_tr[NCB][5];
        NFL_STAMP(0);
        nfl_dense<NP, NCB, NKP, 0, true, 8, 2, STASH, LO, NFL_PRODS[NFL_P_IDX_L1]>(ring, bias_lds, rt, h, P, 0, P, 0, X, 0, st, nfl_act_h(NKP, 1), mst, nfl_msk_h(1));       // L1
        NFL_STAMP(1);
        nfl_dense<NP, NCB, 16, 0, true, 8, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_L2]>(ring, bias_lds, rt, h, X, 0, X, 0, Y, 0, st, nfl_act_h(NKP, 2), mst, nfl_msk_h(2));        // L2
        NFL_STAMP(2);
        nfl_dense<NP, NCB, 16, 0, true, 8, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_L3]>(ring, bias_lds, rt, h, Y, 0, Y, 0, X, 0, st, nfl_act_h(NKP, 3), mst, nfl_msk_h(3));        // L3
        NFL_STAMP(3);
        nfl_dense<NP, NCB, 16, 0, true, 8, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_L4]>(ring, bias_lds, rt, h, X, 0, X, 0, Y, 0, st, nfl_act_h(NKP, 4), mst, nfl_msk_h(4));        // L4
        NFL_STAMP(4);
        nfl_dense<NP, NCB, NKP, 16, true, 8, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_L5]>(ring, bias_lds, rt, h, P, 0, Y, 0, X, 0, st, nfl_act_h(NKP, 5), mst, nfl_msk_h(5));      // L5 (skip)
        NFL_STAMP(5);
        nfl_dense<NP, NCB, 16, 0, true, 8, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_L6]>(ring, bias_lds, rt, h, X, 0, X, 0, Y, 0, st, nfl_act_h(NKP, 6), mst, nfl_msk_h(6));        // L6
        NFL_STAMP(6);
        nfl_dense<NP, NCB, 16, 0, true, 8, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_L7]>(ring, bias_lds, rt, h, Y, 0, Y, 0, X, 0, st, nfl_act_h(NKP, 7), mst, nfl_msk_h(7));        // L7
        NFL_STAMP(7);
        nfl_dense<NP, NCB, 16, 0, true, 8, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_L8]>(ring, bias_lds, rt, h, X, 0, X, 0, Y, 0, st, nfl_act_h(NKP, 8), mst, nfl_msk_h(8));        // L8
        NFL_STAMP(8);
        {
            f16v hacc[NCB];
            nfl_head<NP, NCB, 16, NFL_PRODS[NFL_P_IDX_SIG]>(ring, bias_lds, rt, h, Y, 0, hacc);   // sigma
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) o_sig[cb] = hacc[cb][0];
        }
        NFL_STAMP(9);
        K = nfl_kargs();           // head-side arguments (view directions, latents): loaded after the trunk
        if (!K->a.sigma_only) {
            // xyz_encoding_final has no tiles: it is linear and folded into the 256 columns of dir_encoding.0 /
            // transient_encoding.0 that read its output (nfl_plan.cpp), so both read h8 (Y) directly and write into X
            NFL_STAMP(10);
            {
                h8 D[5][NCB][NP];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    if constexpr (EMBED) {
                        const int b = s_ray[cb] * 32 + s_idx[cb];
                        const float* xr = K->a.d_embedded + (size_t)(b < K->n_points ? b : K->n_points - 1) * K->emb_stride
                                          + K->cx;
#pragma unroll
                        for (int ks = 0; ks < 5; ++ks) {
                            if (ks >= 2 && !K->has_a) break;
                            float v[8];
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                const int f = 16 * (ks < 2 ? ks : ks - 2) + 8 * h + j;
                                v[j] = ks < 2 ? (f < K->cd ? xr[f] : 0.f) : (f < K->n_a ? xr[K->cd + f] : 0.f);
                            }
                            nfl_split8<NP>(v, D[ks][cb]);
                        }
                        continue;
                    }
                    float raw[3], th[3], tl[3];
                    if (K->gen_rays && !K->a.d_view_dir) {
                        f4v g0, g1;
                        const NflKCam cam = nfl_kcam(K);
                        nfl_cam_ray(*cam, cam->pix0 + s_ray[cb], g0, g1);
                        raw[0] = g0[3];
                        raw[1] = g1[0];
                        raw[2] = g1[1];
                    } else {
                        const float* dp = K->a.d_view_dir ? K->a.d_view_dir + (size_t)s_ray[cb] * 3
                                                       : K->a.d_rays + (size_t)s_ray[cb] * 8 + 3;
#pragma unroll
                        for (int k = 0; k < 3; ++k) raw[k] = dp[k];
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) nfl_turns(raw[k], th[k], tl[k]);
                    char* sd = STASH ? st[cb] + nfl_act_d(NKP) * 1024 : nullptr;
                    nfl_pe_kstep<4, NP, LO>(0, h, raw, th, tl, pw_lds + 16, D[0][cb], sd);
                    __builtin_amdgcn_sched_barrier(0);
                    nfl_pe_kstep<4, NP, LO>(1, h, raw, th, tl, pw_lds + 16, D[1][cb], STASH ? sd + 1024 : nullptr);
                    __builtin_amdgcn_sched_barrier(0);
                    if (K->has_a) {
                        const int na = K->n_a;
                        const float* ap = K->a.d_a_emb + (size_t)s_ray[cb] * na + 8 * h;
#pragma unroll
                        for (int ks = 0; ks < 3; ++ks) {
                            float v[8];
                            if (na == 48) {          // the reference's default width: rows are 16-byte aligned
                                const f4v v0 = *reinterpret_cast<const f4v*>(ap + 16 * ks);
                                const f4v v1 = *reinterpret_cast<const f4v*>(ap + 16 * ks + 4);
                                v[0] = v0[0]; v[1] = v0[1]; v[2] = v0[2]; v[3] = v0[3];
                                v[4] = v1[0]; v[5] = v1[1]; v[6] = v1[2]; v[7] = v1[3];
                            } else {                  // narrower code: scalar loads, zeros beyond its width
#pragma unroll
                                for (int j = 0; j < 8; ++j) v[j] = 16 * ks + 8 * h + j < na ? ap[16 * ks + j] : 0.f;
                            }
                            nfl_split8<NP>(v, D[2 + ks][cb]);
                            if (STASH) nfl_stash8<LO>(v, sd + (2 + ks) * 1024);
                        }
                    }
                }
                NFL_STAMP(11);
                if (K->has_a)
                    nfl_dense<NP, NCB, 16, 5, true, 4, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_DIR], ZC>(ring, bias_lds, rt, h, Y, 0, D, 0, X, 0, st, nfl_act_dirh(NKP), mst, nfl_msk_dirh(), zc, ZC ? K->zpad : 0);
                else
                    nfl_dense<NP, NCB, 16, 2, true, 4, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_DIR], ZC>(ring, bias_lds, rt, h, Y, 0, D, 0, X, 0, st, nfl_act_dirh(NKP), mst, nfl_msk_dirh(), zc, ZC ? K->zpad : 0);
            }
            NFL_STAMP(12);
            {
                f16v hacc[NCB];
                nfl_head<NP, NCB, 8, NFL_PRODS[NFL_P_IDX_RGB]>(ring, bias_lds, rt, h, X, 0, hacc);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    o_rgb[cb][0] = hacc[cb][0];
                    o_rgb[cb][1] = hacc[cb][1];
                    o_rgb[cb][2] = hacc[cb][2];
                }
            }
            NFL_STAMP(13);
            K = nfl_kargs();
            if (K->use_t) {
                h8 T[1][NCB][NP];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const int tb = s_ray[cb] * 32 + s_idx[cb];
                    const float* tp = EMBED ? K->a.d_embedded + (size_t)(tb < K->n_points ? tb : K->n_points - 1) * K->emb_stride
                                                  + K->cx + K->cd + (K->has_a ? K->n_a : 0) + 8 * h
                                            : K->a.d_t_emb + (size_t)s_ray[cb] * K->n_tau + 8 * h;
                    float v[8];
                    if (EMBED || K->n_tau != 16) {  // rows of the encoded matrix / of a narrower code are not 16-byte aligned
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = 8 * h + j < K->n_tau ? tp[j] : 0.f;
                    } else {
                        const f4v v0 = *reinterpret_cast<const f4v*>(tp);
                        const f4v v1 = *reinterpret_cast<const f4v*>(tp + 4);
                        v[0] = v0[0]; v[1] = v0[1]; v[2] = v0[2]; v[3] = v0[3];
                        v[4] = v1[0]; v[5] = v1[1]; v[6] = v1[2]; v[7] = v1[3];
                    }
                    nfl_split8<NP>(v, T[0][cb]);
                    if (STASH) nfl_stash8<LO>(v, st[cb] + nfl_act_tau(NKP) * 1024);
                }
                nfl_dense<NP, NCB, 16, 1, true, 4, 1, STASH, LO, NFL_PRODS[NFL_P_IDX_T1]>(ring, bias_lds, rt, h, Y, 0, T, 0, X, 8, st, nfl_act_g(NKP, 1), mst, nfl_msk_g(1));
                nfl_dense<NP, NCB, 8, 0, true, 4, 2, STASH, LO, NFL_PRODS[NFL_P_IDX_T2]>(ring, bias_lds, rt, h, X, 8, X, 8, X, 0, st, nfl_act_g(NKP, 2), mst, nfl_msk_g(2));
                nfl_dense<NP, NCB, 8, 0, true, 4, 2, STASH, LO, NFL_PRODS[NFL_P_IDX_T3]>(ring, bias_lds, rt, h, X, 0, X, 0, X, 8, st, nfl_act_g(NKP, 3), mst, nfl_msk_g(3));
                nfl_dense<NP, NCB, 8, 0, true, 4, 2, STASH, LO, NFL_PRODS[NFL_P_IDX_T4]>(ring, bias_lds, rt, h, X, 8, X, 8, X, 0, st, nfl_act_g(NKP, 4), mst, nfl_msk_g(4));
                f16v hacc[NCB];
                nfl_head<NP, NCB, 8, NFL_PRODS[NFL_P_IDX_THEAD]>(ring, bias_lds, rt, h, X, 0, hacc);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) o_tr[cb][k] = hacc[cb][k];     // row 8 (beta) = register 4
                }
            }
        }

        NFL_STAMP(14);
        // ------------------------------------------------------------ compositing, phase 1
        K = nfl_kargs();
        // (reference models/rendering.py:141-226).  Lanes 0..31 of each half own sample c.
        float w_loc[NCB], sig_t[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const bool ok = s_ok[cb];
            const float z = s_z[cb], dl = s_dl[cb];
            const size_t sidx = (size_t)s_ray[cb] * N + s_idx[cb];
            const float sg = nfl_softplus(o_sig[cb]);
            float cr = 0.f, cg = 0.f, cbl = 0.f, tr = 0.f, tg = 0.f, tb = 0.f, sgt = 0.f, bt = 0.f;
            if (!K->a.sigma_only) {
                cr = nfl_sigmoid(o_rgb[cb][0]);
                cg = nfl_sigmoid(o_rgb[cb][1]);
                cbl = nfl_sigmoid(o_rgb[cb][2]);
            }
            if (K->use_t) {
                sgt = nfl_softplus(o_tr[cb][0]);
                tr = nfl_sigmoid(o_tr[cb][1]);
                tg = nfl_sigmoid(o_tr[cb][2]);
                tb = nfl_sigmoid(o_tr[cb][3]);
                bt = nfl_softplus(o_tr[cb][4]);
            }
            if (K->a.d_field_raw && ok && h == 0) {
                float* fr = K->a.d_field_raw + sidx * 9;
                fr[0] = cr; fr[1] = cg; fr[2] = cbl; fr[3] = sg;
                fr[4] = tr; fr[5] = tg; fr[6] = tb; fr[7] = sgt; fr[8] = bt;
            }
            if constexpr (EMBED) continue;          // the field outputs are the result; nothing to composite
            float alpha, a_s = 0.f, a_t = 0.f;
            if (K->use_t) {
                a_s = 1.f - expf(-dl * sg);
                a_t = 1.f - expf(-dl * sgt);
                alpha = 1.f - expf(-dl * (sg + sgt));
            } else {
                const float nz = K->a.d_noise ? K->a.d_noise[sidx] * K->a.noise_std : 0.f;
                alpha = 1.f - expf(-dl * fmaxf(sg + nz, 0.f));
            }
            if (!ok) { alpha = 0.f; a_s = 0.f; a_t = 0.f; }
            // exclusive product scans of (1 - alpha) over the 32 samples of the segment
            float inc[3] = {1.f - alpha, 1.f - a_s, 1.f - a_t};
#pragma unroll
            for (int d = 1; d < 32; d <<= 1)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float n = __shfl_up(inc[k], d, 32);
                    if (c >= d) inc[k] *= n;
                }
            float exc[3], prod[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float e = __shfl_up(inc[k], 1, 32);
                exc[k] = c == 0 ? 1.f : e;
                prod[k] = __shfl(inc[k], 31, 32);
            }
            const float w = alpha * exc[0];
            w_loc[cb] = w;
            sig_t[cb] = sgt;
            float rec[NFL_NST];
            rec[0] = prod[0]; rec[1] = prod[1]; rec[2] = prod[2];
            rec[3] = nfl_sum32(w);
            rec[11] = nfl_sum32(w * z);
            if (K->use_t) {
                const float ws = a_s * exc[0], wt = a_t * exc[0];
                rec[4] = nfl_sum32(ws * cr); rec[5] = nfl_sum32(ws * cg); rec[6] = nfl_sum32(ws * cbl);
                rec[7] = nfl_sum32(wt * tr); rec[8] = nfl_sum32(wt * tg); rec[9] = nfl_sum32(wt * tb);
                rec[10] = nfl_sum32(wt * bt);
                if (K->a.test_extras) {
                    const float ws1 = a_s * exc[1], wt1 = a_t * exc[2];
                    rec[12] = nfl_sum32(ws1 * cr); rec[13] = nfl_sum32(ws1 * cg); rec[14] = nfl_sum32(ws1 * cbl);
                    rec[15] = nfl_sum32(ws1 * z);
                    rec[16] = nfl_sum32(wt1 * tr); rec[17] = nfl_sum32(wt1 * tg); rec[18] = nfl_sum32(wt1 * tb);
                    rec[19] = nfl_sum32(wt1 * z);
                } else {
#pragma unroll
                    for (int k = 12; k < NFL_NST; ++k) rec[k] = 0.f;
                    if (NFL_LOSS_ON(K->a)) rec[19] = nfl_sum32(ok ? sgt : 0.f);    // s_l: plain sum of the transient densities
                }
            } else {
                rec[4] = nfl_sum32(w * cr); rec[5] = nfl_sum32(w * cg); rec[6] = nfl_sum32(w * cbl);
#pragma unroll
                for (int k = 7; k < NFL_NST; ++k) if (k != 11) rec[k] = 0.f;
            }
            if (lane == 0) {
                float* dst = rec_lds + (wave * NCB + cb) * NFL_REC;
#pragma unroll
                for (int k = 0; k < NFL_NST; ++k) dst[k] = rec[k];
            }
        }
        if constexpr (EMBED) continue;
        NFL_STAMP(15);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        NFL_STAMP(16);

        // ------------------------------------------------------------ compositing, phase 2
        K = nfl_kargs();
        // fold the segments of each ray in order; lane k (< NFL_NST) carries record entry k
        const float* carry_in = rec_lds + (NSLOT + (tile & 1)) * NFL_REC;
        float* carry_out = rec_lds + (NSLOT + ((tile + 1) & 1)) * NFL_REC;
        const int kk = lane < NFL_NST ? lane : 0;
        const int chain = kk < 3 ? kk : (kk < 12 ? 0 : (kk < 16 ? 1 : 2));
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int m = wave * NCB + cb;
            const int g = tile * NSLOT + m;
            if (g >= seg_end) continue;                         // wave-uniform
            const int q = g % SPR, ray = ray0 + g / SPR;
            int m0 = m - q;
            float t_in = 1.f;        // transmittance (chain 0) entering my segment: every lane
            float t_run = 1.f;       // running product of my chain
            float acc = 0.f;
            if (m0 < 0) {
                t_in = carry_in[0];
                t_run = carry_in[chain];
                acc = kk < 3 ? 0.f : carry_in[kk];
                m0 = 0;
            }
            const bool plain = NFL_LOSS_ON(K->a) && kk == 19;      // entry 19 with the fused loss: an unweighted sum (s_l)
            for (int mm = m0; mm <= m; ++mm) {
                const float* r = rec_lds + mm * NFL_REC;
                if (mm < m) t_in *= r[0];
                acc += (plain ? 1.f : t_run) * r[kk];
                t_run *= r[chain];
            }
            // per-sample outputs
            if (s_ok[cb] && h == 0) {
                const size_t sidx = (size_t)ray * N + s_idx[cb];
                if (K->a.d_weights) K->a.d_weights[sidx] = w_loc[cb] * t_in;
                if (K->use_t && K->a.d_transient_sigmas) K->a.d_transient_sigmas[sidx] = sig_t[cb];
            }
            if (q == SPR - 1) {
                // ray complete: lane k holds the composited quantity k
                const float wsum = __shfl(acc, 3);
                if (K->a.d_status) {       // fp16 operand range exceeded somewhere on this ray (header: d_status)
                    const bool bad = lane < NFL_NST && !(fabsf(acc) <= 3.0e38f);
                    if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(K->a.d_status, NFL_STATUS_NONFINITE);
                }
                const float white = K->a.white_back ? 1.f - wsum : 0.f;
                const float stat = acc + white;                  // meaningful on lanes 4..6 and 12..14
                const float tran = __shfl(acc, (lane + 3) & 63); // lanes 4..6 read 7..9
                if (lane == 3 && K->a.d_opacity) K->a.d_opacity[ray] = acc;
                if (lane == 11 && K->a.d_depth) K->a.d_depth[ray] = acc;
                if (lane >= 4 && lane < 7) {
                    if (K->use_t) {
                        if (K->a.d_rgb_static) K->a.d_rgb_static[ray * 3 + lane - 4] = stat;
                        if (K->a.d_rgb_transient) K->a.d_rgb_transient[ray * 3 + lane - 4] = tran;
                        if (K->a.d_rgb) K->a.d_rgb[ray * 3 + lane - 4] = stat + tran;
                    } else if (K->a.d_rgb) {
                        K->a.d_rgb[ray * 3 + lane - 4] = stat;
                    }
                }
                if (NFL_LOSS_ON(K->a)) {
                    // NerfWLoss of this ray (reference losses.py:35-50) and its backward seeds
                    const bool ch = lane >= 4 && lane < 7;
                    const float tgt = ch ? K->a.d_loss_target[ray * 3 + lane - 4] : 0.f;
                    const float diff = ch ? (K->use_t ? stat + tran : stat) - tgt : 0.f;
                    const float sq = diff * diff;
                    const float sum3 = __shfl(sq, 4) + __shfl(sq, 5) + __shfl(sq, 6);
                    const float rinv = 1.f / (float)K->a.n_rays, c0 = K->a.loss_coef;
                    float l0, l1 = 0.f, l2 = 0.f, g_rgb;
                    if (K->use_t) {
                        const float beta = __shfl(acc, 10) + K->beta_min;
                        const float ib2 = 1.f / (beta * beta);
                        l0 = c0 * sum3 * 0.5f * ib2 * rinv * (1.f / 3.f);
                        l1 = c0 * (3.f + logf(beta)) * rinv;
                        l2 = c0 * K->a.lambda_u * __shfl(acc, 19) * rinv / (float)N;
                        g_rgb = c0 * diff * ib2 * rinv * (1.f / 3.f);
                        if (lane == 10 && K->a.d_seed_beta)
                            K->a.d_seed_beta[ray] = c0 * rinv * (1.f / beta - sum3 * ib2 / beta * (1.f / 3.f));
                    } else {
                        l0 = c0 * 0.5f * sum3 * rinv * (1.f / 3.f);
                        g_rgb = c0 * diff * rinv * (1.f / 3.f);
                    }
                    if (ch && K->a.d_seed_rgb) K->a.d_seed_rgb[ray * 3 + lane - 4] = g_rgb;
                    if (lane == 0) {
                        atomicAdd(loss_lds + K->a.loss_slot, l0);
                        if (K->use_t) {
                            atomicAdd(loss_lds + 2, l1);
                            atomicAdd(loss_lds + 3, l2);
                        }
                    }
                }
                if (K->use_t) {
                    if (lane == 10 && K->a.d_beta) K->a.d_beta[ray] = acc + K->beta_min;
                    if (K->a.test_extras) {
                        if (lane >= 12 && lane < 15 && K->a.d_rgb_static_only) K->a.d_rgb_static_only[ray * 3 + lane - 12] = stat;
                        if (lane == 15 && K->a.d_depth_static_only) K->a.d_depth_static_only[ray] = acc;
                        if (lane >= 16 && lane < 19 && K->a.d_rgb_transient_only) K->a.d_rgb_transient_only[ray * 3 + lane - 16] = acc;
                        if (lane == 19 && K->a.d_depth_transient_only) K->a.d_depth_transient_only[ray] = acc;
                    }
                }
            } else if (m == NSLOT - 1) {
                // the ray continues in the next tile: hand its state over
                if (lane < NFL_NST) carry_out[lane] = lane < 3 ? t_run : acc;
            }
        }
        // the next tile's first consume() barrier orders these LDS reads/writes
        // against the next phase-1 record writes (>= 70 barriers away).
        NFL_STAMP(17);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the two prefetched chunks before exit
    NflKArgs K = nfl_kargs();
    if (NFL_LOSS_ON(K->a)) {   // one flush of this workgroup's loss partials
        __syncthreads();
        if (tid < 4 && K->a.d_losses && loss_lds[tid] != 0.f) atomicAdd(K->a.d_losses + tid, loss_lds[tid]);
    }
    if (K->a.d_status) {      // an activation beyond fp16's range: the conversion gave inf (0x7c00) -- header, d_status
        const bool bad = (ring.ovf & 0xffffu) >= 0x7c00u || (ring.ovf >> 16) >= 0x7c00u;
        if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(K->a.d_status, NFL_STATUS_RANGE);
    }
#ifdef NFL_STAMPS
    NFL_STAMP(18);
    t_acc[14] = ring.t_wait;
    t_acc[19] = ring.t_bar;
    if (lane == 0 && blockIdx.x < 1024)
        for (int i = 0; i < NFL_NSTAMP; ++i) nfl_stamp_buf[(blockIdx.x * 4 + wave) * NFL_NSTAMP + i] = t_acc[i];
#endif
}

// Host side: nfl_launch.cpp decides everything (mode, argument block, grid); here the mode picks the instantiation, which
// sets its LDS attribute and launches.  zcache != null: the cache-building pass of nfl_appearance_cache.
template <int NSPLIT, int NCB, int NFX, int MODE>
static int nfl_launch_render_t(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_pass_args* args,
                               hipStream_t stream, float* zcache, int zpad) {
    using C = NflRenderCfg<NSPLIT, NCB, NFX>;
    const NflDevice dev = nfl_device();
    RenderArgs A;
    int grid;
    nfl_render_fill(hp, d_plan, d_packed, args, MODE, zcache, zpad, dev.n_cu, C::NSLOT, &A, &grid);
    if (nfl_lds_attr<&nfl_render_kernel<NSPLIT, NCB, NFX, MODE>>(dev.ordinal, C::LDS_BYTES) != NFL_OK) return NFL_ENODEV;
    hipLaunchKernelGGL((nfl_render_kernel<NSPLIT, NCB, NFX, MODE>), dim3(grid), dim3(256), C::LDS_BYTES, stream, A);
    return hipGetLastError() == hipSuccess ? NFL_OK : NFL_ELAUNCH;
}
template <int NSPLIT, int NCB, int NFX>
static int nfl_launch_render(const NflPlan* hp, const void* d_plan, const void* d_packed, const nfl_pass_args* args,
                             hipStream_t stream, float* zcache = nullptr, int zpad = 0) {
    const int mode = nfl_render_mode(hp, args, zcache != nullptr);
#define NFL_LAUNCH_MODE(M) \
    if (mode == M) return nfl_launch_render_t<NSPLIT, NCB, NFX, M>(hp, d_plan, d_packed, args, stream, zcache, zpad)
#ifdef NFL_DIAG_INFERENCE_ONLY       // sweep builds (nfl_diag.h): only the inference instantiation is compiled
    constexpr bool ALL = false;
#else
    constexpr bool ALL = true;
#endif
    // STASH, STASH2 and ZCACHE are modes of the three-product kernels alone (nfl_render_mode) and instantiated only there;
    // the order is the one the kernels have always been emitted in
    if constexpr (ALL) NFL_LAUNCH_MODE(NFL_MODE_EMBED);
    if constexpr (ALL && NSPLIT == 3) NFL_LAUNCH_MODE(NFL_MODE_STASH2);
    if constexpr (ALL && NSPLIT == 3) NFL_LAUNCH_MODE(NFL_MODE_STASH);
    NFL_LAUNCH_MODE(NFL_MODE_RENDER);
    if constexpr (ALL && NSPLIT == 3) NFL_LAUNCH_MODE(NFL_MODE_ZCACHE);
#undef NFL_LAUNCH_MODE
    return NFL_EINVAL;
}
