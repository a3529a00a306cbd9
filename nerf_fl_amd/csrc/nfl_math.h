// nfl_math.h -- the scalar device math every kernel family shares, so that each of them produces the same bits: the ray of
// a pixel, the activations, the encoder's sine (exact two-float x / 2 pi + minimax polynomial) and one encoded feature, and
// the fp32 -> fp16 pack / hi + lo split of an MFMA operand.  A leaf: nothing here knows the plan, the weight ring or a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nerf_fl_amd.h"
#include "nfl_macros.h"

typedef float f4v __attribute__((ext_vector_type(4)));

// ray of pixel p of a frame (reference datasets/ray_utils.py:5-55); the ONE implementation behind nfl_gen_rays and the
// render kernel's camera prologue, so that both produce the same bits
template <class Cam>
NFL_DEV void nfl_cam_ray(const Cam& c, long long p, f4v& r0, f4v& r1) {
    const float i = (float)(p % c.width), j = (float)(p / c.width);
    const float dx = (i - c.cx) / c.fx, dy = -(j - c.cy) / c.fy, dz = -1.f;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = dx * c.c2w[4 * r] + dy * c.c2w[4 * r + 1] + dz * c.c2w[4 * r + 2];
    const float n = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    r0 = f4v{c.c2w[3], c.c2w[7], c.c2w[11], d[0] / n};
    r1 = f4v{d[1] / n, d[2] / n, c.near, c.far};
}

NFL_DEV float nfl_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // torch default beta=1, threshold=20
NFL_DEV float nfl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// sin(2*pi*r) for r in about [-1, 2]; abs error < 2e-7 (minimax odd polynomial on [-1/4,1/4])
NFL_DEV float nfl_sin_rev(float r) {
    r = r - rintf(r);                                   // [-1/2, 1/2]
    float a = fabsf(r);
    a = a > 0.25f ? 0.5f - a : a;                       // sin(pi - t) = sin(t)
    a = copysignf(a, r);
    const float a2 = a * a;
    float p = 3.953670604e+01f;
    p = __builtin_fmaf(p, a2, -7.654978229e+01f);
    p = __builtin_fmaf(p, a2, 8.160100407e+01f);
    p = __builtin_fmaf(p, a2, -4.134165503e+01f);
    p = __builtin_fmaf(p, a2, 6.283185160e+00f);
    return a * p;
}

// x / (2*pi) as an unevaluated sum th + tl (exact to ~2^-45 relative)
NFL_DEV void nfl_turns(float x, float& th, float& tl) {
    const float C_HI = 0.15915493667125702f;            // fl32(1/(2 pi))
    const float C_LO = 6.4206382432985265e-09f;         // 1/(2 pi) - C_HI
    th = x * C_HI;
    const float e = __builtin_fmaf(x, C_HI, -th);
    tl = __builtin_fmaf(x, C_LO, e);
}

// feature f of [x | sin(2^0 x) | cos(2^0 x) | sin(2^1 x) ...] (3 columns per block);
// f, N compile-time after unrolling, coordinates as turns (th, tl) + raw value
// `pw` = per-frequency weights (LDS, broadcast reads): all ones, or the BARF coarse-to-fine weights
// of reference models/nerf.py:47-75 (computed on the host exactly as the reference does)
template <int N>
NFL_DEV float nfl_pe_feature(int f, const float (&raw)[3], const float (&th)[3], const float (&tl)[3], const float* pw) {
    if (f < 3) return raw[f];
    if (f >= 6 * N + 3) return 0.f;
    const int g = f - 3, k = g / 6, rem = g % 6, t = rem / 3, c = rem % 3;
    const float sc = (float)(1 << k);
    float r = __builtin_amdgcn_fractf(th[c] * sc) + tl[c] * sc;      // 2^k scaling is exact
    if (t) r += 0.25f;                                                // cos(y) = sin(y + pi/2)
    return pw[k] * nfl_sin_rev(r);
}

// relu on the bit pattern: one v_max_i32, and unlike v_max_f32 / v_med3_f32 it needs no canonicalising
// v_max_f32 x,x in front (negative floats are negative integers; -0 and negative NaNs become +0)
NFL_DEV float nfl_relu(float x) {
    int b = __builtin_bit_cast(int, x);
    b = b > 0 ? b : 0;
    return __builtin_bit_cast(float, b);
}
template <class E>
NFL_DEV unsigned nfl_pack2(float a, float b) {      // v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 (round to nearest even)
    typedef E e2v __attribute__((ext_vector_type(2)));
    e2v r;
    r[0] = (E)a;
    r[1] = (E)b;
    return __builtin_bit_cast(unsigned, r);
}
// (x0, x1) -> packed 16-bit hi pair (returned) and the fp32 residuals x - float(hi): one pack + (fp16) two
// v_fma_mix_f32 reading the 16-bit halves directly (exact: a single rounding of x - hi, as the subtraction
// it replaces; no v_cvt_f32_f16 / v_pk_add_f32 + s_nop)
template <class E>
NFL_DEV unsigned nfl_split_pair(float x0, float x1, float& l0, float& l1) {
    const unsigned hi = nfl_pack2<E>(x0, x1);
    if constexpr (__is_same(E, _Float16)) {
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l0) : "v"(hi), "v"(x0));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(l1) : "v"(hi), "v"(x1));
    } else {
        // bf16 -> f32 is a shift / a mask (gfx950 has no v_fma_mix_f32_bf16); the empty asm keeps the two
        // subtractions scalar (v_pk_add_f32 beside MFMAs costs more than two v_sub_f32)
        l0 = x0 - __builtin_bit_cast(float, hi << 16);
        asm volatile("" : "+v"(l0));
        l1 = x1 - __builtin_bit_cast(float, hi & 0xffff0000u);
    }
    return hi;
}

// 8 values -> one lane's fp16 operand of a k-step: dst[0] (NP == 2: and the residuals in dst[1])
template <int NP>
NFL_DEV void nfl_split8(const float (&v)[8], h8 (&dst)[NP]) {
    using E = _Float16;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        if constexpr (NP == 2) {
            float l0, l1;
            reinterpret_cast<unsigned(&)[4]>(dst[0])[j / 2] = nfl_split_pair<E>(v[j], v[j + 1], l0, l1);
            reinterpret_cast<unsigned(&)[4]>(dst[NP - 1])[j / 2] = nfl_pack2<E>(l0, l1);
        } else {
            reinterpret_cast<unsigned(&)[4]>(dst[0])[j / 2] = nfl_pack2<E>(v[j], v[j + 1]);
        }
    }
}
