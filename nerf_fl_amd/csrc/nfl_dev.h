// nfl_dev.h -- the device-side helpers that the fused MLP kernels (nfl_render_impl.h) and the weight-gradient kernels
// (nfl_wgrad.hip) share.  Defines no device globals, so any translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "nfl_plan.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));     // one lane's MFMA operand of v_mfma_f32_32x32x16_f16
typedef float f16v __attribute__((ext_vector_type(16)));     // one lane's 32 x 32 accumulator

#define NFL_DEV __device__ __forceinline__

// compile-time loop: f(integral_constant<int, I>) for I in [I0, I1)
template <int I0, int I1, class F>
NFL_DEV void nfl_static_for(F&& f) {
    if constexpr (I0 < I1) {
        f(std::integral_constant<int, I0>{});
        nfl_static_for<I0 + 1, I1>(f);
    }
}

// max over the NFL_GMAX_SLOTS words the compositing backward left (bit patterns of non-negative floats order
// like unsigned integers); wave-uniform result
NFL_DEV unsigned nfl_gmax_bits(const float* d_gmax) {
    unsigned v = 0u;
    if (d_gmax)
        for (int i = threadIdx.x & 63; i < NFL_GMAX_SLOTS; i += 64) {
            const unsigned o = reinterpret_cast<const unsigned*>(d_gmax)[i];
            v = o > v ? o : v;
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}
