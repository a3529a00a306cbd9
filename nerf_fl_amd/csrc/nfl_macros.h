// nfl_macros.h -- what every device header starts from: the NFL_DEV qualifier, the compile-time loop and the two MFMA
// vector types.  No other include of the project, so the leaf headers (nfl_math.h, nfl_pixel.h) stay leaves.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

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
