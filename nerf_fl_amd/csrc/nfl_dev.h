// nfl_dev.h -- the small helpers that kernels of different translation units share: wave reductions, the kernarg re-read,
// the gradient-maximum word; their launchers' two runtime queries.  Defines no device globals: any unit may include it.
#pragma once
#include "../../include/nerf_fl_amd.h"
#include "nfl_macros.h"
#include "nfl_plan.h"

// reductions over the 64 lanes of a wave by xor butterfly: every lane ends with the result, and the order of the
// additions is the same on every lane
NFL_DEV float nfl_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
NFL_DEV unsigned nfl_wave_max(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}
// sum over 32 lanes (both halves of the wave run it independently)
NFL_DEV float nfl_sum32(float v) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 32);
    return v;
}

// A kernel's argument block (T = the type of its one by-value argument), re-read from the kernarg segment.  Values loaded
// through the returned pointer cannot be hoisted above the call (the empty asm makes the pointer opaque), so arguments that
// are only needed in the cold parts of a tile (ray set-up, compositing, outputs, loss) are s_load'ed there instead of being
// kept in SGPRs -- or rather in SGPR spill lanes of VGPRs -- across the whole MLP, where every register is spoken for.
template <class T>
using NflKernarg = const __attribute__((address_space(4))) T*;
template <class T>
NFL_DEV NflKernarg<T> nfl_kernarg() {
    NflKernarg<T> p = (NflKernarg<T>)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
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
    return __builtin_amdgcn_readfirstlane(nfl_wave_max(v));
}

// ---- the two runtime queries of the launchers with dynamic LDS (forward, dgrad, wgrad) ----
struct NflDevice {
    int ordinal, n_cu;        // the current device and its CU count (256 where the runtime does not say)
};
static inline NflDevice nfl_device() {
    NflDevice d = {0, 256};
    if (hipGetDevice(&d.ordinal) == hipSuccess) (void)hipDeviceGetAttribute(&d.n_cu, hipDeviceAttributeMultiprocessorCount, d.ordinal);
    return d;
}
// Raises KERNEL's dynamic-LDS limit to `bytes` on the current device, `ordinal`, once per device: the attribute is per
// device.  (Two threads may both make the first call; it is idempotent.  Ordinals beyond 63 make it every time.)
template <auto KERNEL>
static int nfl_lds_attr(int ordinal, int bytes) {
    static unsigned long long done = 0ull;
    const unsigned long long bit = (unsigned)ordinal < 64u ? 1ull << ordinal : 0ull;
    if (done & bit) return NFL_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return NFL_ENODEV;
    done |= bit;
    return NFL_OK;
}
