// nfl_stamps.h -- diagnostic builds only (make diag, -DNFL_STAMPS): the buffer the stamped kernel writes its per-wave
// cycle totals to, and its host reader.  Defines a device global and a C symbol, so exactly one translation unit of a
// library includes it: the one that `make diag` builds with the stamps (DIAGTU).
#pragma once
#include <hip/hip_runtime.h>
#define NFL_NSTAMP 20
__device__ unsigned long long nfl_stamp_buf[1024 * 4 * NFL_NSTAMP];
// copy the per-wave phase cycle totals of the last launch to the host
extern "C" int nfl_debug_stamps(unsigned long long* host, int n_entries) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(nfl_stamp_buf), sizeof(unsigned long long) * n_entries) == hipSuccess ? 0 : -1;
}
