// pcx_tall_ragged.hip -- tall rounds (256 < N <= 1024 reporters, E <= 64 events) with a shape and a
// parameter set per round: the tall segment of a ragged table plan (pcx_consensus_ragged_tall_f64,
// pcx_simulate_study_tall_f64).  ragged_params_tall_kernel is the text of
// pcx_medium_round.inc a sixth time, over the helpers of pcx_medium_device.inc under PCX_MEDIUM_TALL
// and in the per-round-parameter form (PCX_MEDIUM_RAGGED 2): the descriptor and the round's entry of
// the parameter table go to scalar registers, then the round's own LDS plan (tall_plan) is computed
// from them.  A translation unit of its own, as pcx_tall.hip and for its reason: the five other
// units' kernels keep the code objects they had.  No clustering (they stay at 256 reporters).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcx_internal.h"

#ifndef PCX_TALL_WAVES  // waves per SIMD the VGPR budget is sized for (pcx_tall.hip's)
#define PCX_TALL_WAVES 2
#endif

namespace pcx {
namespace {

#define PCX_MEDIUM_TALL 1
#include "pcx_medium_device.inc"

// a workgroup-uniform 64-bit value into scalar registers (the descriptor's and the entry's fields)
__device__ __forceinline__ int64_t muniform64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double muniform_f64(double v) {
    return __longlong_as_double((long long)muniform64((int64_t)__double_as_longlong(v)));
}

#define PCX_MEDIUM_RAGGED 2
#include "pcx_medium_round.inc"
#undef PCX_MEDIUM_RAGGED

}  // namespace

hipError_t launch_ragged_tall_params(const BatchArgs& a, const MediumDesc* desc, const RoundParams* params, int64_t nb,
                                     size_t lds, const int64_t s[2], double* Fscr, double* Cscr, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    if (!lds || lds > (size_t)(TALL_LDS_LIMIT - TALL_STATIC_LDS)) return hipErrorInvalidValue;
    // the plan's allowance for the kernel's static LDS against the code object's own figure
    static const hipError_t checked = [] {
        hipFuncAttributes fa;
        const hipError_t e =
            hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(ragged_params_tall_kernel<false>));
        if (e != hipSuccess) return e;
        return fa.sharedSizeBytes <= (size_t)TALL_STATIC_LDS ? hipSuccess : hipErrorInvalidConfiguration;
    }();
    if (checked != hipSuccess) return checked;
    (void)hipGetLastError();  // report launch errors only
    hipLaunchKernelGGL(ragged_params_tall_kernel<false>, dim3((unsigned)nb), dim3(MT), lds, st, a, desc, params, s[0],
                       s[1], Fscr, Cscr);
    return hipGetLastError();
}

}  // namespace pcx
