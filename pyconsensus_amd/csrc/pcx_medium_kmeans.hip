// pcx_medium_kmeans.hip -- the k-means form of the ragged workgroup-per-round kernel
// (pcx_consensus_ragged_kmeans_f64): ragged_kmeans_medium_kernel, the text of
// pcx_medium_round.inc once more over the helpers of pcx_medium_device.inc, and its launcher.  The
// CLUS instantiation only: a call's hierarchical, clusterfeck and k-means rounds above 64 x 32 run on
// it, its other rounds on ragged_params_medium_kernel.  A translation unit of its own, as
// pcx_medium_params.hip and for its reason: the other units' kernels keep the code they have.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcx_internal.h"

namespace pcx {
namespace {

#include "pcx_medium_device.inc"

// a workgroup-uniform 64-bit value into scalar registers (the descriptor's and the entries' fields)
__device__ __forceinline__ int64_t muniform64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double muniform_f64(double v) {
    return __longlong_as_double((long long)muniform64((int64_t)__double_as_longlong(v)));
}

#define PCX_MEDIUM_RAGGED 3
#include "pcx_medium_round.inc"
#undef PCX_MEDIUM_RAGGED

}  // namespace

hipError_t launch_ragged_medium_kmeans(const BatchArgs& a, const MediumDesc* desc, const RoundParams* params,
                                       const KmeansEntry* books, int64_t nb, size_t lds, const int64_t s[3],
                                       double* Fscr, double* Cscr, double* Xscr, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    (void)hipGetLastError();  // report launch errors only
    hipLaunchKernelGGL(ragged_kmeans_medium_kernel<true>, dim3((unsigned)nb), dim3(MT), lds, st, a, desc, params, books,
                       s[0], s[1], s[2], Fscr, Cscr, Xscr);
    return hipGetLastError();
}

}  // namespace pcx
