// pcx_medium_ragged.hip -- the ragged form of the workgroup-per-round kernel (a shape per round,
// pcx_consensus_ragged_wide_f64): ragged_medium_kernel, the text of
// pcx_medium_round.inc over the helpers of pcx_medium_device.inc, the scatter of the one-wave
// rounds' per-round outputs, and their launchers.  A translation unit of its own: built into
// pcx_medium.hip, the new kernels moved the register numbering and the placement of the equal-shape
// clustering kernel, which ran 1 % slower for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "pcx_internal.h"

namespace pcx {
namespace {

#include "pcx_medium_device.inc"

// a workgroup-uniform 64-bit value into scalar registers (a ragged launch's descriptor fields)
__device__ __forceinline__ int64_t muniform64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

#define PCX_MEDIUM_RAGGED 1
#include "pcx_medium_round.inc"
#undef PCX_MEDIUM_RAGGED

// The six [B] outputs of a ragged launch's wave-sized rounds, from where ragged_round_kernel wrote
// them (slot k of its own launch) to their rounds' indices idx[k] in the caller's arrays; a null
// output is skipped.
__global__ void __launch_bounds__(256) ragged_scatter_kernel(const int32_t* __restrict__ idx, int64_t n, WaveTmp s,
                                                             BatchArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int64_t b = idx[k];
    if (a.participation) a.participation[b] = s.participation[k];
    if (a.avg_certainty) a.avg_certainty[b] = s.avg_certainty[k];
    if (a.branch) a.branch[b] = s.branch[k];
    if (a.flags) a.flags[b] = s.flags[k];
    if (a.pi_iters) a.pi_iters[b] = s.pi_iters[k];
    if (a.components) a.components[b] = s.components[k];
}

}  // namespace

int medium_launch_class(size_t dyn_lds) {
    const size_t unit = 1280, cu = 160 * 1024;
    const size_t wg = (dyn_lds + MEDIUM_STATIC_LDS + unit - 1) / unit * unit;
    const size_t fit = cu / wg;
    return fit >= PCX_MEDIUM_WAVES ? PCX_MEDIUM_WAVES : fit < 1 ? 1 : (int)fit;
}

void medium_slot_strides(int N, int E, int alg, int64_t s[3]) {
    s[0] = std::max<int64_t>(s[0], (int64_t)N * E);
    s[1] = std::max<int64_t>(s[1], (int64_t)E * E);
    s[2] = std::max<int64_t>(s[2], medium_xscratch(N, E, alg));
}

hipError_t launch_ragged_medium(const BatchArgs& a, const MediumDesc* desc, int64_t nb, size_t lds, const int64_t s[3],
                                double* Fscr, double* Cscr, double* Xscr, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    (void)hipGetLastError();  // report launch errors only
    if (a.algorithm >= PCX_ALG_KMEANS)
        hipLaunchKernelGGL(ragged_medium_kernel<true>, dim3((unsigned)nb), dim3(MT), lds, st, a, desc, s[0], s[1], s[2],
                           Fscr, Cscr, Xscr);
    else
        hipLaunchKernelGGL(ragged_medium_kernel<false>, dim3((unsigned)nb), dim3(MT), lds, st, a, desc, s[0], s[1], s[2],
                           Fscr, Cscr, Xscr);
    return hipGetLastError();
}

hipError_t launch_ragged_scatter(const BatchArgs& a, const int32_t* idx, int64_t n, void* tmp, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ragged_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, idx, n,
                       ragged_wave_tmp(tmp, n), a);
    return hipGetLastError();
}

}  // namespace pcx
