// pcx_tall.hip -- tall batched rounds (256 < N <= 1024 reporters, E <= 64 events): one workgroup
// per round, one asynchronous launch, bit-identical to the batched SPEC (oracle/pcx_oracle_batched.c
// one_round) built with NMAX = 1024.  pcx_consensus_batched_tall_f64, DESIGN.md 5.3.1.
//
// The kernel's text is pcx_medium_round.inc over the helpers of pcx_medium_device.inc, compiled a
// further time under PCX_MEDIUM_TALL as tall_round_kernel -- a translation unit of its own, so the
// kernels of pcx_medium.hip, pcx_medium_ragged.hip, pcx_medium_params.hip and pcx_medium_kmeans.hip
// keep the code objects they had.  What differs from medium_round_kernel: numpy's pairwise sum to
// any depth (mpw), the NaN rank path of the weighted median over sixteen elements a lane, and an
// LDS plan per shape (tall_plan) in place of the fixed carve -- the waves that run medians and
// certainties side by side (4, 2 or 1) and the np.dot block partials in row chunks, each column's
// chain of additions unchanged.  Algorithms: PCA, absolute, big-five, fixed-variance, cokurtosis;
// the clusterings are one thread per reporter row by design and stay at 256 reporters.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcx_internal.h"

#ifndef PCX_TALL_WAVES  // waves per SIMD the VGPR budget is sized for
#define PCX_TALL_WAVES 2
#endif

namespace pcx {
namespace {

#define PCX_MEDIUM_TALL 1
#include "pcx_medium_device.inc"

#define PCX_MEDIUM_RAGGED 0
#include "pcx_medium_round.inc"
#undef PCX_MEDIUM_RAGGED

}  // namespace

// the plan of an N x E round: {median waves, rows per np.dot chunk, np.dot chunks, threads}; false
// (and zeros) where the round does not fit a workgroup's LDS or the kernel does not take it
bool tall_plan_query(int N, int E, int alg, int32_t out[4]) {
    const TallPlan p = tall_plan(N, E, alg);
    out[0] = p.waves;
    out[1] = p.waves ? 4 * p.nbc : 0;
    out[2] = p.chunks;
    out[3] = p.waves ? MT : 0;
    return p.waves > 0;
}

// dynamic LDS of one round; 0 where the plan does not fit
size_t tall_lds_bytes(int N, int E, int alg) {
    const TallPlan p = tall_plan(N, E, alg);
    if (!p.waves) return 0;
    return (size_t)p.region * sizeof(double) + (size_t)tall_fixed_bytes(N, E);
}

hipError_t launch_tall(const BatchArgs& a, int64_t b0, int64_t nb, double* Fscr, double* Cscr, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    const size_t lds = tall_lds_bytes(a.N, a.E, a.algorithm);
    if (!lds) return hipErrorInvalidValue;
    // the plan's allowance for the kernel's static LDS against the code object's own figure
    static const hipError_t checked = [] {
        hipFuncAttributes fa;
        const hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(tall_round_kernel<false>));
        if (e != hipSuccess) return e;
        return fa.sharedSizeBytes <= (size_t)TALL_STATIC_LDS ? hipSuccess : hipErrorInvalidConfiguration;
    }();
    if (checked != hipSuccess) return checked;
    // (dynamic LDS above 64 KB needs no attribute on gfx950: the launch checks it against 160 KB)
    (void)hipGetLastError();  // report launch errors only
    hipLaunchKernelGGL(tall_round_kernel<false>, dim3((unsigned)nb), dim3(MT), lds, st, a, b0, Fscr, Cscr,
                       (double*)nullptr);
    return hipGetLastError();
}

}  // namespace pcx
