// pcx_batched_params.hip -- the per-round-parameter form of the ragged one-wave round kernel
// (pcx_consensus_ragged_params_f64, pcx_simulate_study_params_f64):
// ragged_params_round_kernel, the text of pcx_batched_round.inc once more over the device helpers of
// pcx_batched.hip, and its launcher.  A translation unit of its own: pcx_batched.hip's kernels keep
// exactly the code they have (its preprocessed text is what it was), and the 50 x 20 kernels of the
// headline path share no inlining decision with the new instantiations.
#define PCX_BATCHED_HELPERS_ONLY
#include "pcx_batched.hip"
#undef PCX_BATCHED_HELPERS_ONLY

namespace pcx {

__device__ __forceinline__ double uniform_f64(double v) {
    return __longlong_as_double((long long)uniform64((int64_t)__double_as_longlong(v)));
}

#define PCX_ROUND_RAGGED 2
#include "pcx_batched_round.inc"
#undef PCX_ROUND_RAGGED

hipError_t launch_ragged_params(const BatchArgs& a, const MediumDesc* desc, const RoundParams* params, int64_t nb,
                                int group, size_t lds, hipStream_t stream) {
    if (nb <= 0) return hipSuccess;
    (void)hipGetLastError();  // report launch errors only
    const dim3 grid((unsigned)nb), block(64);
    if (group == 2) {  // the clusterings: their own instantiation and LDS region
        static bool attr = [] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&ragged_params_round_kernel<0, 0, true, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        }();
        (void)attr;
        hipLaunchKernelGGL((ragged_params_round_kernel<0, 0, true, false>), grid, block, lds, stream, a, desc, params);
    } else if (group == 0) {
        hipLaunchKernelGGL((ragged_params_round_kernel<0, 0, false, true>), grid, block, lds, stream, a, desc, params);
    } else {
        hipLaunchKernelGGL((ragged_params_round_kernel<0, 0, false, false>), grid, block, lds, stream, a, desc, params);
    }
    return hipGetLastError();
}

}  // namespace pcx
