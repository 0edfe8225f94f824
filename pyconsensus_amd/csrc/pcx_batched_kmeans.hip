// pcx_batched_kmeans.hip -- the k-means form of the ragged one-wave round kernel
// (pcx_consensus_ragged_kmeans_f64): ragged_kmeans_round_kernel, the text of
// pcx_batched_round.inc once more over the device helpers of pcx_batched.hip, and its launcher.  The
// CLUS instantiation only: a call's hierarchical, clusterfeck and k-means rounds run on it, its other
// rounds on ragged_params_round_kernel.  A translation unit of its own, as pcx_batched_params.hip and
// for its reason: the other units' kernels keep exactly the code they have.
#define PCX_BATCHED_HELPERS_ONLY
#include "pcx_batched.hip"
#undef PCX_BATCHED_HELPERS_ONLY

namespace pcx {

__device__ __forceinline__ double uniform_f64(double v) {
    return __longlong_as_double((long long)uniform64((int64_t)__double_as_longlong(v)));
}

#define PCX_ROUND_RAGGED 3
#include "pcx_batched_round.inc"
#undef PCX_ROUND_RAGGED

hipError_t launch_ragged_kmeans(const BatchArgs& a, const MediumDesc* desc, const RoundParams* params,
                                const KmeansEntry* books, int64_t nb, size_t lds, hipStream_t stream) {
    if (nb <= 0) return hipSuccess;
    (void)hipGetLastError();  // report launch errors only
    static bool attr = [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&ragged_kmeans_round_kernel<0, 0, true, false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    }();
    (void)attr;
    hipLaunchKernelGGL((ragged_kmeans_round_kernel<0, 0, true, false>), dim3((unsigned)nb), dim3(64), lds, stream, a, desc,
                       params, books);
    return hipGetLastError();
}

}  // namespace pcx
