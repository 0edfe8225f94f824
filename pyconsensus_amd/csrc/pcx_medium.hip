// pcx_medium.hip -- batched oracle rounds above one wavefront (64 < N <= 256 reporters or
// 32 < E <= 64 events): one 256-thread workgroup per round.
//
// Each round is Oracle(reports, event_bounds, reputation).consensus() (pyconsensus/
// __init__.py:102-611) in the operation order of the batched SPEC
// (oracle/pcx_oracle_batched.c one_round, built with NMAX = 256 for these shapes), so the
// results are bit-identical to it: the reference's own orders where they are known (numpy
// pairwise sums, the OpenBLAS dgemv order of np.dot, weightedstats' sequential walk, the
// interpolation's sequential means) and the SPEC's fixed orders elsewhere (fma chains of the
// covariance and scores, the power iteration with Gram squarings, tree64 norms).
//
// Work split: one thread per event column, per reporter row, per matrix entry or per 4 x 4
// tile, as each step allows; one wave per weighted median (bitonic (x, w, index) order, the
// sequential total and walk on every lane alike) and per certainty; the power steps on one
// wave; the reference's sequential sums in their order, loads issued ahead.  LDS holds a work
// region (power-iteration matrices / median scratch / staged covariance rows / np.dot block
// partials), the per-element NA flags and the row / event vectors; the filled matrix and the
// covariance live in a per-round global scratch (L2-resident).  DESIGN.md 5.3.
// Algorithms: all eight; "hierarchical", "clusterfeck" and "k-means" (code books up to 16) in a
// second instantiation of the kernel, their cluster sums / whitened observations in a second
// per-round global scratch.
// The kernel's text is pcx_medium_round.inc over the helpers of pcx_medium_device.inc: compiled here
// as medium_round_kernel (rounds of one shape), and in pcx_medium_ragged.hip as ragged_medium_kernel
// (a descriptor per round: pcx_consensus_ragged_wide_f64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcx_internal.h"

namespace pcx {
namespace {

#include "pcx_medium_device.inc"

// the round kernel's text (pcx_medium_round.inc), here under its equal-shape name
#define PCX_MEDIUM_RAGGED 0
#include "pcx_medium_round.inc"
#undef PCX_MEDIUM_RAGGED

}  // namespace

bool medium_fits(int N, int E, int alg, int kmeans_k) {
    return N >= 1 && N <= MN && E >= 1 && E <= MEV && alg >= PCX_ALG_PCA && alg <= PCX_ALG_CLUSTERFECK &&
           (alg != PCX_ALG_KMEANS || (kmeans_k >= 1 && kmeans_k <= M_KMAX));
}

size_t medium_lds_bytes(int N, int E, int alg) {
    return ((size_t)medium_region(N, E, alg) + (size_t)VN_COUNT * N + (size_t)VE_COUNT * E) * sizeof(double) +
           (size_t)((N * E + 15) >> 4) * 4 + 16;
}

// scratch bytes of one round: the filled matrix unless the caller keeps it, the covariance, the
// clusterings' N x E (clusterfeck: two)
size_t medium_scratch_per_round(const BatchArgs& a) {
    const size_t ne = (size_t)a.N * a.E;
    return ((a.filled ? 0 : ne) + (size_t)a.E * a.E + (size_t)medium_xscratch(a.N, a.E, a.algorithm)) * sizeof(double);
}

// rounds in chunks whose scratch fits `scratch_bytes`
int64_t medium_chunk(const BatchArgs& a, size_t scratch_bytes) {
    const size_t per = medium_scratch_per_round(a);
    int64_t c = (int64_t)(scratch_bytes / (per ? per : 1));
    return c < 1 ? 1 : (c > a.B ? a.B : c);
}

hipError_t launch_medium(const BatchArgs& a, int64_t b0, int64_t nb, double* Fscr, double* Cscr, double* Xscr,
                         hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    const size_t lds = medium_lds_bytes(a.N, a.E, a.algorithm);
    // (dynamic LDS above 64 KB needs no attribute on gfx950: the launch checks it against 160 KB)
    (void)hipGetLastError();  // report launch errors only
    if (a.algorithm >= PCX_ALG_KMEANS)
        hipLaunchKernelGGL(medium_round_kernel<true>, dim3((unsigned)nb), dim3(MT), lds, st, a, b0, Fscr, Cscr, Xscr);
    else
        hipLaunchKernelGGL(medium_round_kernel<false>, dim3((unsigned)nb), dim3(MT), lds, st, a, b0, Fscr, Cscr, Xscr);
    return hipGetLastError();
}

}  // namespace pcx
