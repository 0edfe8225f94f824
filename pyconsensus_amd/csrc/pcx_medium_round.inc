// pcx_medium_round.inc -- the workgroup-per-round kernel's text, included by pcx_medium.hip as
// medium_round_kernel (PCX_MEDIUM_RAGGED 0: rounds of one shape, round b0 + blockIdx.x) and by
// pcx_medium_ragged.hip as ragged_medium_kernel (PCX_MEDIUM_RAGGED 1: a shape per round).  One text
// under two kernel names, as pcx_batched_round.inc: the equal-shape instantiations keep exactly the
// code they had (the kernel sits at its VGPR cap; a shared __device__ body moved the one-wave
// kernel's allocation), and the two cannot drift apart.
//
// Ragged: workgroup blockIdx.x reads rag[blockIdx.x] (MediumDesc) for its shape, for the offsets
// of its cells, reporters and events in the flat inputs and outputs, and for its round's index
// (the [B] outputs; the launch's workgroups are one launch class of the call's rounds, in any
// subset and order).  The descriptor is uniform over the workgroup: read once, held in scalar
// registers.  The round carves its LDS from its own N and E and never reaches past that carve;
// the launch allocates its largest round's.  The scratch slot stays blockIdx.x, its strides
// (sF, sC, sX doubles) the launch's largest N E, E E and medium_xscratch.  big-five caps
// max_components at the round's E; bounds_shared does not exist; k-means is refused by the caller.
//
// CLUS: the instantiation that also holds the clusterings (their code and registers stay out of
// the other one); Xscr is their per-round N x E scratch
//
// Per-round parameters (PCX_MEDIUM_RAGGED 2, pcx_medium_params.hip: ragged_params_medium_kernel,
// DESIGN.md 5.4.3): the ragged form with the round's entry rag[blockIdx.x].param of a device table
// RoundParams[P] written over the seven parameter fields of a local copy `a` of the kernel argument
// `ka` (workgroup-uniform, scalar registers, like the descriptor).  Everything below reads `a`: the
// LDS carve, the work region, the scratch slots and the layout follow the round's own algorithm.
//
// k-means (PCX_MEDIUM_RAGGED 3, pcx_medium_kmeans.hip: ragged_kmeans_medium_kernel, DESIGN.md 5.5.2):
// that form with the round's entry {offset, k} of a device table KmeansEntry[B], indexed by the
// round, written over the copy's kmeans_k and added to its kmeans_init: mkmeans_nc reads the round's
// own books as round 0's.
//
// Tall rounds (PCX_MEDIUM_TALL 1 with PCX_MEDIUM_RAGGED 0, pcx_tall.hip: tall_round_kernel, DESIGN.md
// 5.3.1): rounds of one shape with 256 < N <= 1024.  The work region, the number of waves that run
// medians and certainties side by side, and the np.dot partials' chunks come from the round's LDS
// plan (tall_plan) in place of medium_region / medium_work / MT / 64; no clustering.
//
// Tall rounds with a shape and a parameter set per round (PCX_MEDIUM_TALL 1 with PCX_MEDIUM_RAGGED 2,
// pcx_tall_ragged.hip: ragged_params_tall_kernel, DESIGN.md 5.5.3): the per-round-parameter form whose
// plan is the round's own -- tall_plan of the descriptor's N and E and the set's algorithm, computed
// once they sit in scalar registers.  The launch's dynamic LDS is its largest round's plan; the
// scratch slots are blockIdx.x at the launch's strides sF, sC; no clustering, so no third slot.
#if PCX_MEDIUM_TALL
#define PCX_MROUND_REGION tplan.region
#define PCX_MROUND_WORK tplan.region
#define PCX_MROUND_MWAVES tplan.waves
#define PCX_MROUND_WV0(end) (wv < tplan.waves ? wv : (end))
#define PCX_MROUND_VECMAT(v, out) bvecmat_chunked(v, F, N, E, out, mlds, tplan.nbc)
#else
#define PCX_MROUND_REGION medium_region(N, E, a.algorithm)
#define PCX_MROUND_WORK medium_work(N, E, a.algorithm)
#define PCX_MROUND_MWAVES (MT / 64)
#define PCX_MROUND_WV0(end) wv
#define PCX_MROUND_VECMAT(v, out) bvecmat(v, F, N, E, out, mlds)
#endif
#if PCX_MEDIUM_RAGGED
#define PCX_MROUND_CELL0 rcell
#define PCX_MROUND_ROW0 rrow
#define PCX_MROUND_EV0 rev
#define PCX_MROUND_BO rev
#define PCX_MROUND_FSLOT ((int64_t)blockIdx.x * sF)
#define PCX_MROUND_CSLOT ((int64_t)blockIdx.x * sC)
#define PCX_MROUND_XSLOT ((int64_t)blockIdx.x * sX)
#define PCX_MROUND_ARGS ar
template <bool CLUS>
#if PCX_MEDIUM_TALL  // (with PCX_MEDIUM_RAGGED 2 alone)
__global__ void __launch_bounds__(MT, PCX_TALL_WAVES) ragged_params_tall_kernel(
    BatchArgs ka, const MediumDesc* __restrict__ rag, const RoundParams* __restrict__ ptab, int64_t sF, int64_t sC,
    double* Fscr, double* Cscr) {
#elif PCX_MEDIUM_RAGGED == 3
__global__ void __launch_bounds__(MT, PCX_MEDIUM_WAVES) ragged_kmeans_medium_kernel(
    BatchArgs ka, const MediumDesc* __restrict__ rag, const RoundParams* __restrict__ ptab,
    const KmeansEntry* __restrict__ ktab, int64_t sF, int64_t sC, int64_t sX, double* Fscr, double* Cscr, double* Xscr) {
#elif PCX_MEDIUM_RAGGED == 2
__global__ void __launch_bounds__(MT, PCX_MEDIUM_WAVES) ragged_params_medium_kernel(
    BatchArgs ka, const MediumDesc* __restrict__ rag, const RoundParams* __restrict__ ptab, int64_t sF, int64_t sC,
    int64_t sX, double* Fscr, double* Cscr, double* Xscr) {
#else
__global__ void __launch_bounds__(MT, PCX_MEDIUM_WAVES) ragged_medium_kernel(BatchArgs a, const MediumDesc* __restrict__ rag,
                                                                             int64_t sF, int64_t sC, int64_t sX,
                                                                             double* Fscr, double* Cscr, double* Xscr) {
#endif
    extern __shared__ __attribute__((aligned(16))) double mlds[];
    __shared__ double sh[MT];
    __shared__ double scal[16];
    const MediumDesc* const rd = rag + blockIdx.x;
    const int N = __builtin_amdgcn_readfirstlane(rd->N), E = __builtin_amdgcn_readfirstlane(rd->E), ES = E + 1;
    const int64_t b = __builtin_amdgcn_readfirstlane(rd->round);  // round; scratch slot blockIdx.x
    const int64_t rcell = muniform64(rd->cell), rrow = muniform64(rd->row), rev = muniform64(rd->ev);
#if PCX_MEDIUM_RAGGED >= 2
    const RoundParams* const rp = ptab + __builtin_amdgcn_readfirstlane(rd->param);
    BatchArgs a = ka;
    a.algorithm = __builtin_amdgcn_readfirstlane(rp->algorithm);
    a.max_components = __builtin_amdgcn_readfirstlane(rp->max_components);
    a.catch_tol = muniform_f64(rp->catch_tol);
    a.alpha = muniform_f64(rp->alpha);
    a.variance_threshold = muniform_f64(rp->variance_threshold);
    a.hierarchy_threshold = muniform_f64(rp->hierarchy_threshold);
    a.cluster_threshold = muniform_f64(rp->cluster_threshold);
#endif
#if PCX_MEDIUM_RAGGED == 3
    const KmeansEntry* const ke = ktab + b;
    a.kmeans_k = __builtin_amdgcn_readfirstlane(ke->k);
    a.kmeans_init = ka.kmeans_init + muniform64(ke->offset);
#endif
    BatchArgs ar = a;  // what component_scores reads: the round's shape, max_components capped (:134-137)
    ar.N = N;
    ar.E = E;
    ar.max_components = a.max_components < E ? a.max_components : E;
#if PCX_MEDIUM_TALL
    const TallPlan tplan = tall_plan(N, E, a.algorithm);  // (the round's own, uniform like its descriptor)
#endif
#else
#define PCX_MROUND_CELL0 (b * N * E)
#define PCX_MROUND_ROW0 (b * N)
#define PCX_MROUND_EV0 (b * E)
#define PCX_MROUND_BO (a.bounds_shared ? 0 : b * E)
#define PCX_MROUND_FSLOT ((int64_t)blockIdx.x * N * E)
#define PCX_MROUND_CSLOT ((int64_t)blockIdx.x * E * E)
#define PCX_MROUND_XSLOT ((int64_t)blockIdx.x * medium_xscratch(N, E, alg))
#define PCX_MROUND_ARGS a
template <bool CLUS>
#if PCX_MEDIUM_TALL
__global__ void __launch_bounds__(MT, PCX_TALL_WAVES) tall_round_kernel(BatchArgs a, int64_t b0, double* Fscr, double* Cscr,
                                                                        double* Xscr) {
#else
__global__ void __launch_bounds__(MT, PCX_MEDIUM_WAVES) medium_round_kernel(BatchArgs a, int64_t b0, double* Fscr, double* Cscr,
                                                                            double* Xscr) {
#endif
    extern __shared__ __attribute__((aligned(16))) double mlds[];
    __shared__ double sh[MT];
    __shared__ double scal[16];
    const int64_t b = b0 + blockIdx.x;  // round; scratch slot blockIdx.x
    const int N = a.N, E = a.E, ES = E + 1;
#if PCX_MEDIUM_TALL
    const TallPlan tplan = tall_plan(N, E, a.algorithm);  // (uniform: scalar registers)
#endif
#endif
    const int tid = threadIdx.x;
    double* M = mlds;
    double* Tm = M + E * ES;
    // work region: M and Tm in the power iteration / Jacobi, per wave the median operands and
    // sort scratch in the interpolation, the outcomes and the certainty
    double* vN = mlds + PCX_MROUND_REGION;
    double* vE = vN + VN_COUNT * N;
    // NA flags [N][E], two bits per element (bit 0 NaN, bit 1 zero), sixteen to a word
    uint32_t* flw = (uint32_t*)(vE + VE_COUNT * E);
    auto FL = [&](int e) -> uint32_t { return (flw[e >> 4] >> ((e & 15) << 1)) & 3u; };
    auto VNp = [&](int k) { return vN + k * N; };
    auto VEp = [&](int k) { return vE + k * E; };
    double* rep = VNp(VN_REP);
    double* tok = VNp(VN_TOK);
    const double* Rin = a.reports + PCX_MROUND_CELL0;
    double* F = a.filled ? a.filled + PCX_MROUND_CELL0 : Fscr + PCX_MROUND_FSLOT;
    double* C = Cscr + PCX_MROUND_CSLOT;
    const int64_t bo = PCX_MROUND_BO;
    const bool has_bounds = a.scaled != nullptr;
    const int alg = a.algorithm;
    const int lane = tid & 63, wv = tid >> 6;
    const int PN = medium_pow2(N);
    double* wb = mlds + wv * medium_wave_stride(N);  // this wave's median operands and sort scratch
    __shared__ unsigned long long scmask_s;
    __shared__ int scl[MEV], nscl_s;
    MSTAMP(0);
    if (tid < 64) {  // the scaled events: a mask and their list in index order
        const bool p = has_bounds && tid < E && a.scaled[bo + tid] != 0;
        const unsigned long long bal = __ballot(p);
        if (p) scl[__popcll(bal & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) {
            scmask_s = bal;
            nscl_s = __popcll(bal);
        }
    }
    auto scaled = [&](int j) { return ((scmask_s >> j) & 1ull) != 0; };
    long long mprof[3] = {0, 0, 0};  // diagnostic (PCX_STAMPS): median total+dom / rank / walk cycles

    for (int w = tid; w < (N * E + 15) >> 4; w += MT) flw[w] = 0u;  // (ordered by the barrier below)
    // --- a1: reputation (:138-146)
    if (tid == 0) scal[0] = a.reputation ? mpw([&](int i) { return a.reputation[PCX_MROUND_ROW0 + i]; }, N) : 0.0;
    __syncthreads();
    for (int i = tid; i < N; i += MT) {
        const double r = a.reputation ? a.reputation[PCX_MROUND_ROW0 + i] / scal[0] : 1.0 / (double)N;
        rep[i] = r;
        tok[i] = trunc(r * 1e6);
    }
    __syncthreads();
    if (tid == 0) scal[1] = mseq([&](int i) { return tok[i]; }, N) - 1.0;  // denom
    // --- a2: rescale (:266-269), NA (:278)
    for (int e0 = tid; e0 < N * E; e0 += 8 * MT) {  // eight reports' loads ahead of the stores
        double xv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = e0 + u * MT;
            xv[u] = e < N * E ? Rin[e] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = e0 + u * MT;
            if (e >= N * E) break;
            const int j = e % E;
            double x = xv[u];
            if (scaled(j)) {
                x = (x - a.lo[bo + j]) / (a.hi[bo + j] - a.lo[bo + j]);
                if (a.int_dtype) x = trunc(x);
            }
            F[e] = x;
            const uint32_t bits = (__builtin_isnan(x) ? 1u : 0u) | (x == 0.0 ? 2u : 0u);
            if (bits) atomicOr(&flw[e >> 4], bits << ((e & 15) << 1));
            if (a.original) a.original[PCX_MROUND_CELL0 + e] = x;
        }
    }
    __syncthreads();
    MSTAMP(1);
    // --- a3: interpolate (:284-313): binary columns one thread each; scaled columns one at a
    // time with the whole block (weighted median)
    {
        // one thread per binary column (E <= 64): the present total from the LDS flags, then the
        // weighted mean over the present rows in row order, the filled matrix staged through the
        // work region in row chunks (one round trip per chunk, not per eight rows)
        const int j = tid;
        const bool act = j < E && !scaled(j);
        int nmiss = 0;
        double tot = 0.0;
        if (act) {
            int i = 0;
            for (; i + 8 <= N; i += 8) {
                uint8_t f[8];
                double r[8];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    f[q] = FL((i + q) * E + j);
                    r[q] = rep[i + q];
                }
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    nmiss += f[q] ? 1 : 0;
                    if (!f[q]) tot += r[q];
                }
            }
            for (; i < N; i++) {
                const bool m = FL(i * E + j) != 0;
                nmiss += m ? 1 : 0;
                if (!m) tot += rep[i];
            }
        }
        const bool need = act && nmiss > 0;
        double g = 0.0;
        if (__syncthreads_or(need)) {
            int CR = PCX_MROUND_WORK / E;
            CR = CR > 64 ? 64 : CR;
            double* st = mlds;
            for (int c0 = 0; c0 < N; c0 += CR) {
                const int cr = N - c0 < CR ? N - c0 : CR;
                for (int idx = tid; idx < cr * E; idx += MT) st[idx] = F[c0 * E + idx];
                __syncthreads();
                if (need) {
                    int r = 0;
                    for (; r + 8 <= cr; r += 8) {
                        uint8_t f[8];
                        double w8[8], x[8];
#pragma unroll
                        for (int q = 0; q < 8; q++) {
                            f[q] = FL((c0 + r + q) * E + j);
                            w8[q] = rep[c0 + r + q];
                            x[q] = st[(r + q) * E + j];
                        }
#pragma unroll
                        for (int q = 0; q < 8; q++)
                            if (!f[q]) g += (w8[q] / tot) * x[q];
                    }
                    for (; r < cr; r++)
                        if (!FL((c0 + r) * E + j)) g += (rep[c0 + r] / tot) * st[r * E + j];
                }
                __syncthreads();
            }
        }
        if (need) {
            g = mcatch(g, a.catch_tol);
            if (a.int_dtype) g = trunc(g);
            for (int i = 0; i < N; i++)
                if (FL(i * E + j)) F[i * E + j] = g;
        }
    }
    MSTAMP(2);
    const int nscl = nscl_s;
    for (int c = PCX_MROUND_WV0(nscl); c < nscl; c += PCX_MROUND_MWAVES) {  // one wave per scaled column
        const int j = scl[c];
        // present values and their reputations in row order (wave compaction), then the
        // sequential present total on lane 0 and the weights rep / total
        int np_ = 0;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            const bool p = i < N && FL(i * E + j) == 0;
            const unsigned long long bal = __ballot(p);
            if (p) {
                const int o = np_ + __popcll(bal & ((1ull << lane) - 1ull));
                wb[o] = F[i * E + j];
                wb[N + o] = rep[i];
            }
            np_ += __popcll(bal);
        }
        mwsync();
        double tot = 0.0;
        if (lane == 0) tot = mseq([&](int q) { return wb[N + q]; }, np_);
        tot = mbcast(tot, 0);
        for (int q = lane; q < np_; q += 64) wb[N + q] = wb[N + q] / tot;
        mwsync();
        if (np_ < N) {  // wave-uniform
            double g = wv_wmedian(wb, wb + N, np_, wb + 2 * N, PN);
            if (a.int_dtype) g = trunc(g);
            for (int i = lane; i < N; i += 64)
                if (FL(i * E + j)) F[i * E + j] = g;
        }
        mwsync();
    }
    __syncthreads();
    MSTAMP(3);
    // old = np.dot(rep, F) (:489)
    PCX_MROUND_VECMAT([&](int i) { return rep[i]; }, VEp(VE_OLD));
    double* loading = VEp(VE_LD);
    double* s = VNp(VN_S);
    double* nc = VNp(VN_U);  // nc, then u
    int flags = 0, iters = 0, branch = PCX_BRANCH_NONE;
    for (int j = tid; j < E; j += MT) loading[j] = 0.0;
    for (int i = tid; i < N; i += MT) s[i] = nc[i] = 0.0;
    __syncthreads();
    MSTAMP(4);
    int comps = -1;
    const bool clustering = CLUS && alg >= PCX_ALG_KMEANS;  // they call wpca too: loading only
    if (alg == PCX_ALG_PCA || alg == PCX_ALG_BIG_FIVE || alg == PCX_ALG_FIXED_VARIANCE || clustering) {
        // --- a5: weighted mean (np.ma.average, :317-319)
        double* mu = VEp(VE_MU);
        if (tid == 0) scal[4] = mpw([&](int i) { return rep[i]; }, N);
        __syncthreads();
        for (int j = tid; j < E; j += MT) {
            double acc;
            if (E == 1) {
                acc = mpw([&](int i) { return F[i * E + j] * rep[i]; }, N);
            } else {
                acc = F[j] * rep[0];
                for (int i = 1; i < N; i++) acc = acc + F[i * E + j] * rep[i];
            }
            mu[j] = acc / scal[4];
        }
        __syncthreads();
        MSTAMP(5);
        // --- a6: covariance (:326), lower triangle mirrored: one 4 x 4 tile (J >= K) per thread,
        // rows staged through the work region in chunks (A = (F - mu) * tok, D = F - mu), each
        // entry's fma chain in row order
        {
            const double denom = scal[1];
            const int nT = (E + 3) >> 2, ntiles = nT * (nT + 1) / 2;
            int tJ = 0, tK = tid;
            while (tK > tJ) {
                tK -= tJ + 1;
                tJ++;
            }
            double acc[4][4];
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[p][q] = 0.0;
            int CR = PCX_MROUND_WORK / (2 * E);
            CR = CR > 32 ? 32 : CR;
            double* Al = mlds;
            double* Dl = mlds + CR * E;
            for (int c0 = 0; c0 < N; c0 += CR) {
                const int cr = N - c0 < CR ? N - c0 : CR;
                for (int idx = tid; idx < cr * E; idx += MT) {
                    const int i = c0 + idx / E, j = idx % E;
                    const double d = F[i * E + j] - mu[j];
                    Dl[idx] = d;
                    Al[idx] = d * tok[i];
                }
                __syncthreads();
                if (tid < ntiles)
                    for (int r = 0; r < cr; r++) {
                        double av[4], dv[4];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int j = 4 * tJ + q, k = 4 * tK + q;
                            av[q] = j < E ? Al[r * E + j] : 0.0;
                            dv[q] = k < E ? Dl[r * E + k] : 0.0;
                        }
#pragma unroll
                        for (int p = 0; p < 4; p++)
#pragma unroll
                            for (int q = 0; q < 4; q++) acc[p][q] = fma(av[p], dv[q], acc[p][q]);
                    }
                __syncthreads();
            }
            if (tid < ntiles)
#pragma unroll
                for (int p = 0; p < 4; p++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int j = 4 * tJ + p, k = 4 * tK + q;
                        if (j < E && k <= j) {
                            const double c = acc[p][q] / denom;
                            C[j * E + k] = c;
                            C[k * E + j] = c;
                        }
                    }
        }
        __syncthreads();
        MSTAMP(6);
        // --- a7: power iteration (SPEC power_iter)
        int finite = 1, nonzero = 0;
        for (int e = tid; e < E * E; e += MT) {
            finite &= __builtin_isfinite(C[e]) ? 1 : 0;
            nonzero |= C[e] != 0.0 ? 1 : 0;
        }
        finite = __syncthreads_and(finite);
        nonzero = __syncthreads_or(nonzero);
        double* x = VEp(VE_X);
        if (!finite) {
            for (int j = tid; j < E; j += MT) x[j] = 1.0;
            flags |= PCX_FLAG_SVD_FAIL;
        } else if (!nonzero) {
            for (int j = tid; j < E; j += MT) x[j] = j == 0 ? 1.0 : 0.0;
            flags |= PCX_FLAG_ZERO_COV;
        } else {
            if (tid == 0) {
                int kd = 0;
                for (int j = 1; j < E; j++)
                    if (C[j * E + j] > C[kd * E + kd]) kd = j;
                scal[5] = (double)kd;
            }
            __syncthreads();
            if (tid < 64) {
                const int kd0 = (int)scal[5];
                const double t = sqrt(wtree64([&](int j) { const double v = C[j * E + kd0]; return v * v; }, E));
                if (tid == 0) scal[6] = t;
            }
            __syncthreads();
            const int kd = (int)scal[5];
            for (int j = tid; j < E; j += MT) x[j] = C[j * E + kd] / scal[6];
            for (int e = tid; e < E * E; e += MT) M[(e / E) * ES + e % E] = C[e];
            __syncthreads();
            auto square = [&]() {  // M <- (M M) * 2^-ilogb(max|MM|): one 4 x 4 tile per thread
                // (E <= 64: at most 16 x 16 tiles, one per thread; the product stays in registers
                // across the block max, then overwrites M)
                double lm = 0.0;
                const int nT = (E + 3) >> 2, J = tid / nT, K = tid % nT;
                const bool own = tid < nT * nT;
                double acc[4][4];
#pragma unroll
                for (int p = 0; p < 4; p++)
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[p][q] = 0.0;
                if (own) {
                    for (int l = 0; l < E; l++) {
                        double mr[4], mc[4];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int j = 4 * J + q, k = 4 * K + q;
                            mr[q] = j < E ? M[j * ES + l] : 0.0;
                            mc[q] = k < E ? M[l * ES + k] : 0.0;
                        }
#pragma unroll
                        for (int p = 0; p < 4; p++)
#pragma unroll
                            for (int q = 0; q < 4; q++) acc[p][q] = fma(mr[p], mc[q], acc[p][q]);
                    }
#pragma unroll
                    for (int p = 0; p < 4; p++)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const double v = fabs(acc[p][q]);
                            if (4 * J + p < E && 4 * K + q < E && v > lm) lm = v;
                        }
                }
                const double mx = bmax(lm, sh);  // (its barriers: every read of M is done)
                const bool pow2 = mx >= M_DBL_MIN && __builtin_isfinite(mx);
                const double sc = pow2 ? ldexp(1.0, -ilogb(mx)) : 1.0;
                if (own)
#pragma unroll
                    for (int p = 0; p < 4; p++)
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const int j = 4 * J + p, k = 4 * K + q;
                            const double t = acc[p][q];
                            if (j < E && k < E) M[j * ES + k] = pow2 ? t * sc : (mx > 0.0 ? t / mx : t);
                        }
                __syncthreads();
            };
            int sqn = 0;
            for (; sqn < M_PI_PRESQUARE; sqn++) square();
            MSTAMP(28);
            // the power steps between squarings and the polish on wave 0: lane j = row j, x in
            // registers (x_k broadcast by readlane), tree64 norm and max-norm by shuffles
            __shared__ int pi_s[3];
            auto step = [&](const double* A, int lda, double xr) {  // (A x) / ||A x||
                const int row = lane < E ? lane : 0;
                double acc = 0.0;
                for (int k = 0; k < E; k++) acc = fma(A[row * lda + k], mbcast(xr, k), acc);
                const double yv = lane < E ? acc : 0.0;
                const double t = mbcast(sqrt(wtree64v(yv * yv)), 0);
                return yv / t;
            };
            int since = 0;
            for (;;) {
                if (wv == 0) {
                    double xr = lane < E ? x[lane] : 0.0;
                    int it = iters, sn = since, st = 0;
                    for (;;) {
                        const double yn = step(M, ES, xr);
                        double dl = lane < E ? fabs(yn - xr) : 0.0;
                        for (int s2 = 1; s2 < 64; s2 <<= 1) dl = fmax(dl, __shfl_xor(dl, s2, 64));
                        xr = yn;
                        it++;
                        sn++;
                        if (dl <= M_PI_TOL) {
                            st = 1;
                            break;
                        }
                        if (it >= M_PI_MAXIT) {
                            st = 2;
                            break;
                        }
                        if (sn >= M_PI_SQUARE_EVERY && sqn < M_PI_MAX_SQUARINGS) break;
                    }
                    if (lane < E) x[lane] = xr;
                    if (lane == 0) {
                        pi_s[0] = st;
                        pi_s[1] = it;
                        pi_s[2] = sn;
                    }
                }
                __syncthreads();
                const int st = pi_s[0];
                iters = pi_s[1];
                since = pi_s[2];
                __syncthreads();
                if (st == 1) break;
                if (st == 2) {
                    flags |= PCX_FLAG_PI_MAXIT;
                    break;
                }
                square();
                sqn++;
                since = 0;
            }
            MSTAMP(29);
            for (int e = tid; e < E * E; e += MT) M[(e / E) * ES + e % E] = C[e];  // C into LDS
            __syncthreads();
            if (wv == 0) {
                double xr = lane < E ? x[lane] : 0.0;
                for (int p = 0; p < M_PI_POLISH; p++) xr = step(M, ES, xr);
                if (lane < E) x[lane] = xr;
            }
            __syncthreads();
            iters += M_PI_POLISH + sqn;  // SPEC: steps + polish + squarings
            if (tid == 0) {  // SPEC sign rule
                int f = -1, nnz = 0;
                for (int j = 0; j < E; j++)
                    if (x[j] != 0.0) {
                        nnz++;
                        if (f < 0) f = j;
                    }
                const bool neg = nnz == 1 ? x[f] < 0.0 : x[f] > 0.0;
                scal[8] = neg ? 1.0 : 0.0;
            }
            __syncthreads();
            if (scal[8] != 0.0)
                for (int j = tid; j < E; j += MT) x[j] = -x[j];
        }
        __syncthreads();
        if (tid == 0) scal[9] = sqrt(mpw([&](int j) { return x[j] * x[j]; }, E));
        __syncthreads();
        for (int j = tid; j < E; j += MT) loading[j] = x[j] / scal[9];
        __syncthreads();
        MSTAMP(7);
        if (clustering) {
            // scores stay zeros
        } else if (alg == PCX_ALG_PCA) {
            for (int i = tid; i < N; i += MT) {  // scores (:337)
                double acc = 0.0;
                for (int j = 0; j < E; j++) acc = fma(F[i * E + j] - mu[j], loading[j], acc);
                s[i] = acc;
            }
        } else if (flags & PCX_FLAG_SVD_FAIL) {  // the reference's second svd raises (:375, :431)
            for (int i = tid; i < N; i += MT) s[i] = __builtin_nan("");
        } else {
            comps = component_scores(PCX_MROUND_ARGS, C, M, Tm, ES, F, mu, s, sh, scal);
        }
    } else if (alg == PCX_ALG_COKURTOSIS) {
        for (int i = tid; i < N; i += MT) s[i] = a.aux_scores[PCX_MROUND_ROW0 + i];
    }
    __syncthreads();
    MSTAMP(8);
    if (clustering) {
#if !PCX_MEDIUM_TALL
        // --- nc from the clusters (SPEC hier_nc / kmeans_nc / feck_nc); the work region is free
        double* X = Xscr + PCX_MROUND_XSLOT;
        if (alg == PCX_ALG_HIERARCHICAL)
            mhier_nc(F, VEp(VE_MU), N, E, a.hierarchy_threshold, X, mlds, nc);
#if !PCX_MEDIUM_RAGGED  // (a ragged launch refuses k-means: its code-book size depends on the round's N)
        else if (alg == PCX_ALG_KMEANS)
            mkmeans_nc(a, b, F, VEp(VE_MU), N, E, X, mlds, nc, scal);
#elif PCX_MEDIUM_RAGGED == 3  // (the round's own books: a.kmeans_init points at them)
        else if (alg == PCX_ALG_KMEANS)
            mkmeans_nc(a, 0, F, VEp(VE_MU), N, E, X, mlds, nc, scal);
#endif
        else
            mfeck_nc(a, F, tok, N, E, X, mlds, nc, scal);
#endif
    } else if (alg != PCX_ALG_ABSOLUTE) {
        // --- a8/a9: nonconformity_rank (:487-500), tie -> nonconformity (:475-485)
        double* set1 = VNp(VN_SET1);
        double* set2 = VNp(VN_SET2);
        double* n1 = VNp(VN_NW1);
        double* n2 = VNp(VN_NW2);
        if (tid == 0) {  // NaN propagates like np.min / np.max
            double mn = s[0], mx = s[0];
            auto upd = [&](double v) {
                if (__builtin_isnan(v) || v < mn) mn = __builtin_isnan(mn) ? mn : v;
                if (__builtin_isnan(v) || v > mx) mx = __builtin_isnan(mx) ? mx : v;
            };
            int i = 1;
            for (; i + 8 <= N; i += 8) {  // in row order, loads eight ahead
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; q++) v[q] = s[i + q];
#pragma unroll
                for (int q = 0; q < 8; q++) upd(v[q]);
            }
            for (; i < N; i++) upd(s[i]);
            scal[10] = mn;
            scal[11] = mx;
        }
        __syncthreads();
        for (int i = tid; i < N; i += MT) {
            set1[i] = s[i] + fabs(scal[10]);
            set2[i] = s[i] - scal[11];
        }
        __syncthreads();
        if (tid == 0) {  // normalize (:244-249); the two sets on two waves
            double S1 = mpw([&](int i) { return fabs(set1[i]); }, N);
            scal[12] = S1;
            scal[13] = S1 == 0 ? mpw([&](int i) { return fabs(set1[i]) + 1.0; }, N) : S1;
        } else if (tid == 64) {
            double S2 = mpw([&](int i) { return fabs(set2[i]); }, N);
            scal[14] = S2;
            scal[15] = S2 == 0 ? mpw([&](int i) { return fabs(set2[i]) + 1.0; }, N) : S2;
        }
        __syncthreads();
        MSTAMP(24);
        for (int i = tid; i < N; i += MT) {
            n1[i] = scal[12] == 0 ? (fabs(set1[i]) + 1.0) / scal[13] : fabs(set1[i]) / scal[13];
            n2[i] = scal[14] == 0 ? (fabs(set2[i]) + 1.0) / scal[15] : fabs(set2[i]) / scal[15];
        }
        __syncthreads();
        double* old = VEp(VE_OLD);
        MSTAMP(25);
        PCX_MROUND_VECMAT([&](int i) { return n1[i]; }, VEp(VE_D1));
        __syncthreads();
        PCX_MROUND_VECMAT([&](int i) { return n2[i]; }, VEp(VE_D2));
        __syncthreads();
        for (int j = tid; j < E; j += MT) {
            const double a1 = VEp(VE_D1)[j], a2 = VEp(VE_D2)[j];
            const double t = 0.01 * old[j];
            VEp(VE_NEW1)[j] = a1 + t;
            VEp(VE_NEW2)[j] = a2 + t;
        }
        __syncthreads();
        MSTAMP(26);
        double ref = 0.0;
        if (alg == PCX_ALG_PCA) {
            double* nw1 = VEp(VE_NEW1);
            double* nw2 = VEp(VE_NEW2);
            for (int j = tid; j < E; j += MT) {
                int lt0 = 0, eq0 = 0, lt1 = 0, eq1 = 0, lt2 = 0, eq2 = 0;
                const double o = old[j], v1 = nw1[j], v2 = nw2[j];
                auto cnt = [&](double a0, double a1, double a2) {
                    lt0 += a0 < o;
                    eq0 += a0 == o;
                    lt1 += a1 < v1;
                    eq1 += a1 == v1;
                    lt2 += a2 < v2;
                    eq2 += a2 == v2;
                };
                int k = 0;
                for (; k + 8 <= E; k += 8) {  // broadcast loads eight ahead
                    double b0[8], b1[8], b2[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        b0[q] = old[k + q];
                        b1[q] = nw1[k + q];
                        b2[q] = nw2[k + q];
                    }
#pragma unroll
                    for (int q = 0; q < 8; q++) cnt(b0[q], b1[q], b2[q]);
                }
                for (; k < E; k++) cnt(old[k], nw1[k], nw2[k]);
                const double r0 = (double)lt0 + (double)(eq0 + 1) * 0.5;
                const double r1 = (double)lt1 + (double)(eq1 + 1) * 0.5;
                const double r2 = (double)lt2 + (double)(eq2 + 1) * 0.5;
                // rankdata propagates NaN (every rank NaN): a NaN value makes the rule's sums NaN
                const bool nan = __builtin_isnan(o) || __builtin_isnan(v1) || __builtin_isnan(v2);
                VEp(VE_E1)[j] = nan ? __builtin_nan("") : fabs(r1 - r0);
                VEp(VE_E2)[j] = nan ? __builtin_nan("") : fabs(r2 - r0);
            }
            __syncthreads();
            if (tid == 0)
                scal[2] = mpw([&](int j) { return VEp(VE_E1)[j]; }, E) - mpw([&](int j) { return VEp(VE_E2)[j]; }, E);
            __syncthreads();
            ref = scal[2];
            __syncthreads();
        }
        MSTAMP(27);
        int pick1;
        if (ref == 0) {
            if (tid == 0) {
                const double* d1 = VEp(VE_D1);
                const double* d2 = VEp(VE_D2);
                const double q1 = mpw([&](int j) { const double v = d1[j] - old[j]; return v * v; }, E);
                const double q2 = mpw([&](int j) { const double v = d2[j] - old[j]; return v * v; }, E);
                scal[3] = (q1 - q2) <= 0 ? 1.0 : 0.0;
            }
            __syncthreads();
            pick1 = scal[3] != 0.0;
            branch = pick1 ? PCX_BRANCH_TIE_SET1 : PCX_BRANCH_TIE_SET2;
        } else {
            pick1 = ref < 0;
            branch = pick1 ? PCX_BRANCH_SET1 : PCX_BRANCH_SET2;
        }
        for (int i = tid; i < N; i += MT) nc[i] = pick1 ? set1[i] : set2[i];
    }
    __syncthreads();
    MSTAMP(9);
    // --- a10: reputation update (:460-472)
    double* thisr = VNp(VN_THIS);
    double* smooth = VNp(VN_SMOOTH);
    if (tid == 0) scal[4] = mpw([&](int i) { return rep[i]; }, N) / (double)N;
    __syncthreads();
    for (int i = tid; i < N; i += MT) nc[i] = nc[i] * (rep[i] / scal[4]);  // u (nc no longer needed)
    __syncthreads();
    if (tid == 0) {
        const double S = mpw([&](int i) { return fabs(nc[i]); }, N);
        scal[5] = S;
        scal[6] = S == 0 ? mpw([&](int i) { return fabs(nc[i]) + 1.0; }, N) : S;
    }
    __syncthreads();
    for (int i = tid; i < N; i += MT) {
        const double t = scal[5] == 0 ? (fabs(nc[i]) + 1.0) / scal[6] : fabs(nc[i]) / scal[6];
        thisr[i] = t;
        smooth[i] = a.alpha * t + (1.0 - a.alpha) * rep[i];
    }
    __syncthreads();
    MSTAMP(10);
    // --- a12/a13: outcomes (:510-538)
    double* raw = VEp(VE_RAW);
    double* adj = VEp(VE_ADJ);
    double* fin = VEp(VE_FIN);
    PCX_MROUND_VECMAT([&](int i) { return smooth[i]; }, raw);
    __syncthreads();
    for (int j = tid; j < E; j += MT) {
        if (!scaled(j)) {
            adj[j] = mcatch(raw[j], a.catch_tol);
            fin[j] = adj[j];
        }
    }
    __syncthreads();
    MSTAMP(11);
    for (int c = PCX_MROUND_WV0(nscl); c < nscl; c += PCX_MROUND_MWAVES) {  // one wave per scaled column
        const int j = scl[c];
        for (int i = lane; i < N; i += 64) wb[i] = F[i * E + j];
        mwsync();
        const double r = wv_wmedian(wb, smooth, N, wb + 2 * N, PN, a.stamps ? mprof : nullptr);
        if (lane == 0) {
            raw[j] = r;
            adj[j] = r;
            double f = r * (a.hi[bo + j] - a.lo[bo + j]);
            f = f + a.lo[bo + j];
            fin[j] = f;
        }
    }
    __syncthreads();
    MSTAMP(12);
    // --- a14: certainty (:540-546): sum of smooth over the matching rows (pairwise), per event
    double* cert = VEp(VE_CERT);
    for (int j = PCX_MROUND_WV0(E); j < E; j += PCX_MROUND_MWAVES) {  // one wave per event: the matching rows' weights in row order
        const double aj = adj[j];
        int m = 0;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            const bool p = i < N && F[i * E + j] == aj;
            const unsigned long long bal = __ballot(p);
            if (p) wb[m + __popcll(bal & ((1ull << lane) - 1ull))] = smooth[i];
            m += __popcll(bal);
        }
        mwsync();
        if (lane == 0)
            cert[j] = m ? mpw([&](int q) { return wb[q]; }, m) : (alg == PCX_ALG_PCA ? __builtin_nan("") : 0.0);
        mwsync();
    }
    __syncthreads();
    MSTAMP(13);
    double* reward = VEp(VE_REWARD);
    double* pc = VEp(VE_PC);
    double* relc = VEp(VE_RELC);
    if (tid == 64) {  // (wave 1: wave 0 runs the participation columns meanwhile)
        const double S = mpw([&](int j) { return fabs(cert[j]); }, E);
        const double Sp = S == 0 ? mpw([&](int j) { return fabs(cert[j]) + 1.0; }, E) : S;
        for (int j = 0; j < E; j++) reward[j] = S == 0 ? (fabs(cert[j]) + 1.0) / Sp : fabs(cert[j]) / Sp;
        scal[7] = mpw([&](int j) { return cert[j]; }, E) / (double)E;  // avg certainty
    }
    // --- a15: participation and bonuses (:549-581)
    for (int j = tid; j < E; j += MT) {
        pc[j] = 1.0 - mdot2([&](int i) { return smooth[i]; }, [&](int i) { return FL(i * E + j) ? 1.0 : 0.0; }, N);
        int nz = 0;
        for (int i = 0; i < N; i++) nz += (FL(i * E + j) & 2) ? 1 : 0;
        if (a.nas_filled) a.nas_filled[PCX_MROUND_EV0 + j] = (double)nz;
    }
    __syncthreads();
    MSTAMP(14);
    double* pr = VNp(VN_SET1);  // reuse
    double* narow = VNp(VN_SET2);
    double* rel = VNp(VN_NW1);
    double* a2v = VNp(VN_NW2);
    double* rmask = VNp(VN_XS);
    for (int i = tid; i < N; i += MT) {
        int nz = 0, nn = 0;
        for (int j = 0; j < E; j++) {
            nz += (FL(i * E + j) & 2) ? 1 : 0;
            nn += (FL(i * E + j) & 1) ? 1 : 0;
        }
        narow[i] = (double)nz;
        pr[i] = 1.0 - narow[i] / (double)E;
        rmask[i] = nn == E ? 1.0 : 0.0;  // Q15: a fully NaN row is masked
        a2v[i] = rmask[i] != 0.0 ? 0.0 : fabs(pr[i]);
    }
    __syncthreads();
    if (tid == 0) {  // the three totals on three waves
        scal[8] = 1.0 - mpw([&](int j) { return pc[j]; }, E) / (double)E;  // pna
    } else if (tid == 64) {
        double S = mpw([&](int i) { return a2v[i]; }, N);
        const bool bump = S == 0;
        if (bump) S = mpw([&](int i) { return rmask[i] != 0.0 ? 0.0 : fabs(pr[i]) + 1.0; }, N);
        scal[9] = S;
        scal[10] = bump ? 1.0 : 0.0;
    } else if (tid == 128) {
        const double P = mpw([&](int j) { return fabs(pc[j]); }, E);
        const double Pp = P == 0 ? mpw([&](int j) { return fabs(pc[j]) + 1.0; }, E) : P;
        for (int j = 0; j < E; j++) relc[j] = P == 0 ? (fabs(pc[j]) + 1.0) / Pp : fabs(pc[j]) / Pp;
    }
    __syncthreads();
    const double pna = scal[8];
    // PCA: a NaN total of |u| (scal[5]) leaves the reference's this_rep / smooth_rep fully MASKED
    // (SPEC rep_masked: participation_columns, reporter_bonus, author_bonus are numpy.ma's data)
    const bool rep_masked = alg == PCX_ALG_PCA && __builtin_isnan(scal[5]);
    for (int i = tid; i < N; i += MT) {
        const bool masked = rmask[i] != 0.0;
        const double ai = masked ? 0.0 : fabs(pr[i]) + (scal[10] != 0.0 ? 1.0 : 0.0);
        rel[i] = masked ? fabs(pr[i]) : ai / scal[9];
        const int64_t o = PCX_MROUND_ROW0 + i;
        if (a.old_rep) a.old_rep[o] = rep[i];
        if (a.this_rep) a.this_rep[o] = thisr[i];
        if (a.smooth_rep) a.smooth_rep[o] = smooth[i];
        if (a.scores) a.scores[o] = s[i];
        if (a.na_row) a.na_row[o] = narow[i];
        if (a.participation_rows) a.participation_rows[o] = pr[i];
        if (a.relative_part) a.relative_part[o] = rel[i];
        if (a.reporter_bonus) a.reporter_bonus[o] = (masked || rep_masked) ? rel[i] : rel[i] * pna + smooth[i] * (1.0 - pna);
    }
    for (int j = tid; j < E; j += MT) {
        const int64_t o = PCX_MROUND_EV0 + j;
        if (a.adj_first_loadings) a.adj_first_loadings[o] = loading[j];
        if (a.outcomes_raw) a.outcomes_raw[o] = raw[j];
        if (a.outcomes_adjusted) a.outcomes_adjusted[o] = adj[j];
        if (a.outcomes_final) a.outcomes_final[o] = fin[j];
        if (a.certainty) a.certainty[o] = cert[j];
        if (a.consensus_reward) a.consensus_reward[o] = reward[j];
        if (a.participation_columns) a.participation_columns[o] = rep_masked ? 1.0 : pc[j];
        if (a.author_bonus) a.author_bonus[o] = rep_masked ? 1.0 : relc[j] * pna + reward[j] * (1.0 - pna);
    }
    MSTAMP(15);
    if (a.stamps && tid == 0)
        for (int k = 0; k < 3; k++) a.stamps[b * 32 + 20 + k] = mprof[k];
    if (tid == 0) {
        if (a.participation) a.participation[b] = 1.0 - pna;
        if (a.avg_certainty) a.avg_certainty[b] = scal[7];
        if (a.branch) a.branch[b] = branch;
        if (a.flags) a.flags[b] = flags;
        if (a.pi_iters) a.pi_iters[b] = iters;
        if (a.components) a.components[b] = comps;
    }
}
#undef PCX_MROUND_CELL0
#undef PCX_MROUND_ROW0
#undef PCX_MROUND_EV0
#undef PCX_MROUND_BO
#undef PCX_MROUND_FSLOT
#undef PCX_MROUND_CSLOT
#undef PCX_MROUND_XSLOT
#undef PCX_MROUND_ARGS
#undef PCX_MROUND_REGION
#undef PCX_MROUND_WORK
#undef PCX_MROUND_MWAVES
#undef PCX_MROUND_WV0
#undef PCX_MROUND_VECMAT
