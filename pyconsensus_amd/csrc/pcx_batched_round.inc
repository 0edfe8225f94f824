// pcx_batched_round.inc -- the round kernel's text, included twice by pcx_batched.hip: as
// batched_round_kernel (PCX_ROUND_RAGGED 0: B rounds of one shape) and as ragged_round_kernel
// (PCX_ROUND_RAGGED 1: a shape per round), and once by pcx_batched_params.hip (PCX_ROUND_RAGGED 2,
// below).  One text under two kernel names keeps the equal-shape
// instantiations' code exactly what it was (a shared __device__ body, inlined, compiled the 50 x 20
// kernels to different register and scratch counts), and the two cannot drift apart.
//
// NT/ET > 0: the round shape is a compile-time constant (the Monte Carlo shapes the
// launcher specialises, e.g. the 50 x 20 of config C3): every loop bound is known, so
// the sequential column/row loops unroll and their LDS reads issue ahead of the
// dependent adds.  NT = ET = 0: any N <= 64, E <= 32 at run time.  Same arithmetic.
//
// Ragged (NT = ET = 0 only): round b's shape and the offsets of its cells, reporters and events in
// the flat inputs and outputs come from rag[b] (RaggedDesc) in place of a.N / a.E and b * N * E,
// b * N, b * E.  The descriptor is wave-uniform: it is read once and held in scalar registers
// (readfirstlane), so the loop bounds and branches on N and E stay on the scalar unit as they do for
// the kernel arguments.  The round carves its LDS from its own N, E and ES = E | 1 and never reaches
// past that carve; the launch allocates the largest round's.  The [B] outputs stay at b.
//
// Per-round parameters (PCX_ROUND_RAGGED 2, pcx_batched_params.hip: ragged_params_round_kernel,
// DESIGN.md 5.4.3): the ragged form over MediumDesc, whose `param` picks the round's entry of a
// device table RoundParams[P] and whose `round` is where the six [B] outputs go (a launch holds the
// rounds of one instantiation group, in any subset and order).  The entry is wave-uniform like the
// descriptor: read once, held in scalar registers, written over the seven parameter fields of a
// local copy `a` of the kernel argument `ka`, which the text below reads as it reads the argument in
// the other two forms.  (out_args() still reads the output pointers from the argument itself.)
//
// k-means (PCX_ROUND_RAGGED 3, pcx_batched_kmeans.hip: ragged_kmeans_round_kernel, DESIGN.md 5.5.2):
// the per-round-parameter form with one more wave-uniform read, the round's entry {offset, k} of a
// device table KmeansEntry[B] indexed by the round: the local copy's kmeans_k becomes the round's
// code-book size and its kmeans_init the round's own books in the flat array (kmeans_restarts is the
// call's, in the argument), so kmeans_nc reads them as it does in the equal-shape form, as round 0.
#if PCX_ROUND_RAGGED >= 2
#define PCX_ROUND_CELL0 rcell
#define PCX_ROUND_ROW0 rrow
#define PCX_ROUND_EV0 rev
#define PCX_ROUND_B rround
template <int NT, int ET, bool CLUS, bool PK>
#if PCX_ROUND_RAGGED == 3
__global__ void __launch_bounds__(64, 3) ragged_kmeans_round_kernel(BatchArgs ka, const MediumDesc* __restrict__ rag,
                                                                    const RoundParams* __restrict__ ptab,
                                                                    const KmeansEntry* __restrict__ ktab) {
#else
__global__ void __launch_bounds__(64, 3) ragged_params_round_kernel(BatchArgs ka, const MediumDesc* __restrict__ rag,
                                                                    const RoundParams* __restrict__ ptab) {
#endif
    static_assert(NT == 0 && ET == 0, "a ragged launch has no compiled shape");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const MediumDesc* const rd = rag + blockIdx.x;
    const int N = __builtin_amdgcn_readfirstlane(rd->N), E = __builtin_amdgcn_readfirstlane(rd->E), ES = E | 1;
    const int64_t rcell = uniform64(rd->cell), rrow = uniform64(rd->row), rev = uniform64(rd->ev);
    const int64_t rround = __builtin_amdgcn_readfirstlane(rd->round);
    const RoundParams* const rp = ptab + __builtin_amdgcn_readfirstlane(rd->param);
    BatchArgs a = ka;
    a.algorithm = __builtin_amdgcn_readfirstlane(rp->algorithm);
    a.max_components = __builtin_amdgcn_readfirstlane(rp->max_components);
    a.catch_tol = uniform_f64(rp->catch_tol);
    a.alpha = uniform_f64(rp->alpha);
    a.variance_threshold = uniform_f64(rp->variance_threshold);
    a.hierarchy_threshold = uniform_f64(rp->hierarchy_threshold);
    a.cluster_threshold = uniform_f64(rp->cluster_threshold);
#if PCX_ROUND_RAGGED == 3
    const KmeansEntry* const ke = ktab + rround;
    a.kmeans_k = __builtin_amdgcn_readfirstlane(ke->k);
    a.kmeans_init = ka.kmeans_init + uniform64(ke->offset);
#endif
#elif PCX_ROUND_RAGGED
#define PCX_ROUND_CELL0 rcell
#define PCX_ROUND_ROW0 rrow
#define PCX_ROUND_EV0 rev
#define PCX_ROUND_B blockIdx.x
template <int NT, int ET, bool CLUS, bool PK>
__global__ void __launch_bounds__(64, 3) ragged_round_kernel(BatchArgs a, const RaggedDesc* __restrict__ rag) {
    static_assert(NT == 0 && ET == 0, "a ragged launch has no compiled shape");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const RaggedDesc* const rd = rag + blockIdx.x;
    const int N = __builtin_amdgcn_readfirstlane(rd->N), E = __builtin_amdgcn_readfirstlane(rd->E), ES = E | 1;
    const int64_t rcell = uniform64(rd->cell), rrow = uniform64(rd->row), rev = uniform64(rd->ev);
#else
#define PCX_ROUND_CELL0 (b * (int64_t)N * E)
#define PCX_ROUND_ROW0 (b * N)
#define PCX_ROUND_EV0 (b * E)
#define PCX_ROUND_B blockIdx.x
template <int NT, int ET, bool CLUS, bool PK>
__global__ void __launch_bounds__(64, (NT > 0 && PK) ? PACKED_WAVES : 3) batched_round_kernel(BatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int N = NT > 0 ? NT : a.N, E = ET > 0 ? ET : a.E, ES = ET > 0 ? compiled_es(ET) : a.ES;
#endif
    const int l = lane_id();
    const int64_t b = PCX_ROUND_B;
    constexpr int NRM = NT > 0 ? NT : 64;  // median scratch rows
    Smem S = carve(smem, N, E, ES, NRM, PK);
    const bool row = l < N, col = l < E;
    const int64_t bo = a.bounds_shared ? 0 : PCX_ROUND_EV0;
    const bool has_bounds = a.scaled != nullptr;
    // Whether the call gave reputations.  The compiled shapes read a flag formed here: testing the pointer
    // at each site, with the rescale's row held in registers, the scalar allocator gave up the kernel's first
    // eight-register argument load after the round's load and fetched it again for the test, and kept the
    // 32-byte stack slot of the spill it had planned.  The other forms test the pointer where they did.
    constexpr bool REPFLAG = NT > 0 && ET > 0;
    const bool rep_flag = REPFLAG && a.reputation != nullptr;
    // numpy's pairwise sum over the reporters' / the events' lanes: both are prefixes of the wave
    // (of compile-time length in a compiled shape).  The row sums stage their values in the head of
    // the "M" region, N doubles (2 N for a pair), dead at every one of their sites (DESIGN.md 5.2,
    // "Pairwise sums with the chains in lanes 0..7"): see wave_pw_sum_lds; the column sums of fewer
    // than 24 events run in registers, see wave_pw_sum_dpp.
    auto pw_rows = [&](double v) { return wave_pw_sum_lds<NT>(v, N, S.M); };
    auto pw_rows2 = [&](double v1, double v2, double& s1, double& s2) { wave_pw_sum2_lds<NT>(v1, v2, N, S.M, s1, s2); };
    auto pw_cols = [&](double v) { return wave_pw_sum_dpp<ET>(v, E); };
    constexpr int CR = live_rows(ET);  // 16-lane rows that hold events (a compiled shape's; else all four)

    // The output pointers are read from the kernel-argument segment where they are used (scalar
    // loads, the segment's address made opaque at each use): as fields of `a` all of them are
    // fetched at kernel entry and held -- 60 scalar registers spilled to lanes until the epilogue.
    typedef const __attribute__((address_space(4))) BatchArgs* KernArgs;
    auto out_args = [&]() -> KernArgs {
        uint64_t p = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();  // `a` is the first argument: offset 0
        asm volatile("" : "+s"(p));
        return (KernArgs)p;
    };

    long long mprof[3] = {0, 0, 0};  // diagnostic: median sort / walk cycles (PCX_STAMPS)
    STAMP(0);
    // ---- load the round -------------------------------------------------
    const double* Rg = a.reports + PCX_ROUND_CELL0;
    bool scj = false;
    double loj = 0.0, hij = 0.0;
    if (col && has_bounds) {
        scj = a.scaled[bo + l] != 0;
        loj = a.lo[bo + l];
        hij = a.hi[bo + l];
    }
    double raw = row && (REPFLAG ? rep_flag : a.reputation != nullptr) ? a.reputation[PCX_ROUND_ROW0 + l] : 0.0;
    if constexpr (NT > 0 && ET > 0 && (NT * ET) % 2 == 0) {
        // every 16-byte load of the round in flight at once, then the LDS scatter
        constexpr int TOT2 = NT * ET / 2, NV = (TOT2 + W - 1) / W;
        double2 v[NV];
#pragma unroll
        for (int q = 0; q < NV; q++)
            if (l + W * q < TOT2) v[q] = reinterpret_cast<const double2*>(Rg)[l + W * q];
#pragma unroll
        for (int q = 0; q < NV; q++) {
            const int idx = 2 * (l + W * q);
            if (idx < NT * ET) {
                const int i0 = idx / ET, j0 = idx - i0 * ET;
                const int i1 = (idx + 1) / ET, j1 = idx + 1 - i1 * ET;
                S.F[i0 * ES + j0] = v[q].x;
                S.F[i1 * ES + j1] = v[q].y;
            }
        }
    } else {
        for (int idx = l; idx < N * E; idx += W) {
            const int i = idx / E, j = idx - i * E;
            S.F[i * ES + j] = Rg[idx];
        }
    }
    const uint64_t scaled_mask = ballot(col && scj);

    // ---- a1: reputation (__init__.py:138-146) -----------------------------
    double rep;
    if (REPFLAG ? rep_flag : a.reputation != nullptr) {
        const double tot = pw_rows(raw);
        rep = raw / tot;
    } else {
        rep = 1.0 / (double)N;
    }
    const double tok = trunc(rep * 1e6);
    if (row) S.rep[l] = rep;
    const double denom = tree_sum(row ? tok : 0.0) - 1.0;  // exact integer sum
    wsync();

    STAMP(1);
    // ---- a2: rescale (:266-269) + NA masks (:278) -------------------------
    // (the next column's value is loaded before this column's stores: a load after a store to
    // the same LDS array would otherwise wait for it)
    // per-lane counts, 7 bits each: row l's zeros (bits 0-7) and NaNs (8-15), column l's zeros (16-23)
    uint32_t nacnt = 0;
    // Each row lane collects its own row's NaN / zero columns as bits of two 32-bit masks straight
    // from the compares (E <= 32), and lane j takes column j's zero count when column j is visited,
    // so a column's two ballots die with it.  (Summed from the ballots' bits instead, the whole
    // accumulation sank to its first use after the certainty, and forty ballots waited for it in
    // spilled scalar registers.)
    // Only a scaled column (a wave-uniform branch on scaled_mask) fetches its bounds and divides,
    // and the lanes past the last row hold 1.0, neither NaN nor zero, so the compares are the
    // ballots with no row mask applied.
    uint32_t nanb = 0, zerob = 0;
    int zcol = 0;  // column l's zero count (lanes < E)
    constexpr bool ROWREG = NT > 0 && ET > 0;  // the compiled shapes: column loops over a register-held row
    uint32_t missb = 0;                        // ROWREG: row l's missing columns (nanb | zerob), kept for the fill
    uint32_t mjlo = 0, mjhi = 0;               // ROWREG: column l's missing rows, the two halves of miss[l]
    if constexpr (ROWREG) {
        // The row lane reads its whole row in one batch of 16-byte reads (the compiled pitch is even, so
        // every row starts on 16 bytes) and the column loop runs from registers: no LDS read, no wait
        // and no per-column address in it.  Column j's two scalars go to lane j by v_writelane_b32: its
        // zero count, and the two halves of its missing mask, which lane j stores as miss[j] once after
        // the loop and keeps as miss_j (lane 0 stored each from under its own EXEC pair, and the next
        // column's wait on its load waited for that store too).
        static_assert(compiled_es(ET) % 2 == 0, "16-byte row reads");
        double xr[ET];
#pragma unroll
        for (int j = 0; j < ET; j++) xr[j] = 1.0;
        if (row) {
            const double2* const Fr = reinterpret_cast<const double2*>(S.F + l * ES);
#pragma unroll
            for (int q = 0; q < ET / 2; q++) {
                const double2 v = Fr[q];
                xr[2 * q] = v.x;
                xr[2 * q + 1] = v.y;
            }
            if (ET & 1) xr[ET - 1] = S.F[l * ES + ET - 1];
        }
        static_cols<0, ET>([&](auto jc) {
            constexpr int j = jc.value;
            const bool sc = (scaled_mask >> j) & 1;
            double x = xr[j];
            if (sc) {  // wave-uniform
                const double lo = bcast(loj, j), hi = bcast(hij, j);
                if (row) {
                    x = (x - lo) / (hi - lo);
                    if (a.int_dtype) x = trunc(x);
                    S.F[l * ES + j] = x;
                }
            }
            const bool xn = __builtin_isnan(x), xz = x == 0.0;
            nanb |= xn ? 1u << j : 0u;
            zerob |= xz ? 1u << j : 0u;
            const uint64_t zm = ballot(xz), mm = ballot(xn) | zm;
            zcol = (int)write_lane<j>((uint32_t)zcol, (uint32_t)popc(zm));
            mjlo = write_lane<j>(mjlo, (uint32_t)mm);
            mjhi = write_lane<j>(mjhi, (uint32_t)(mm >> 32));
            // (formed here, as below: a column's compare masks die with it)
            asm volatile("" : "+v"(nanb), "+v"(zerob), "+v"(zcol), "+v"(mjlo), "+v"(mjhi));
        });
        missb = nanb | zerob;
        if (col) S.miss[l] = ((uint64_t)mjhi << 32) | mjlo;
    } else {
    double xnext = row ? S.F[l * ES] : 1.0;
    // (the compiled shapes' loop unrolled: left rolled, as the compiler leaves it with the
    // scaled columns' branch inside, a column's load runs only one column ahead)
#pragma unroll(ET > 0 ? ET : 1)
    for (int j = 0; j < E; j++) {
        const bool sc = (scaled_mask >> j) & 1;
        double x = xnext;
        if (j + 1 < E) xnext = row ? S.F[l * ES + j + 1] : 1.0;
        if (sc) {  // wave-uniform
            const double lo = bcast(loj, j), hi = bcast(hij, j);
            if (row) {
                x = (x - lo) / (hi - lo);
                if (a.int_dtype) x = trunc(x);
                S.F[l * ES + j] = x;
            }
        }
        const bool xn = __builtin_isnan(x), xz = x == 0.0;
        nanb |= xn ? 1u << j : 0u;
        zerob |= xz ? 1u << j : 0u;
        const uint64_t zm = ballot(xz), mm = ballot(xn) | zm;
        zcol = l == j ? popc(zm) : zcol;
        if (l == 0) S.miss[j] = mm;
        // the three registers are formed here: without this the compiler sinks their updates to
        // the first use again and keeps every column's compare masks alive for them
        asm volatile("" : "+v"(nanb), "+v"(zerob), "+v"(zcol));
    }
    }
    nacnt = (uint32_t)__popc(zerob) | ((uint32_t)__popc(nanb) << 8) | ((uint32_t)zcol << 16);
    wsync();
    // result["original"] (the rescaled reports), from LDS in row-major order: every store
    // instruction writes 64 consecutive doubles (whole lines), not one column's 50 strided ones
    if (double* const og = out_args()->original) round_to_global(og + PCX_ROUND_CELL0, S.F, N, E, ES, NT, ET);

    STAMP(2);
    // ---- a3: interpolation guesses (:284-313), column phase ----------------
    uint64_t miss_j = 0;
    if constexpr (ROWREG) {
        if (col) miss_j = ((uint64_t)mjhi << 32) | mjlo;  // (lane j took column j's mask in the rescale loop)
    } else {
        if (col) miss_j = S.miss[l];
    }
    // every reputation >= 0 (a NaN fails): the condition of the row-split sums here and of the
    // prescreen below.  Equal reputations (reputation == nullptr) are 1 / N and pass.
    const bool nonneg = !ballot(row && !(rep >= 0.0));
    const bool binary_fill = col && miss_j && !scj;
    bool tot_exact;          // S.tot holds the SPEC's sequential totals (else the row-split ones)
    uint64_t need_bin = 0;   // the binary columns whose guess waits for the exact replay (below)
    {
        // The fast sums of column c over its present rows: tot = sum rep, sp = sum rep * F,
        // sa = sum |rep| * |F|.  A binary column's guess only matters through catch(): it is
        // catch(sp / tot) where that value clears both thresholds by 1e-12 * sa / tot, and the
        // SPEC's exact sequential sum is replayed otherwise (after the prescreen, below).  A
        // scaled column's tot feeds the prescreen, whose margin is 2^-16 tot; the sort divides by
        // the SPEC's sequential total, replayed with the binary columns'.
        //   Row-split (every rep >= 0 and 3 E <= 64): lane g * E + c sums column c's rows g, g + 3,
        // g + 6, ... in ascending order, and lane c takes (p0 + p1) + p2 by ds_bpermute: chains a
        // third as long on lanes that idle otherwise.  Each split sum is within (N + N / 3 + 1) u
        // of the sum of its terms' magnitudes from the sequential one (DESIGN.md 5.2), fifty times
        // inside the fast test's margin, and tot' > 0 exactly when the sequential total is (no term < 0).
        //   Otherwise the sums run on lane c over all its rows in row order (G = 1): tot is then
        // the SPEC's own.  A compiled shape's round with a negative or NaN reputation forms no
        // fast sums at all: every guess and total of it comes from the replay.
        constexpr bool SPLITC = NT > 0 && ET > 0 && 3 * ET <= W;
        const bool split = SPLITC ? nonneg : (nonneg && 3 * E <= W);
        const bool sums = SPLITC ? nonneg : true;
        tot_exact = SPLITC ? false : !split;
        double tot = 0.0, sp = 0.0, sa = 0.0;
        const int g = split ? (l >= E) + (l >= 2 * E) : 0;
        const bool live = l < (split ? 3 * E : E);
        const int c = live ? l - g * E : 0;
        // bit k of m: row g + k is missing.  Rows past N and idle lanes count as missing.
        uint64_t m = ~0ull;
        if (sums) {
            const uint64_t past = N < 64 ? ~0ull << N : 0ull;
            const uint64_t mc = split ? S.miss[c] : miss_j;
            m = live ? ((mc | past) >> g) | ~(~0ull >> g) : ~0ull;
        }
        if constexpr (SPLITC) {
            if (split) {
                // every bound, offset and bit position a constant: the loads are unconditional
                // (two rows past F's end lie in the round's own LDS, idle lanes read column 0)
                // and a missing row is zeroed by selects: rep to +0.0, F by its high word alone
                // (what is left is finite, and 0 times it is 0)
                constexpr int TS = (NT + 2) / 3;
                const double* const Fp = S.F + g * ES + c;
                const double* const rp = S.rep + g;
                const uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
#pragma unroll
                for (int t = 0; t < TS; t++) {
                    const bool miss = ((3 * t < 32 ? mlo : mhi) & (1u << ((3 * t) & 31))) != 0;
                    const double r0 = rp[3 * t];
                    const uint64_t fu = (uint64_t)__double_as_longlong(Fp[3 * t * ES]);
                    const uint32_t fh = miss ? 0u : (uint32_t)(fu >> 32);
                    const double re = miss ? 0.0 : r0;
                    const double f = __longlong_as_double((long long)(((uint64_t)fh << 32) | (uint32_t)fu));
                    tot = tot + re;
                    sp = fma(re, f, sp);
                    sa = fma(re, fabs(f), sa);
                }
            }
        } else {
            const int G = split ? 3 : 1;
            const double* const Fc = S.F + c;
            for (int k = 0; k < N; k += G) {
                const bool miss = (m >> k) & 1;
                const int i = g + k;
                const double re = miss ? 0.0 : S.rep[i];
                const double f = miss ? 0.0 : Fc[i * ES];
                tot = tot + re;
                sp = fma(re, f, sp);
                sa = fma(fabs(re), fabs(f), sa);
            }
        }
        if (split) {  // lane c: (p0 + p1) + p2
            const int l1 = (l + E) & (W - 1), l2 = (l + 2 * E) & (W - 1);
            const double t1 = bpermute_d(l1, tot), t2 = bpermute_d(l2, tot);
            const double p1 = bpermute_d(l1, sp), p2 = bpermute_d(l2, sp);
            const double a1 = bpermute_d(l1, sa), a2 = bpermute_d(l2, sa);
            tot = (tot + t1) + t2;
            sp = (sp + p1) + p2;
            sa = (sa + a1) + a2;
        }
        const double t_lo = 1.5 - a.catch_tol, t_hi = 1.5 + a.catch_tol;  // catch_() thresholds
        const double accf = sp / tot, margin = 1e-12 * (sa / tot);
        const bool fast = sums && tot > 0.0 && __builtin_isfinite(accf) && __builtin_isfinite(margin) &&
                          fabs(accf - t_lo) > margin && fabs(accf - t_hi) > margin;
        need_bin = ballot(binary_fill && !fast);
        if (binary_fill && fast) {
            double gs = catch_(accf, a.catch_tol);
            if (a.int_dtype) gs = trunc(gs);
            S.guess[l] = gs;
        }
        if (col && miss_j) S.tot[l] = tot;  // the present-reputation total, for the median phase
    }
    wsync();
    STAMP(13);
    // scaled columns with missing reports: weighted median of the present values
    {
        uint64_t todo = ballot(col && scj && miss_j != 0);
        // the (x, w) pairs of interpolation median j: present reports, rep / tot (:292-303).
        // weightedstats' sum(weights), sequential in row order (absent rows add +0.0, which leaves
        // a sum from +0.0 unchanged), is formed inside the median only where a decision needs it
        auto pair_of = [&](int j, double& x, double& w, bool& present) {
            const uint64_t mj = S.miss[j];
            present = row && !((mj >> l) & 1);
            const double tot = S.tot[j];
            x = row ? S.F[l * ES + j] : 0.0;
            w = present ? S.rep[l] / tot : 0.0;
        };
        auto finish = [&](int j, double g) {
            if (a.int_dtype) g = trunc(g);
            if (l == 0) S.guess[j] = g;
        };
        // The prescreen (wave_wmedian_screen, DESIGN.md 5.2) first, over every such column: keys and
        // single-precision reputations in the head of the median scratch, which the sorts below
        // overwrite only afterwards.  A round with a negative or NaN reputation does not prescreen
        // (its sums are not monotone), nor one of equal reputations (reputation == nullptr): with an even
        // count of present rows a running sum lies exactly on half, every such column is refused after
        // the prescreen's work, and the batch measured slower than with the sort alone (DESIGN.md 5.2).
        constexpr int NRS = NT > 0 ? NT : 64, KP = (NRS + 3) & ~3;
        const uint64_t all_j = todo;
        if (todo && (REPFLAG ? rep_flag : a.reputation != nullptr) && nonneg) {
            uint32_t* const kx = reinterpret_cast<uint32_t*>(S.M);
            float* const wf = reinterpret_cast<float*>(S.M) + KP;
            if (l < KP) wf[l] = row ? (float)rep : 0.f;
            for (uint64_t t = todo; t; t &= t - 1) {
                const int j = __builtin_ctzll(t);
                const uint64_t mj = S.miss[j];
                const bool present = row && !((mj >> l) & 1);
                const double x0 = row ? S.F[l * ES + j] : 0.0;
                double g;
                if (wave_wmedian_screen<NRS>(x0, rep, present, S.tot[j], N, kx, wf, g)) {
                    finish(j, g);
                    todo &= ~(1ull << j);
                }
            }
            wsync();
        }
        if (a.stamps && l == 0) {  // diagnostic counters: plain stores, no clock read
            a.stamps[b * 32 + 24] = popc(all_j) - popc(todo);
            a.stamps[b * 32 + 25] = popc(todo);
        }
        // The exact replay, the SPEC's sequential form: tot in row order (a missing row adds +0.0,
        // which leaves a sum that starts at +0.0 unchanged), then sum (rep / tot) * F in row order.
        // Wave-wide when a binary column's fast value did not clear the thresholds (or the round
        // formed no fast sums), or when a median goes to the sort, which divides by the exact total.
        const bool replay = need_bin || (todo && !tot_exact);
        if (a.stamps && l == 0) {
            a.stamps[b * 32 + 26] = popc(need_bin);
            a.stamps[b * 32 + 27] = replay;
        }
        if (replay) {
            constexpr int NR = NT > 0 ? NT : 64;
            const double* const Fc = S.F + (col ? l : 0);
            double tot = 0.0;
#pragma unroll 10
            for (int i = 0; i < NR; i++) {
                if (i < N) {
                    const bool miss = (miss_j >> i) & 1;
                    const double re = miss ? 0.0 : S.rep[i];
                    tot = tot + re;
                }
            }
            if (need_bin) {
                double ex = 0.0;
#pragma unroll 10
                for (int i = 0; i < NR; i++) {
                    if (i < N) {
                        const double t = (S.rep[i] / tot) * Fc[i * ES];
                        ex = ((miss_j >> i) & 1) ? ex : ex + t;
                    }
                }
                if ((need_bin >> l) & 1) {
                    double gs = catch_(ex, a.catch_tol);
                    if (a.int_dtype) gs = trunc(gs);
                    S.guess[l] = gs;
                }
            }
            if (col && miss_j) S.tot[l] = tot;
            wsync();
        }
        // the rest one median at a time: the scratch lives in M, dead until the covariance
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            double x0, w0;
            bool p0;
            pair_of(j, x0, w0, p0);
            finish(j, wave_wmedian_rank<(NT > 0 ? NT : 64)>(x0, w0, p0, N, S.M, a.stamps ? mprof : nullptr));
            wsync();
        }
    }
    wsync();
    STAMP(14);
    // fill (row phase; the next column's masks and fill loaded ahead of this column's store)
    if constexpr (ROWREG) {
        // the row's missing columns are the bits the lane collected in the rescale loop (bit l of
        // miss[j] is bit j of nanb | zerob): the guesses in one batch of uniform reads, then the
        // predicated stores with no read between them
        if (row) {
            double gs[ET];
#pragma unroll
            for (int j = 0; j < ET; j++) gs[j] = S.guess[j];
#pragma unroll
            for (int j = 0; j < ET; j++)
                if ((missb >> j) & 1) S.F[l * ES + j] = gs[j];
        }
    } else
    if (row) {
        uint64_t mn = S.miss[0];
        double gn = S.guess[0];
        for (int j = 0; j < E; j++) {
            const uint64_t mj = mn;
            const double g = gn;
            if (j + 1 < E) {
                mn = S.miss[j + 1];
                gn = S.guess[j + 1];
            }
            if ((mj >> l) & 1) S.F[l * ES + j] = g;
        }
    }
    wsync();
    if (double* const fg = out_args()->filled) round_to_global(fg + PCX_ROUND_CELL0, S.F, N, E, ES, NT, ET);

    STAMP(3);
    // ---- old = rep . F (np.dot) -------------------------------------------
    // A compiled shape with 3 E <= 64 forms it in the nonconformity block, as the third vector of the
    // n1 / n2 pass (F does not change in between), and only where it is read: not for alg == 1 or a
    // clustering.
    constexpr bool OLD3 = NT > 0 && ET > 0 && 3 * ET <= W;
    double oldj = 0.0;
    if constexpr (!OLD3) oldj = col ? ob_vecmat(S.rep, S.F + l, ES, N, E, l) : 0.0;  // np.dot(rep, F) (:490)

    double sc_i = 0.0, nc_i = 0.0, ld_j = 0.0;
    int branch = 5, flags = 0, iters = 0, comps = -1;
    const int alg = a.algorithm;
    const bool clus = CLUS && alg >= 5;  // k-means / hierarchical / clusterfeck call wpca too (:393, :408, :422)
    // sum(rep), numpy's pairwise: the weighted mean's denominator (a5) and mean(rep) (a10) are the
    // same sum of the same operands, formed here once for both
    const double rep_sum = pw_rows(rep);
    if (alg == 0 || alg == 2 || alg == 3 || clus) {  // wpca (:315-339): PCA, big-five, fixed-variance
        // ---- a5: weighted mean, np.ma.average (:317-319) -------------------
        const double den = rep_sum;
        double muj = 0.0;
        if (E == 1) {
            const double p = row ? S.F[l * ES] * rep : 0.0;
            const double acc = pw_rows(p);
            muj = acc / den;
        } else if (col) {
            double acc = S.F[l] * S.rep[0];
            for (int i = 1; i < N; i++) acc = acc + S.F[i * ES + l] * S.rep[i];
            muj = acc / den;
        }
        if constexpr (!PK) {  // (the clusterings and big-five read it from LDS)
            wsync();
            if (col) S.mu[l] = muj;
            wsync();
        }

        STAMP(4);
        // ---- a6: token-weighted covariance (:326), lower triangle ----------
        // fp64 MFMA, lower tiles of the 2 x 2 grid: entry (j, k), j >= k, accumulates
        // fma((F_ij - mu_j) * tok_i, F_ik - mu_k, acc) over i ascending -- the SPEC's
        // chain bit for bit (rows past N and events past E are exact zero padding)
        bool nonzero = false, finite = true;
        {
            constexpr int NR = NT > 0 ? NT : 64;
            const int ml = l & 15, kq = l >> 4;
            const bool two = E > 16;
            const double m0 = __shfl(muj, ml), m1 = __shfl(muj, 16 + ml);  // column ml's / 16 + ml's mean
            const double mu0 = ml < E ? m0 : 0.0, mu1 = 16 + ml < E ? m1 : 0.0;
            d4v c00 = {0, 0, 0, 0}, c10 = {0, 0, 0, 0}, c11 = {0, 0, 0, 0};
#pragma unroll
            for (int i0 = 0; i0 < NR; i0 += 4) {
                if (i0 < N) {
                    const int i = i0 + kq;
                    const bool ok = i < N;
                    const double tk = ok ? trunc(S.rep[i] * 1e6) : 0.0;  // the integer tokens (a1)
                    const bool v0 = ok && ml < E, v1 = ok && 16 + ml < E;
                    const double d0 = v0 ? S.F[i * ES + ml] - mu0 : 0.0;
                    const double d1 = v1 ? S.F[i * ES + 16 + ml] - mu1 : 0.0;
                    const double a0 = v0 ? d0 * tk : 0.0, a1 = v1 ? d1 * tk : 0.0;
                    c00 = mfma_f64(a0, d0, c00);
                    if (two) {
                        c10 = mfma_f64(a1, d0, c10);
                        c11 = mfma_f64(a1, d1, c11);
                    }
                }
            }
            // The compiled shapes divide through one reciprocal of the wave-uniform denom per round (div_rn,
            // pcx_fastdiv.h: four instructions for the division's eleven, the same bits).  An exact-zero
            // accumulator (a column every reporter agrees on), denom == 0 and a non-finite denom take
            // div_rn's guard, the division itself, behind a branch no lane of an ordinary round takes.
            double yden = 0.0;
            if constexpr (ROWREG) yden = range_rcp(denom);
            auto put = [&](int j, int k, double acc) {  // j >= k
                double c;
                if constexpr (ROWREG)
                    c = div_rn(acc, denom, yden);
                else
                    c = acc / denom;
                S.C[sym_at<PK>(j, k, ES)] = c;
                if (!PK) {
                    S.M[sym_at<PK>(j, k, ES)] = c;
                    S.C[k * ES + j] = c;
                    S.M[k * ES + j] = c;
                }
                nonzero |= c != 0.0;
                finite &= __builtin_isfinite(c) != 0;
            };
            if constexpr (PK) wsync();  // packed C lies over rep, which the loop above read
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j0 = kq + 4 * r, j1 = 16 + kq + 4 * r, k0 = ml, k1 = 16 + ml;
                if (j0 < E && k0 <= j0) put(j0, k0, c00[r]);
                if (j1 < E && k0 < E) put(j1, k0, c10[r]);
                if (j1 < E && k1 <= j1) put(j1, k1, c11[r]);
            }
        }
        const bool any_nz = ballot(nonzero) != 0;
        const bool all_fin = ballot(!finite) == 0;
        wsync();

        STAMP(5);
        // ---- a7: leading eigenvector by power iteration (:330-336) -------
        double xv = 0.0;
        if (!all_fin) {
            xv = col ? 1.0 : 0.0;
            flags |= 2;
        } else if (!any_nz) {
            xv = l == 0 ? 1.0 : 0.0;
            flags |= 1;
        } else {
            // start: the column with the largest diagonal entry (first max; C is finite here)
            const double dg = col ? S.C[sym_at<PK>(l, l, ES)] : -__builtin_inf();
            // (the lanes from E on hold -inf, below every finite entry: live rows only).  The maximum
            // is formed by the whole wave, outside the `col &&`: on its right-hand side the DPP steps
            // ran with the lanes from E on switched off and read 0.0 for them, above every entry
            // when the whole diagonal is negative (a negative reputation), and no lane matched.
            const double dgmax = wave_max<CR>(dg);
            const int kd = __builtin_ctzll(ballot(col && dg == dgmax));
            double x0 = col ? S.C[sym_at<PK>(l, kd, ES)] : 0.0;
            const double ss0 = tree_sum<CR>(x0 * x0);  // squares, +0.0 from lane E on: no row sum is -0.0
            double n0;
            if constexpr (ROWREG)
                n0 = sqrt_uniform(ss0);
            else
                n0 = sqrt(ss0);
            xv = col ? x0 / n0 : 0.0;
            // packed: M starts as C's operands and is squared in registers (the covariance
            // accumulators cannot seed it: (d_j tok) d_k and (d_k tok) d_j round differently, and C
            // is its lower triangle mirrored); the matrix-vector steps read M's triangle from C's
            // place in LDS, and C's operands (creg) are written back for the polish steps
            constexpr int NS = !PK ? 1 : ET > 0 ? (ET + 3) / 4 : EMAX / 4;
            SymOps<NS> mreg, creg;
            if constexpr (PK) {
                load_sym_ops<NS>(S.C, E, mreg);
                creg = mreg;
            }
            auto square = [&](bool in_loop) {
                if constexpr (PK) {  // (M's triangle lies over C in LDS between the squarings)
                    if (in_loop) load_sym_ops<NS>(S.C, E, mreg);
                    square_scaled_reg<NS>(mreg, E);
                    if (in_loop) store_sym_ops<NS>(S.C, E, mreg);
                } else {
                    square_scaled<PK>(S.M, ES, E);
                }
            };
            int sqn = 0;
            for (; sqn < PI_PRESQUARE; sqn++) square(false);
            if constexpr (PK) store_sym_ops<NS>(S.C, E, mreg);
            const SymBase sb = sym_base(S.C, col ? l : 0);  // (the matrix-vector steps' row of the triangle)
            int it = 0, since = 0;
            for (;;) {
                const double y = matvec_unit<PK, CR, ET>(PK ? S.C : S.M, ES, xv, E, sb);
                // SPEC: d = max over the events of |y - x|, stop when d <= PI_TOL.  Only the compare
                // is used, and d <= PI_TOL holds exactly when no event lane has |y - x| > PI_TOL:
                // the maximum (v_max_f64) drops a NaN operand and the lanes from E on feed 0.0, so a
                // NaN difference never reaches d, just as `NaN > PI_TOL` is false for it (all of
                // them NaN: d = 0.0, the loop stops, and so does this); an infinite difference makes
                // d infinite and the compare true, and the loop goes on in both forms.
                const bool moved = ballot(col && fabs(y - xv) > PI_TOL) != 0;
                xv = y;
                it++;
                since++;
                if (!moved) break;
                if (it >= PI_MAXIT) {
                    flags |= 4;
                    break;
                }
                if (since >= PI_SQUARE_EVERY && sqn < PI_MAX_SQUARINGS) {
                    square(true);
                    sqn++;
                    since = 0;
                }
            }
            // the polish steps run on C itself
            if constexpr (PK) store_sym_ops<NS>(S.C, E, creg);
            for (int p = 0; p < PI_POLISH; p++) xv = matvec_unit<PK, CR, ET>(S.C, ES, xv, E, sb);
            // SPEC sign: first nonzero component negative; a unit vector e_k is +e_k
            const uint64_t nzm = ballot(col && xv != 0.0);
            if (nzm) {
                const double xf = bcast(xv, __builtin_ctzll(nzm));
                const bool neg = popc(nzm) == 1 ? xf < 0.0 : xf > 0.0;
                if (neg) xv = -xv;
            }
            iters = it + PI_POLISH + sqn;
        }
        // loading = v / sqrt(sum(v**2)) with numpy's pairwise sum (:336)
        const double ssv = pw_cols(xv * xv);
        double nv;
        if constexpr (ROWREG)
            nv = sqrt_uniform(ssv);
        else
            nv = sqrt(ssv);
        ld_j = col ? xv / nv : 0.0;
        wsync();
        if (clus) {
            // the loading only: scores stay zeros (:357)
        } else if (alg == 0) {
            // scores s = wcd . loading (:337), row phase (column j's mean and loading from lane j)
            const int r = row ? l : 0;
            double acc = 0.0;
            if constexpr (ET > 0 && ET <= 32) {
                // the means and the loading spread once over all four rows, each column's subtraction
                // and multiply-add taking its own by row_newbcast (pcx_batched.hip, "broadcasts inside
                // the 16-lane row"); the whole wave runs this: `clus` and `alg` are launch constants
                const RowSpread mu = row_spread4(muj), ld = row_spread4(ld_j);
                double one = 1.0;  // (a register operand of the subtraction, settled like the spreads)
                asm("s_nop 1" : "+v"(one));
                static_cols<0, ET>([&](auto j) {
                    fmac_rowbcast<j.value>(acc, ld, sub_rowbcast<j.value>(S.F[r * ES + j.value], mu, one));
                });
            } else {
                for (int j = 0; j < E; j++) acc = fma(S.F[r * ES + j] - lane_value(muj, j), lane_value(ld_j, j), acc);
            }
            if (row) sc_i = acc;
        } else if (flags & 2) {
            sc_i = __builtin_nan("");  // the reference's second svd raises (:375, :431)
        } else if constexpr (!PK) {  // (the packed layout is never launched for these)
            // ---- big-five (:373-390) / fixed-variance (:429-451): net score =
            // sum_c Sigma_c * (wcd . loading_c); Sigma, loadings from Jacobi (SPEC)
            const double trace = pw_cols(col ? S.C[l * ES + l] : 0.0);  // np.trace
            wsync();
            for (int o = l; o < E * E; o += W) {
                const int j = o / E, k = o - j * E;
                S.M[j * ES + k] = S.C[j * ES + k];
            }
            wsync();
            jacobi_eig_wave(S.M, S.C, ES, E, S.x, S.ld);  // A in M; V overwrites C; x, ld are dead
            const double sig = col ? fabs(S.M[l * ES + l]) : 0.0;
            if (col) S.nv1[l] = sig;
            wsync();
            if (col) {  // order: descending Sigma, ties by index
                int rk = 0;
                for (int k = 0; k < E; k++) rk += (S.nv1[k] > sig) | ((S.nv1[k] == sig) & (k < l));
                S.nv2[rk] = (double)l;
            }
            wsync();
#if PCX_ROUND_RAGGED  // max_components capped at the round's E (:134-137)
            const int kmax = alg == 2 && a.max_components < E ? a.max_components : E;
#else
            const int kmax = alg == 2 ? a.max_components : E;
#endif
            double net = 0.0, ve = 0.0;
            int used = kmax;
            for (int c = 0; c < kmax; c++) {
                const int idx = (int)S.nv2[c];
                const double sg = S.nv1[idx];
                const double fl = S.C[idx] < 0.0 ? -1.0 : 1.0;  // loading *= -1 if loading[0] < 0
                if (row) {
                    double d = 0.0;
                    for (int j = 0; j < E; j++) d = fma(S.F[l * ES + j] - S.mu[j], fl * S.C[j * ES + idx], d);
                    net = net + sg * d;
                }
                if (alg == 3) {  // cumsum(Sigma / trace) >= threshold -> stop (:432, :448)
                    ve = ve + sg / trace;
                    if (ve >= a.variance_threshold) {
                        used = c + 1;
                        break;
                    }
                }
            }
            comps = alg == 3 ? used : -1;
            sc_i = net;
            wsync();
        }
    } else if (alg == 4) {  // cokurtosis: caller-supplied scores (:455-457)
        sc_i = row ? a.aux_scores[PCX_ROUND_ROW0 + l] : 0.0;
    }
    STAMP(6);
    if constexpr (CLUS) {
        if (clus) {
            double* X = smem + smem_doubles(N, E, ES, NRM, PK);
            if (alg == 6)
                nc_i = hier_nc(S.F, S.mu, ES, N, E, a.hierarchy_threshold, reinterpret_cast<uint64_t*>(X));
#if !PCX_ROUND_RAGGED  // (a ragged launch refuses k-means: its code-book size depends on the round's N)
            else if (alg == 5)
                nc_i = kmeans_nc(a, b, S.F, S.mu, ES, N, E, X);
#elif PCX_ROUND_RAGGED == 3  // (the round's own books: a.kmeans_init points at them)
            else if (alg == 5)
                nc_i = kmeans_nc(a, 0, S.F, S.mu, ES, N, E, X);
#endif
            else
                nc_i = feck_nc(a, S.F, ES, N, E, rep, X);
            wsync();
        }
    }
    if (alg != 1 && !clus) {
        // ---- a8/a9: nonconformity_rank (:487-500) / nonconformity (:475-485); the
        // non-PCA algorithms call nonconformity directly (:389, :450, :456)
        const bool any_nan = ballot(row && __builtin_isnan(sc_i)) != 0;
        double mn = wave_max(row ? -sc_i : -__builtin_inf());
        mn = -mn;
        double mx = wave_max(row ? sc_i : -__builtin_inf());
        if (any_nan) {
            mn = __builtin_nan("");
            mx = __builtin_nan("");
        }
        const double set1 = sc_i + fabs(mn);
        const double set2 = sc_i - mx;
        double a1 = fabs(set1), a2 = fabs(set2);
        double S1, S2;
        pw_rows2(a1, a2, S1, S2);  // (both operands exist before either sum is needed; the re-sums are rare)
        if (S1 == 0) {
            a1 += 1.0;
            S1 = pw_rows(a1);
        }
        if (S2 == 0) {
            a2 += 1.0;
            S2 = pw_rows(a2);
        }
        if (row) {
            S.n1[l] = a1 / S1;
            S.n2[l] = a2 / S2;
            // OLD3: rep from the row lanes' registers into the smooth slot, dead from the scores until
            // the reputation update stores smooth_rep (rep's own place went to the covariance)
            if constexpr (OLD3) S.smooth[l] = rep;
        }
        if constexpr (!OLD3) {
            if (col) S.old[l] = oldj;
        }
        wsync();
        double d1 = 0.0, d2 = 0.0;
        if constexpr (OLD3) {
            // three products in one pass over the rows: lane g E + j runs column j on n1, n2 or rep
            // (g = 0, 1, 2), each lane ob_vecmat's own sequence on its vector, then d2 and old come
            // down to lane j by ds_bpermute
            const int g = (l >= ET) + (l >= 2 * ET);
            const bool live = l < 3 * ET;
            const int jc = live ? l - g * ET : 0;
            double d = 0.0;
            if (live) d = ob_vecmat(g == 0 ? S.n1 : g == 1 ? S.n2 : S.smooth, S.F + jc, ES, N, E, jc);
            const double dn = bpermute_d((l + ET) & (W - 1), d), dr = bpermute_d((l + 2 * ET) & (W - 1), d);
            if (col) {
                d1 = d;
                d2 = dn;
                oldj = dr;
                S.old[l] = oldj;
            }
        } else {
            // both products in one pass over the rows: lane j < E runs column j on n1, lane 32 + j
            // the same column on n2 (E <= 32) -- one instruction stream, each lane its own vector
            // and its column's own order (block, tail or ddot), then d2 moves down to lane j
            const int jc = l & 31;
            double d = 0.0;
            if (jc < E) d = ob_vecmat(l < 32 ? S.n1 : S.n2, S.F + jc, ES, N, E, jc);  // np.dot(normalize(set), F) (:492)
            const uint64_t du = (uint64_t)__double_as_longlong(d);
            const int up = ((l + 32) & 63) << 2;
            const uint32_t ulo = (uint32_t)__builtin_amdgcn_ds_bpermute(up, (int)(uint32_t)du);
            const uint32_t uhi = (uint32_t)__builtin_amdgcn_ds_bpermute(up, (int)(uint32_t)(du >> 32));
            if (col) {
                d1 = d;
                d2 = __longlong_as_double((long long)(((uint64_t)uhi << 32) | ulo));
            }
        }
        if (col) {
            const double t = 0.01 * oldj;
            S.nv1[l] = d1 + t;
            S.nv2[l] = d2 + t;
        }
        wsync();
        double ref = 0.0;  // non-PCA: straight to the continuous rule
        if (alg == 0) {
            double r0, r1, r2;
            if (3 * E <= W) {  // (wave-uniform)
                rank_avg3(S.old, S.nv1, S.nv2, E, r0, r1, r2);
            } else {
                r0 = rank_avg(S.old, E);
                r1 = rank_avg(S.nv1, E);
                r2 = rank_avg(S.nv2, E);
            }
            const double e1 = fabs(r1 - r0), e2 = fabs(r2 - r0);
            ref = pw_cols(e1) - pw_cols(e2);
        }
        bool pick1;
        if (ref == 0) {
            const double q1 = d1 - oldj, q2 = d2 - oldj;
            const double ref2 = pw_cols(q1 * q1) - pw_cols(q2 * q2);
            pick1 = ref2 <= 0;
            branch = pick1 ? 3 : 4;
        } else {
            pick1 = ref < 0;
            branch = pick1 ? 1 : 2;
        }
        nc_i = pick1 ? set1 : set2;
    }

    STAMP(7);
    // ---- a10: reputation update (:460-472) --------------------------------
    const double meanrep = rep_sum / (double)N;
    double u = fabs(nc_i * (rep / meanrep));
    double Su = pw_rows(u);
    // PCA: a NaN total leaves the reference's this_rep / smooth_rep fully MASKED (SPEC
    // rep_masked: participation_columns, reporter_bonus and author_bonus are numpy.ma's data)
    const bool rep_masked = alg == 0 && __builtin_isnan(Su);
    if (Su == 0) {
        u += 1.0;
        Su = pw_rows(u);
    }
    const double this_i = u / Su;
    const double smooth_i = a.alpha * this_i + (1.0 - a.alpha) * rep;
    wsync();
    if (row) S.smooth[l] = smooth_i;
    wsync();

    STAMP(8);
    // ---- a12/a13: outcomes (:510-538) -------------------------------------
    // The compiled shapes load the scaled columns' bounds again here (L2 hits, in flight over the
    // np.dot and the medians) instead of holding four registers since the rescale: under the
    // 128-register budget the allocator otherwise spills them and reloads them per rescaled column.
    double lo2 = NT > 0 ? 0.0 : loj, hi2 = NT > 0 ? 0.0 : hij;  // (read by scaled columns only)
    if constexpr (NT > 0) {
        if (col && scj) {
            lo2 = a.lo[bo + l];
            hi2 = a.hi[bo + l];
        }
    }
    double rawj = col ? ob_vecmat(S.smooth, S.F + l, ES, N, E, l) : 0.0;  // np.dot(smooth_rep, F) (:510)
    STAMP(15);
    if (scaled_mask) {
        // The fill-group test (DESIGN.md 5.2).  A scaled column with missing rows holds its fill g in
        // every one of them, and smooth_rep stays close to rep, whose median of the present rows g is:
        // the rows equal to g almost always straddle half the weight.  With the tree-order sums
        //   Wt = sum w,  below = sum w [x < g],  group = sum w [x == g]
        // (each within (N + 6) u Wt of the SPEC's sequential sum over the same rows) and the margin
        // M of the scan-decided walk (wave_wmedian_rank), below <= Wt / 2 - M and below + group >
        // Wt / 2 + M place the SPEC's crossing inside the group: the median is g bit for bit, with no
        // sort.  The SPEC's earlier exits come first, in its order, wherever the data is near one: a
        // weight within the slack of half the total or above it (the dominant exit compares against
        // the exact total), no positive weight, a NaN or a negative weight (the sums are not monotone),
        // a NaN value, and a fill that is NaN, zero (the group may mix -0.0 and +0.0) or so large that
        // g + g overflows in the two-value mean.  Every such column takes wave_wmedian_rank.
        const double Wt = tree_sum(row ? smooth_i : 0.0);
        const double mid = 0.5 * Wt, slack = 0x1p-45 * Wt;
        const double Mg = 0x1p-44 * Wt + slack + DBL_EPS;
        // the weights' conditions hold for every column of the round (a NaN weight fails both compares)
        const bool wok = Mg < __builtin_inf() && !ballot(row && !(smooth_i >= 0.0 && smooth_i < mid - slack)) &&
                         ballot(row && smooth_i > 0.0) != 0;
        uint64_t slow = 0;  // the columns the test does not decide
        // Compiled shapes with 3 E <= 64: every column's two sums in one pass, in the guesses' layout.
        // Lane g * E + c adds, over column c's rows g, g + 3, g + 6, ... in ascending order,
        // w [x < fill_c] and w [x == fill_c] (w = smooth_rep from LDS, fill_c read from the column's
        // first missing row; the indicator is 1.0 or 0.0 and fma(w, 1, s) is s + w), keeps a "saw a NaN
        // value" bit, and lane c takes (p0 + p1) + p2 by ds_bpermute.  The sums need accuracy only:
        // any order of adding at most N non-negative terms stays within (N - 1) u of the exact sum,
        // inside the (N + 6) u Wt the margin Mg allows, so mid, slack and Mg are the loop's.
        constexpr bool FGSPLIT = NT > 0 && ET > 0 && 3 * ET <= W;
        if constexpr (FGSPLIT) {
            slow = scaled_mask;
            if (wok) {  // (wave-uniform)
                constexpr int TS = (NT + 2) / 3;
                const int g = (l >= ET) + (l >= 2 * ET);
                const bool live = l < 3 * ET;
                const int c = live ? l - g * ET : 0;
                const uint64_t mc = S.miss[c];
                const int fm = mc ? __builtin_ctzll(mc) : 0;
                const double gf = S.F[fm * ES + c];  // the fill (a column with no missing row: unused)
                const double* const Fp = S.F + g * ES + c;
                const double* const wp = S.smooth + g;
                double below = 0.0, group = 0.0;
                bool sawnan = false;
#pragma unroll
                for (int t = 0; t < TS; t++) {
                    // (rows past the last: the loads lie in the round's own LDS and are switched off here)
                    const bool in = 3 * t + 2 < NT || g + 3 * t < NT;
                    const double x = Fp[3 * t * ES], w = in ? wp[3 * t] : 0.0;
                    const double ib = in && x < gf ? 1.0 : 0.0, ig = in && x == gf ? 1.0 : 0.0;
                    below = fma(w, ib, below);
                    group = fma(w, ig, group);
                    sawnan |= in && x != x;
                }
                const int l1 = (l + ET) & (W - 1), l2 = (l + 2 * ET) & (W - 1);
                const double b1 = bpermute_d(l1, below), b2 = bpermute_d(l2, below);
                const double g1 = bpermute_d(l1, group), g2 = bpermute_d(l2, group);
                below = (below + b1) + b2;
                group = (group + g1) + g2;
                const uint64_t nm = ballot(live && sawnan);
                const bool cnan = (((nm | (nm >> ET)) | (nm >> (2 * ET))) >> l) & 1;  // (read on lanes < E)
                // (a NaN fill fails the second compare)
                const bool decided = col && scj && mc != 0 && gf != 0.0 && fabs(gf) < 0x1p1023 && !cnan &&
                                     below <= mid - Mg && below + group > mid + Mg;
                if (decided) rawj = gf;
                slow = scaled_mask & ~ballot(decided);
            }
        } else
        for (uint64_t todo = scaled_mask; todo; todo &= todo - 1) {  // (no LDS write, no wave barrier)
            const int j = __builtin_ctzll(todo);
            const double x0 = row ? S.F[l * ES + j] : 0.0;
            const uint64_t mj = (uint64_t)uniform64((int64_t)S.miss[j]);
            bool decided = false;
            if (wok && mj) {
                const double g = bcast(x0, __builtin_ctzll(mj));  // the first missing row's: the fill
                if (g != 0.0 && fabs(g) < 0x1p1023 && !ballot(row && x0 != x0)) {  // (a NaN g fails the second)
                    const double below = tree_sum(row && x0 < g ? smooth_i : 0.0);
                    const double group = tree_sum(row && x0 == g ? smooth_i : 0.0);
                    decided = below <= mid - Mg && below + group > mid + Mg;
                    if (decided && l == j) rawj = g;
                }
            }
            if (!decided) slow |= 1ull << j;
        }
        if (a.stamps && l == 0) {  // diagnostic counters: plain stores, no clock read
            a.stamps[b * 32 + 22] = popc(scaled_mask) - popc(slow);
            a.stamps[b * 32 + 23] = popc(slow);
        }
        while (slow) {  // scratch in M, dead after the scores
            const int j = __builtin_ctzll(slow);
            slow &= slow - 1;
            const double x0 = row ? S.F[l * ES + j] : 0.0;
            // (weightedstats' sequential total of smooth_rep is formed inside only where a decision needs it)
            const double m = wave_wmedian_rank<(NT > 0 ? NT : 64)>(x0, smooth_i, row, N, S.M, a.stamps ? mprof : nullptr);
            if (l == j) rawj = m;
            wsync();
        }
    }
    STAMP(16);
    double adjj = 0.0, finj = 0.0;
    if (col) {
        if (scj) {
            adjj = rawj;
            finj = adjj * (hi2 - lo2);
            finj = finj + lo2;
        } else {
            adjj = catch_(rawj, a.catch_tol);
            finj = adjj;
        }
        S.adj[l] = adjj;
    }
    wsync();

    STAMP(9);
    // ---- a14: certainty (:540-546): pairwise sum of the matching smooth_rep --
    // every column at once, one lane per column: the hit masks first (F is read for the
    // last time), then each row lane scatters its smooth_rep into the compacted hit list of
    // every column it matches (into F, dead from here on), then lane j runs numpy's pairwise
    // add.reduce (n <= 128: eight strided accumulators, fixed tree, sequential tail) on
    // its column's list
    double certj = 0.0;
    {
        uint64_t* hitm = reinterpret_cast<uint64_t*>(S.M);  // [E]; M is dead after the medians
        const int NS = cert_stride(N, ES);  // odd stride: lane-per-column reads spread over the banks
        double* comp = S.F;    // [E][NS]
        uint64_t hm_l = 0;     // ROWREG: column l's hit mask (lanes < E)
        if constexpr (ROWREG) {
            // The row in one batch of reads, after which F is dead and the hit lists can go over it:
            // column j's adjusted outcome comes from lane j's register (readlane), its hit mask stays
            // in scalar registers for the scatter's store and goes to lane j by v_writelane_b32 for
            // the sum below.  One loop, no LDS read and no wait in it, no mask in LDS.
            double fr[ET];
#pragma unroll
            for (int j = 0; j < ET; j++) fr[j] = 0.0;
            if (row) {
                const double2* const Fr = reinterpret_cast<const double2*>(S.F + l * ES);
#pragma unroll
                for (int q = 0; q < ET / 2; q++) {
                    const double2 v = Fr[q];
                    fr[2 * q] = v.x;
                    fr[2 * q + 1] = v.y;
                }
                if (ET & 1) fr[ET - 1] = S.F[l * ES + ET - 1];
            }
            wsync();
            uint32_t hlo = 0, hhi = 0;
            static_cols<0, ET>([&](auto jc) {
                constexpr int j = jc.value;
                const double av = bcast(adjj, j);
                const uint64_t hm = ballot(row && fr[j] == av);
                if ((hm >> l) & 1) comp[j * NS + mbcnt64(hm)] = smooth_i;
                hlo = write_lane<j>(hlo, (uint32_t)hm);
                hhi = write_lane<j>(hhi, (uint32_t)(hm >> 32));
            });
            hm_l = ((uint64_t)hhi << 32) | hlo;
            wsync();
        } else {
        double fn = row ? S.F[l * ES] : 0.0, an = S.adj[0];  // (next column's loads ahead of this column's store)
        for (int j = 0; j < E; j++) {
            const double f = fn, av = an;
            if (j + 1 < E) {
                fn = row ? S.F[l * ES + j + 1] : 0.0;
                an = S.adj[j + 1];
            }
            const uint64_t hm = ballot(row && f == av);
            if (l == 0) hitm[j] = hm;
        }
        wsync();
        for (int j = 0; j < E; j++) {
            const uint64_t hm = hitm[j];
            if ((hm >> l) & 1) comp[j * NS + mbcnt64(hm)] = smooth_i;
        }
        wsync();
        }
        if (col) {
            constexpr int TMAX = (NT > 0 ? NT : 64) / 8;
            const uint64_t hm = ROWREG ? hm_l : hitm[l];
            const int n = popc(hm), T = n >> 3;
            const double* c = comp + l * NS;
            double res = 0.0;
            if (T) {
                double r[8];
#pragma unroll
                for (int k = 0; k < 8; k++) r[k] = c[k];
#pragma unroll
                for (int t = 1; t < TMAX; t++)
                    if (t < T) {
#pragma unroll
                        for (int k = 0; k < 8; k++) r[k] = r[k] + c[8 * t + k];
                    }
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            }
            for (int q = 8 * T; q < n; q++) res = res + c[q];  // the tail (everything when n < 8)
            certj = n ? res : (a.algorithm == 0 ? __builtin_nan("") : 0.0);
        }
    }
    // normalize(certainty), mean(certainty)
    double ac = fabs(certj);
    double Sc = pw_cols(ac);
    if (Sc == 0) {
        ac += 1.0;
        Sc = pw_cols(ac);
    }
    const double reward = ac / Sc;
    const double avg_cert = pw_cols(certj) / (double)E;

    STAMP(10);
    // ---- a15: participation and bonuses (:549-581) -------------------------
    double pcj = 0.0, nzj = 0.0;
    // every smooth_rep finite: a row with na = 0 adds p = x * 0 = +-0 and pe = +-0, which leave
    // (s, c) bit for bit as they were (neither is ever -0.0), so only the missing rows are visited
    const bool smooth_finite = !ballot(row && !__builtin_isfinite(smooth_i));
    if (col) {
        const uint64_t nam = S.miss[l];
        // dot2(smooth, na) with na in {0,1}
        double s = 0.0, c = 0.0;
        auto step = [&](double x, double y) {
            const double p = x * y;
            const double pe = fma(x, y, -p);
            const double t = s + p;
            const double z = t - s;
            const double se = (s - (t - z)) + (p - z);
            s = t;
            c = c + (pe + se);
        };
        if (smooth_finite) {
            for (uint64_t mm = nam; mm; mm &= mm - 1) step(S.smooth[__builtin_ctzll(mm)], 1.0);
        } else {
            for (int i = 0; i < N; i++) step(S.smooth[i], ((nam >> i) & 1) ? 1.0 : 0.0);
        }
        pcj = 1.0 - (s + c);
        nzj = (double)((nacnt >> 16) & 0xffu);
    }
    double narow = 0.0;
    int nnan = 0;
    if (row) {
        narow = (double)(nacnt & 0xffu);
        nnan = (int)((nacnt >> 8) & 0xffu);
    }
    const bool rowmasked = row && nnan == E;
    const double pr = 1.0 - narow / (double)E;
    const double pna = 1.0 - pw_cols(pcj) / (double)E;
    double ar = rowmasked ? 0.0 : fabs(pr);
    double Sr = pw_rows(ar);
    if (Sr == 0) {
        ar = rowmasked ? 0.0 : fabs(pr) + 1.0;
        Sr = pw_rows(ar);
    }
    const double rel = rowmasked ? fabs(pr) : ar / Sr;
    double apc = fabs(pcj);
    double Spc = pw_cols(apc);
    if (Spc == 0) {
        apc += 1.0;
        Spc = pw_cols(apc);
    }
    const double relc = apc / Spc;

    STAMP(11);
    // ---- write the round ---------------------------------------------------
    const auto oa = out_args();
    if (row) {
        const int64_t o = PCX_ROUND_ROW0 + l;
        if (oa->old_rep) oa->old_rep[o] = rep;
        if (oa->this_rep) oa->this_rep[o] = this_i;
        if (oa->smooth_rep) oa->smooth_rep[o] = smooth_i;
        if (oa->scores) oa->scores[o] = sc_i;
        if (oa->na_row) oa->na_row[o] = narow;
        if (oa->participation_rows) oa->participation_rows[o] = pr;
        if (oa->relative_part) oa->relative_part[o] = rel;
        if (oa->reporter_bonus) oa->reporter_bonus[o] = (rowmasked || rep_masked) ? rel : rel * pna + smooth_i * (1.0 - pna);
    }
    if (col) {
        const int64_t o = PCX_ROUND_EV0 + l;
        if (oa->adj_first_loadings) oa->adj_first_loadings[o] = ld_j;
        if (oa->outcomes_raw) oa->outcomes_raw[o] = rawj;
        if (oa->outcomes_adjusted) oa->outcomes_adjusted[o] = adjj;
        if (oa->outcomes_final) oa->outcomes_final[o] = finj;
        if (oa->certainty) oa->certainty[o] = certj;
        if (oa->consensus_reward) oa->consensus_reward[o] = reward;
        if (oa->nas_filled) oa->nas_filled[o] = nzj;
        if (oa->participation_columns) oa->participation_columns[o] = rep_masked ? 1.0 : pcj;
        if (oa->author_bonus) oa->author_bonus[o] = rep_masked ? 1.0 : relc * pna + reward * (1.0 - pna);
    }
    if (l == 0) {
        if (oa->participation) oa->participation[b] = 1.0 - pna;
        if (oa->avg_certainty) oa->avg_certainty[b] = avg_cert;
        if (oa->branch) oa->branch[b] = branch;
        if (oa->flags) oa->flags[b] = flags;
        if (oa->pi_iters) oa->pi_iters[b] = iters;
        if (oa->components) oa->components[b] = comps;
    }
    STAMP(12);
    if (a.stamps && threadIdx.x == 0) {
        a.stamps[b * 32 + 20] = mprof[0];
        a.stamps[b * 32 + 21] = mprof[1];
    }
}
#undef PCX_ROUND_CELL0
#undef PCX_ROUND_ROW0
#undef PCX_ROUND_EV0
#undef PCX_ROUND_B
