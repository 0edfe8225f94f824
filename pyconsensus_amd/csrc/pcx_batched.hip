// pcx_batched.hip -- batched oracle rounds on MI355X (gfx950): one wavefront per
// independent round (Simulator.jl-style Monte Carlo, README.rst:52-56).
//
// Each workgroup is ONE wave64 that runs a complete
// Oracle(reports, event_bounds, reputation).consensus()
// (pyconsensus/__init__.py:102-611, algorithm="PCA") for one N x E round held in
// LDS (N <= 64 reporters: one lane per reporter row; E <= 32 events: one lane per
// event column).  All arithmetic is IEEE fp64; the file is compiled with
// -ffp-contract=off and every fma() is deliberate.  The arithmetic order is the
// one written down in oracle/pcx_oracle_batched.c (the "SPEC"), so results are
// bit-identical to that CPU restatement; see there for which steps replay the
// reference's numpy order exactly and which use compensated dots / power
// iteration in place of OpenBLAS / LAPACK.
//
// Lane roles per phase:
//   row phase    lane i = reporter i      (rescale, fill, scores, bonuses)
//   column phase lane j = event j         (sequential column sums, GEMV^T, ranks)
//   entry phase  lane o = matrix entry o  (covariance, matrix squaring)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "pcx_fastdiv.h"
#include "pcx_internal.h"

namespace pcx {

namespace {

constexpr int W = 64;        // wavefront
constexpr int NMAX = 64;  // reporters per round (one lane each)
constexpr int EMAX = 32;  // events per round (MFMA tiles 2 x 16; pcx_api.cpp validates)
static_assert(EMAX <= 2 * 16, "2 x 2 grid of 16 x 16 MFMA tiles");
static_assert(NMAX == W, "one reporter per lane");
constexpr int PACKED_WAVES = 4;  // waves per SIMD the compiled packed shapes' VGPR budget is sized for (128 VGPRs)

// power iteration constants (SPEC; equal to oracle/pcx_oracle_batched.c)
constexpr double PI_TOL = 1e-14;
constexpr int PI_MAXIT = 256;
constexpr int PI_PRESQUARE = 3;
constexpr int PI_SQUARE_EVERY = 32;
constexpr int PI_MAX_SQUARINGS = 8;
constexpr int PI_POLISH = 2;
constexpr double DBL_MIN_ = 2.2250738585072014e-308;
constexpr double DBL_EPS = 2.220446049250313080847e-16;

__device__ __forceinline__ int lane_id() { return threadIdx.x; }

// The round's helpers run inlined: the 50 x 20 kernel is ~83 KB of code, yet the instruction
// cache misses 0.14 % of its fetches (SQC_ICACHE_MISSES / HITS, profiles/r3); outlined (calls,
// __noinline__, 49 KB + shared helpers) the call ABI spills and the kernel ran 29 %
// slower (24.4 M vs 34.4 M rounds/s).
#define PCX_OUTLINE __forceinline__

// diagnostic phase stamps (PCX_STAMPS=1): shader-clock reads at phase boundaries
#define STAMP(k)                                                                  \
    do {                                                                          \
        if (a.stamps) {                                                           \
            const long long t_ = (long long)__builtin_amdgcn_s_memtime();         \
            if (threadIdx.x == 0) a.stamps[b * 32 + (k)] = t_;                    \
        }                                                                         \
    } while (0)

// One wave per workgroup: the LDS operations of a wave execute in issue order, so a
// compiler-ordering wave barrier suffices between an LDS write and another lane's read
// (no lgkmcnt(0) drain, which __syncthreads() emits).
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }

__device__ __forceinline__ int popc(uint64_t m) { return __popcll(m); }

// broadcast from a wave-uniform lane: v_readlane into SGPRs (no LDS-pipe round trip)
__device__ __forceinline__ double bcast(double v, int src) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// lane l <- lane l ^ S inside a 16-lane row, DPP only (VALU, no LDS-pipe round trip):
// quad_perm (1, 2), row_shr:4 / row_shl:4 selected by lane bit 2 (4), row_ror:8 (8).
// bound_ctrl: a lane whose source lies outside its row reads 0, which is what `old` = 0 gave it --
// but with it the compiler need not write that 0 into the destination ahead of every DPP move.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
template <int S>
__device__ __forceinline__ uint32_t xor_lane32(uint32_t v) {
    if constexpr (S == 1) return dpp32<0xB1>(v);
    else if constexpr (S == 2) return dpp32<0x4E>(v);
    else if constexpr (S == 8) return dpp32<0x128>(v);
    else {
        static_assert(S == 4, "row-local distances only");
        const uint32_t up = dpp32<0x114>(v), dn = dpp32<0x104>(v);  // lane l-4 | lane l+4
        return (threadIdx.x & 4) ? up : dn;
    }
}

template <int S>
__device__ __forceinline__ double xor_lane(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = xor_lane32<S>((uint32_t)u), hi = xor_lane32<S>((uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// lane l <- lane l + D of its 16-lane row (row_shl: the lanes past the row's end read +0.0)
template <int D>
__device__ __forceinline__ double shl_lane(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = dpp32<0x100 + D>((uint32_t)u), hi = dpp32<0x100 + D>((uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ double lane_value(double v, int k) {  // lane k's v (k wave-uniform)
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), k);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// SPEC tree64: a butterfly inside each 16-lane row (xor 1, 2, 4, 8: every lane of a row
// ends with the same row sum R_r), then (R0 + R1) + (R2 + R3) from lanes 0, 16, 32, 48.
// Only those four lanes are read, so the xor-4 step is row_shl:4 alone: lane 0 needs lane 4's value
// and lane 8, which lane 0 reads at the xor-8 step, lane 12's -- the additions that reach lane 0 and
// their order are the butterfly's (pw_tree8 relies on the same).  wave_max does likewise.
// ROWS < 4: the caller's lanes from 16 * ROWS on hold +0.0 and no row sum is -0.0 (squares, say),
// so the dead rows' sums are +0.0 and adding them changes no bit: R0 + 0 = R0 unless R0 is -0.0.
// The dead rows' readlanes and adds are left out.
template <int ROWS = 4>
__device__ __forceinline__ double tree_sum(double v) {
    static_assert(ROWS == 1 || ROWS == 2 || ROWS == 4, "live 16-lane rows");
    v = v + xor_lane<1>(v);
    v = v + xor_lane<2>(v);
    v = v + shl_lane<4>(v);
    v = v + xor_lane<8>(v);
    if constexpr (ROWS == 1) return lane_value(v, 0);
    if constexpr (ROWS == 2) return lane_value(v, 0) + lane_value(v, 16);
    return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
}
// the live rows of a column-phase value (lanes >= E are padding) of a compiled shape
constexpr int live_rows(int ET) { return ET > 0 ? (ET <= 16 ? 1 : ET <= 32 ? 2 : 4) : 4; }

// inclusive prefix sum over the lanes in lane order (row_shr DPP inside each 16-lane row, then the
// rows' totals by readlane): a fixed tree order, deterministic, within ~6 u of the exact sums
template <int D>
__device__ __forceinline__ double shr_lane(double v) {  // lane l <- lane l - D of its row, else +0.0
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x110 + D, 0xf, 0xf, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x110 + D, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double wave_scan_d(double v) {
    v = v + shr_lane<1>(v);
    v = v + shr_lane<2>(v);
    v = v + shr_lane<4>(v);
    v = v + shr_lane<8>(v);
    const double r0 = lane_value(v, 15), r1 = lane_value(v, 31), r2 = lane_value(v, 47);
    const int row = threadIdx.x >> 4;
    const double r01 = r0 + r1;
    return row == 0 ? v : v + (row == 1 ? r0 : row == 2 ? r01 : r01 + r2);
}

// ROWS < 4: the lanes from 16 * ROWS on hold the caller's pad (-inf, or 0.0 under values >= 0), which
// a live row's maximum already includes or exceeds: leaving the dead rows out is exact.
template <int ROWS = 4>
__device__ __forceinline__ double wave_max(double v) {
    static_assert(ROWS == 1 || ROWS == 2 || ROWS == 4, "live 16-lane rows");
    v = fmax(v, xor_lane<1>(v));
    v = fmax(v, xor_lane<2>(v));
    v = fmax(v, shl_lane<4>(v));
    v = fmax(v, xor_lane<8>(v));
    if constexpr (ROWS == 1) return lane_value(v, 0);
    if constexpr (ROWS == 2) return fmax(lane_value(v, 0), lane_value(v, 16));
    return fmax(fmax(lane_value(v, 0), lane_value(v, 16)), fmax(lane_value(v, 32), lane_value(v, 48)));
}

// sqrt of a wave-uniform s (a tree_sum, a pairwise sum: the same value on every lane).  The library's
// sqrt scales an argument below 2^-767 by 2^256 and its root back by 2^-128, and passes +-0 and +inf
// through a class test: a compare, two v_ldexp_f64, the class test and three selects around the Newton
// sequence, nine of its 21 instructions.  With 2^-767 <= s < inf (decided on the scalar unit from the
// high word: a negative or NaN s fails the unsigned compare) the scale is zero, both ldexps are the
// identity and the select passes the result through, so the sequence alone is the library's result
// bit for bit: v_rsq_f64, g = s r, h = r / 2, one coupled step, two residual corrections, as in the
// compiler's listing of sqrt for gfx950.  Every other s takes sqrt itself.
__device__ __forceinline__ double sqrt_uniform(double s) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)__double_as_longlong(s) >> 32));
    if (hi - 0x10000000u >= 0x7ff00000u - 0x10000000u) return sqrt(s);
    const double r = __builtin_amdgcn_rsq(s);
    double g = s * r, h = r * 0.5;
    const double e = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, e, g);
    h = __builtin_fma(h, e, h);
    g = __builtin_fma(__builtin_fma(-g, g, s), h, g);
    g = __builtin_fma(__builtin_fma(-g, g, s), h, g);
    return g;
}

__device__ __forceinline__ double catch_(double x, double tol) {  // __init__.py:251-258
    if (x < 1.5 - tol) return 1.0;
    if (x > 1.5 + tol) return 2.0;
    return 1.5;
}

__device__ __forceinline__ double readlane_d(double v, int k) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), k);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ double shr1_d(double v) {  // lane l <- lane l-1 (lane 0 <- 0.0)
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x138, 0xf, 0xf, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x138, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ double permute_d(int dst_lane, double v) {  // forward permute
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(dst_lane * 4, (int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute(dst_lane * 4, (int)(uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ double bpermute_d(int src_lane, double v) {  // lane l <- lane src_lane's v
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane * 4, (int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane * 4, (int)(uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ int mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// numpy pairwise add.reduce (n <= 128 branch: 8 accumulators) of the lanes that
// have `sel` set, taken in lane order.  All 64 lanes call it; every lane gets the
// result.  Register-only: element p (p-th selected lane) is permuted to lane
// 8*(p%8) + p/8, so accumulator k's chain a_k, a_{k+8}, ... sits in lanes 8k..8k+7 and
// runs as a DPP wave_shr chain (each step recomputes final lanes identically); the
// accumulators, the fixed tree and the tail are then read back wave-uniformly.
// Same additions in the same order as numpy (and the C oracle's pw_sum).
__device__ PCX_OUTLINE double wave_pw_sum(double v, bool sel) {
    const int l = lane_id();
    const uint64_t m = ballot(sel);
    const int n = popc(m);
    if (n < 8) {
        double res = 0.0;
        uint64_t mm = m;
        while (mm) {
            const int k = __builtin_ctzll(mm);
            mm &= mm - 1;
            res += readlane_d(v, k);
        }
        return res;
    }
    const int p = sel ? mbcnt64(m) : n + mbcnt64(~m);
    const double a = permute_d((p & 7) * 8 + (p >> 3), v);
    const int T = n >> 3;  // full rounds of 8: positions < 8T feed the accumulators
    double c = a;
    for (int t = 1; t < T; t++) {
        const double prev = shr1_d(c);
        c = (l & 7) == 0 ? a : prev + a;
    }
    const double r0 = readlane_d(c, 0 * 8 + T - 1), r1 = readlane_d(c, 1 * 8 + T - 1);
    const double r2 = readlane_d(c, 2 * 8 + T - 1), r3 = readlane_d(c, 3 * 8 + T - 1);
    const double r4 = readlane_d(c, 4 * 8 + T - 1), r5 = readlane_d(c, 5 * 8 + T - 1);
    const double r6 = readlane_d(c, 6 * 8 + T - 1), r7 = readlane_d(c, 7 * 8 + T - 1);
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (int q = 8 * T; q < n; q++) res += readlane_d(a, (q & 7) * 8 + (q >> 3));
    return res;
}

// wave_pw_sum(v, l < n): the selected lanes are a prefix, so the p-th selected lane is lane p and
// an unselected lane's place n + (l - n) is its own too -- the permute address is an expression of
// the lane alone, with no ballot and no lane counts.  NC > 0: n = NC at compile time, so the n < 8
// branch is decided, the accumulator chain unrolls (T - 1 steps) and the accumulators' and the
// tail's lanes are constants.  NC = 0: n = nrt, wave-uniform.  The additions and their order are
// wave_pw_sum's: eight strided accumulators, the fixed tree, the sequential tail.
template <int NC>
__device__ PCX_OUTLINE double wave_pw_sum_prefix(double v, int nrt) {
    const int l = lane_id();
    const int n = NC > 0 ? NC : nrt;
    if (n < 8) {
        double res = 0.0;
        for (int k = 0; k < n; k++) res += readlane_d(v, k);
        return res;
    }
    const double a = permute_d((l & 7) * 8 + (l >> 3), v);
    const int T = n >> 3;
    double c = a;
    for (int t = 1; t < T; t++) {
        const double prev = shr1_d(c);
        c = (l & 7) == 0 ? a : prev + a;
    }
    const double r0 = readlane_d(c, 0 * 8 + T - 1), r1 = readlane_d(c, 1 * 8 + T - 1);
    const double r2 = readlane_d(c, 2 * 8 + T - 1), r3 = readlane_d(c, 3 * 8 + T - 1);
    const double r4 = readlane_d(c, 4 * 8 + T - 1), r5 = readlane_d(c, 5 * 8 + T - 1);
    const double r6 = readlane_d(c, 6 * 8 + T - 1), r7 = readlane_d(c, 7 * 8 + T - 1);
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (int q = 8 * T; q < n; q++) res += readlane_d(a, (q & 7) * 8 + (q >> 3));
    return res;
}

// numpy's fixed tree over eight accumulators r_k on lanes 8 q + k, k < 8, of a 16-lane row: lane 8 q
// ends with ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), three DPP steps.  Lane 8 q + 1 forms
// r1 + r0 where lane 8 q forms r0 + r1, and so on: the operand order inside an addition does not
// change its bits.  The last step is row_shl:4 alone, since only lane 8 q reads the result.
__device__ __forceinline__ double pw_tree8(double c) {
    c = c + xor_lane<1>(c);
    c = c + xor_lane<2>(c);
    return c + shl_lane<4>(c);
}

// wave_pw_sum_prefix with the accumulator chains in lanes 0..7, the values staged in LDS: lane l
// reads scr[(l & 7) + 8 t] and adds in t order (a compiled shape: one ds_read per step, the offsets
// immediates, all of them issued ahead of the adds), pw_tree8 leaves the tree's result on lane 0,
// the tail is added from LDS broadcast reads, and one readlane pair makes the sum wave-uniform.
// Every chain starts from its first element (no 0.0 enters: a -0.0 stays -0.0).  Same additions in
// the same order as wave_pw_sum_prefix, with no permute, no DPP chain and no readlane per accumulator.
// scr: n doubles of LDS that are dead at the call (the first wsync orders the caller's last reads of
// them before the store).  n < 8 keeps the readlane loop.
template <int NC>
__device__ PCX_OUTLINE double wave_pw_sum_lds(double v, int nrt, double* scr) {
    const int l = lane_id();
    const int n = NC > 0 ? NC : nrt;
    if (n < 8) {
        double res = 0.0;
        for (int k = 0; k < n; k++) res += readlane_d(v, k);
        return res;
    }
    wsync();
    if (l < n) scr[l] = v;
    wsync();
    const int T = n >> 3;
    const double* const p = scr + (l & 7);
    double c = p[0];
    if constexpr (NC > 0) {
#pragma unroll
        for (int t = 1; t < NC / 8; t++) c = c + p[8 * t];
    } else {
        for (int t = 1; t < T; t++) c = c + p[8 * t];
    }
    c = pw_tree8(c);
    for (int q = 8 * T; q < n; q++) c = c + scr[q];  // (lane 0's is the sum; the other lanes' are not read)
    return readlane_d(c, 0);
}

// Two such sums at once, v1 and v2 over the same n lanes: the second sum's values are staged behind
// the first's (scr: 2 n doubles) and its chains, tree and tail run in lanes 8..15 of the same
// instructions.
template <int NC>
__device__ PCX_OUTLINE void wave_pw_sum2_lds(double v1, double v2, int nrt, double* scr, double& s1, double& s2) {
    const int l = lane_id();
    const int n = NC > 0 ? NC : nrt;
    if (n < 8) {
        double r1 = 0.0, r2 = 0.0;
        for (int k = 0; k < n; k++) {
            r1 += readlane_d(v1, k);
            r2 += readlane_d(v2, k);
        }
        s1 = r1;
        s2 = r2;
        return;
    }
    wsync();
    if (l < n) {
        scr[l] = v1;
        scr[n + l] = v2;
    }
    wsync();
    const int T = n >> 3;
    const double* const base = scr + ((l & 8) ? n : 0);
    const double* const p = base + (l & 7);
    double c = p[0];
    if constexpr (NC > 0) {
#pragma unroll
        for (int t = 1; t < NC / 8; t++) c = c + p[8 * t];
    } else {
        for (int t = 1; t < T; t++) c = c + p[8 * t];
    }
    c = pw_tree8(c);
    for (int q = 8 * T; q < n; q++) c = c + base[q];
    s1 = readlane_d(c, 0);
    s2 = readlane_d(c, 8);
}

// wave_pw_sum_prefix for 8 <= n < 24 (T = 1 or 2), registers only: lane k + 8 is row_shl:8 away from
// lane k inside the first DPP row, so the chains are one addition (n >= 16) or none, pw_tree8 leaves
// the tree's result on lane 0, and the tail (lanes 8 T .. n - 1) is read by readlane.  The same
// additions in the same order.  Other lengths take wave_pw_sum_prefix.
template <int NC>
__device__ PCX_OUTLINE double wave_pw_sum_dpp(double v, int nrt) {
    const int n = NC > 0 ? NC : nrt;
    if (n < 8 || n >= 24) return wave_pw_sum_prefix<NC>(v, nrt);
    const int T = n >> 3;
    double c = v;
    if (T == 2) c = v + shl_lane<8>(v);  // (wave-uniform)
    c = pw_tree8(c);
    double res = readlane_d(c, 0);
    for (int q = 8 * T; q < n; q++) res += readlane_d(v, q);
    return res;
}

// SPEC dot2 over rows i < N of column-strided data: a[i] * b[i*bs]
__device__ __forceinline__ double dot2(const double* a, const double* b, int bs, int n) {
    double s = 0.0, c = 0.0;
    for (int i = 0; i < n; i++) {
        const double x = a[i], y = b[i * bs];
        const double p = x * y;
        const double pe = fma(x, y, -p);
        const double t = s + p;
        const double z = t - s;
        const double se = (s - (t - z)) + (p - z);
        s = t;
        c = c + (pe + se);
    }
    return s + c;
}

// np.dot(v, F) for one event column j, in the operation order of numpy 2.2 / OpenBLAS
// 0.3.29 (SkylakeX kernels) in the build container, where the goldens come from -- the
// SPEC's ob_vecmat (oracle/pcx_oracle_batched.c), fitted bit for bit by
// tests/golden/probe_openblas_order.py.  Events j < E & ~3: reporters in blocks of 4, the
// second product rounded then fma with the 1st, 3rd, 4th, y = y + block; tails of 2 / 1.
// The last E % 4 events: a sequential fma chain (E == 2, 3: pairs y + fma(a, x, a' x')).
// E == 1: numpy's ddot (32-wide, then 16-wide fma accumulators, lanes (0+2)+(1+3), fma tail).
__device__ __noinline__ double ob_ddot(const double* v, const double* f, int ld, int n) {
    double acc8[4][8], acc4[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q < 8; q++) acc8[r][q] = 0.0;
    const int n32 = n & -32, n16 = n & -16;
    for (int i = 0; i < n32; i += 32)
#pragma unroll
        for (int k = 0; k < 32; k++) acc8[k / 8][k % 8] = fma(v[i + k], f[(i + k) * ld], acc8[k / 8][k % 8]);
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc4[r][q] = acc8[r][q] + acc8[r][q + 4];
    for (int i = n32; i < n16; i += 16)
#pragma unroll
        for (int k = 0; k < 16; k++) acc4[k / 4][k % 4] = fma(v[i + k], f[(i + k) * ld], acc4[k / 4][k % 4]);
    double A[4];
#pragma unroll
    for (int q = 0; q < 4; q++) A[q] = ((acc4[0][q] + acc4[1][q]) + acc4[2][q]) + acc4[3][q];
    double d = (A[0] + A[2]) + (A[1] + A[3]);
    for (int i = n16; i < n; i++) d = fma(v[i], f[i * ld], d);
    return d;
}

__device__ PCX_OUTLINE double ob_vecmat(const double* v, const double* f, int ld, int N, int E, int j) {
    if (E == 1) return ob_ddot(v, f, ld, N);
    if (j < (E & ~3)) {
        double y = 0.0;
        int n = 0;
        for (; n + 4 <= N; n += 4) {
            double t = f[(n + 1) * ld] * v[n + 1];
            t = fma(f[n * ld], v[n], t);
            t = fma(f[(n + 2) * ld], v[n + 2], t);
            t = fma(f[(n + 3) * ld], v[n + 3], t);
            y = y + t;
        }
        if (n + 2 <= N) {
            double t = f[(n + 1) * ld] * v[n + 1];
            t = fma(f[n * ld], v[n], t);
            y = y + t;
            n += 2;
        }
        if (n < N) y = y + f[n * ld] * v[n];
        return y;
    }
    double t = 0.0;
    int i = 0;
    if (E == 2 || E == 3)
        for (; i + 4 <= N; i += 4) {
            t = t + fma(f[i * ld], v[i], f[(i + 1) * ld] * v[i + 1]);
            t = t + fma(f[(i + 2) * ld], v[i + 2], f[(i + 3) * ld] * v[i + 3]);
        }
    for (; i < N; i++) t = fma(f[i * ld], v[i], t);
    return t;
}

// weightedstats.weighted_median restated (oracle/pcx_oracle.py): lane i holds the
// pair (x, w) if `sel`; W is the builtin sequential sum of the selected weights in
// lane order (computed by the caller).  Scratch: sx, sw (64 doubles each).
__device__ __noinline__ double wave_wmedian(double x, double w, bool sel, double W, double* sx, double* sw) {
    const int l = lane_id();
    const double mid = 0.5 * W;
    const uint64_t dom = ballot(sel && w > mid);
    if (dom) {
        // Python max(weights) then .index(): the first maximal weight
        double mx = wave_max(sel ? w : -__builtin_inf());
        const uint64_t at = ballot(sel && w == mx);
        return bcast(x, __builtin_ctzll(at));
    }
    if (!ballot(sel && w > 0.0)) return __builtin_nan("");
    const uint64_t selm = ballot(sel);
    const int n = popc(selm);
    wsync();
    if (sel) {
        sx[l] = x;
        sw[l] = w;
    }
    wsync();
    int r = 0;
    if (sel) {  // stable rank by (x, w) in numpy's sort order (the SPEC's): a NaN after every number,
        // NaNs equal among themselves -- a total order, so the ranks fill slots 0 .. n - 1
        const bool xin = __builtin_isnan(x), win = __builtin_isnan(w);
        uint64_t rest = selm;
        while (rest) {
            const int mrow = __builtin_ctzll(rest);
            rest &= rest - 1;
            const double xm = sx[mrow], wm = sw[mrow];
            const bool xmn = __builtin_isnan(xm), wmn = __builtin_isnan(wm);
            const bool xlt = (xm < x) || (xin && !xmn), xeq = (xm == x) || (xin && xmn);
            const bool wlt = (wm < w) || (win && !wmn), weq = (wm == w) || (win && wmn);
            r += (xlt || (xeq && (wlt || (weq && mrow < l)))) ? 1 : 0;
        }
    }
    wsync();
    if (sel) {
        sx[r] = x;
        sw[r] = w;
    }
    wsync();
    double res = 0.0;
    if (l == 0) {
        double cum = 0.0;
        int k = 0;
        bool fail = false;
        while (cum <= mid) {
            if (k == n) {
                fail = true;
                break;
            }
            cum += sw[k];
            k++;
        }
        if (fail) {
            res = __builtin_nan("");
        } else {
            const double before = cum - sw[k - 1];
            if (fabs(before - mid) < DBL_EPS) {
                if (k >= 2)
                    res = (sx[k - 2] + sx[k - 1]) / 2.0;
                else
                    res = n == 1 ? sx[0] / 1.0 : __builtin_nan("");
            } else {
                res = sx[k - 1];
            }
        }
    }
    return bcast(res, 0);
}

// The same weighted median as wave_wmedian, with the sort and the walk spread over
// the wave:
//  * rank: every selected lane counts the selected pairs strictly below its own in
//    the (x, w) order, one LDS-broadcast pass over the rows (unselected rows hold
//    (+inf, +inf), which no selected pair exceeds, so they need no mask);
//  * compare-equal pairs share that count; an LDS atomic on a per-rank counter
//    spreads them over [r, r + d).  Equal pairs are bitwise equal here (x and w are
//    never +-0 with equal partners: zero reports are missing), so their order cannot
//    change the walk;
//  * each pair is scattered to its rank (ox, ow), and the cumulative weight runs
//    left to right, eight broadcast loads per step group, stopping at the first
//    cum > mid: the SPEC's sequential sums bit for bit; `before` is the same subtraction.
// NaN keys have no total order: rounds with a NaN among the selected pairs take
// wave_wmedian (in ox / ow).  NR = compile-time row count bound (64 when the shape is dynamic).
// scr: med_scr(NR) doubles of LDS: ox [NR] | ow [med_ow(NR)] | NR int counters
// (ow holds the zero-padded walk groups: every prefetched group of eight).
__host__ __device__ constexpr int med_ow(int NR) { return (NR + 7) / 8 * 8 + 8; }
__host__ __device__ constexpr int med_scr(int NR) { return NR + med_ow(NR) + (NR + 1) / 2; }

// top 32 bits of the order-preserving key of a double (-0.0 folded onto +0.0)
__device__ __forceinline__ uint32_t key_hi32(double x) {
    uint64_t u = __double_as_longlong(x == 0.0 ? 0.0 : x);
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return (uint32_t)(u >> 32);
}

// weightedstats' total (the selected weights summed in row order, an absent row adding +0.0) is
// formed only where a decision needs it.  A tree-order total Wt differs from it by < (N + 6) u Wt,
// so every comparison against mid = Wt / 2 that clears the slack 2^-45 Wt is the one the exact
// total would make.
template <int NR>
__device__ PCX_OUTLINE double wave_wmedian_rank(double x, double w, bool sel, int N, double* scr,
                                                    long long* prof = nullptr) {
    const int l = lane_id();
    double *ox = scr, *ow = scr + NR;
    int* cnt = reinterpret_cast<int*>(scr + NR + med_ow(NR));
    const long long t0 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
    double slack = 0.0;
    // the exact total (row order, an absent row adding +0.0), read lane by lane: a near tie or
    // NaN data only, so it needs no LDS of its own (the sorted pairs may already fill ox / ow)
    auto exact_total = [&]() {
        const double v = sel ? w : 0.0;
        double t = 0.0;
        for (int i = 0; i < N; i++) t = t + readlane_d(v, i);
        slack = 0.0;
        return t;
    };
    double Wtot = tree_sum(sel ? w : 0.0);
    slack = 0x1p-45 * Wtot;
    if (!(slack < __builtin_inf()) || ballot(sel && fabs(w - 0.5 * Wtot) <= slack)) Wtot = exact_total();
    double mid = 0.5 * Wtot;
    if (ballot(sel && w > mid)) {  // weightedstats: a weight above half the total wins outright
        const double mx = wave_max(sel ? w : -__builtin_inf());
        return bcast(x, __builtin_ctzll(ballot(sel && w == mx)));  // first maximal weight
    }
    if (!ballot(sel && w > 0.0)) return __builtin_nan("");
    if (ballot(sel && (__builtin_isnan(x) || __builtin_isnan(w)))) {
        if (slack != 0.0) Wtot = exact_total();
        return wave_wmedian(x, w, sel, Wtot, ox, ow);
    }
    const int n = popc(ballot(sel));
    // rank by the top 32 bits of x's order-preserving key (one 32-bit compare per row,
    // four keys per LDS read; unselected rows hold the largest key, below no selected
    // one); pairs whose keys collide -- the atomic hands a rank out twice -- are rare and
    // take the (x, w) lexicographic pass
    uint32_t* kx = reinterpret_cast<uint32_t*>(ox);
    const uint32_t key = sel ? key_hi32(x) : 0xffffffffu;
    wsync();
    if (l < NR) {
        cnt[l] = 0;
        kx[l] = key;
    }
    for (int q = l; q < med_ow(NR); q += 64) ow[q] = 0.0;  // slots past n add +0.0 in the walk
    wsync();
    int r = 0;
#pragma unroll
    for (int m = 0; m < NR; m++) {
        if (NR == 64 && m >= N) break;
        r += kx[m] < key ? 1 : 0;
    }
    if (sel) atomicAdd(&cnt[r], 1);
    wsync();
    // rows sharing a key (equal x: e.g. the filled guesses of the outcome median, or a
    // 32-bit key collision) are ordered among themselves by (x, w, row), one step per
    // such row
    const bool tied = sel && cnt[r] > 1;
    uint64_t T = ballot(tied);
    int sub = 0;
    // (the tied rows' x, w and rank read from their lanes' registers: no LDS round trip per row)
    while (T) {
        const int m = __builtin_ctzll(T);
        T &= T - 1;
        const double xm = bcast(x, m), wm = bcast(w, m);
        const int rm = __builtin_amdgcn_readlane(r, m);
        const bool before = (xm < x) | ((xm == x) & ((wm < w) | ((wm == w) & (m < l))));
        sub += (tied && rm == r && before) ? 1 : 0;
    }
    if (sel) {
        ox[r + sub] = x;
        ow[r + sub] = w;
    }
    wsync();
    if (prof) {
        const long long t1 = (long long)__builtin_amdgcn_s_memtime();
        prof[0] += t1 - t0;
        prof[2] = t1;
    }
    // wave-uniform walk: cum_k = (((0 + w_0) + w_1) + ... + w_{k-1}), eight sorted
    // weights per step group as LDS broadcasts, the next group's loads issued before
    // the current group's dependent adds
    double cum = 0.0, before = 0.0;
    int k = 0;
    double v[8];  // (the walk's first group: loaded by the branches that walk, the scan-decided case reads none)
    bool walked = false;
    if (!ballot(sel && !(w >= 0.0))) {
        // non-negative weights.  First the prefix sums of the sorted weights in a tree order
        // (slot l on lane l; slots past n hold +0.0): they differ from the walk's sequential
        // sums by < (n + 6) u W, so when the tree sum crossing mid lies more than 2^-44 W above
        // it and its predecessor more than 2^-44 W + DBL_EPS below, the sequential walk crosses
        // at the same slot and the half test below fails -- decided without the serial chain.
        // Otherwise (a near tie) the walk runs.
        const double ps = wave_scan_d(ow[l]);  // (ow holds med_ow(NR) >= 64 slots)
        const double W = lane_value(ps, 63);
        const double margin = 0x1p-44 * W + slack;
        const uint64_t above = ballot(ps > mid);
        if (above) {
            const int j = __builtin_ctzll(above);
            const double sj = bcast(ps, j), sp = j > 0 ? bcast(ps, j - 1) : 0.0;
            if (j < n && sj - mid > margin && (j == 0 || mid - sp > margin + DBL_EPS)) {
                k = j + 1;
                before = j == 0 ? 0.0 : sp;  // j = 0: the walk's c_0 - w_0 = 0 exactly
                walked = true;
            }
        } else if (mid - W > margin) {
            walked = true;  // no crossing: k = 0
        }
    }
    if (!walked && slack != 0.0) {  // a near tie: the walk needs the exact total
        Wtot = exact_total();
        mid = 0.5 * Wtot;
    }
    if (!walked) {
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = ow[q];
    }
    if (walked) {
    } else if (!ballot(sel && !(w >= 0.0))) {
        // non-negative weights: the running sums only grow (slots past n add +0.0), so a
        // group holds the first cum > mid iff its last sum exceeds mid
        for (int t = 0; t < n; t += 8) {
            double nv[8], c[8];
#pragma unroll
            for (int q = 0; q < 8; q++) nv[q] = ow[t + 8 + q];
            c[0] = cum + v[0];
#pragma unroll
            for (int q = 1; q < 8; q++) c[q] = c[q - 1] + v[q];
            if (c[7] > mid) {
                int hit = 7;
#pragma unroll
                for (int q = 6; q >= 0; q--)
                    if (c[q] > mid) hit = q;
                k = t + hit + 1;
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if (q == hit) before = c[q] - v[q];
                break;
            }
            cum = c[7];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = nv[q];
        }
    } else
    for (int t = 0; t < n; t += 8) {
        double nv[8], c[8];
#pragma unroll
        for (int q = 0; q < 8; q++) nv[q] = ow[t + 8 + q];
        c[0] = cum + v[0];
#pragma unroll
        for (int q = 1; q < 8; q++) c[q] = c[q - 1] + v[q];
        int hit = 8;
#pragma unroll
        for (int q = 7; q >= 0; q--)
            if (t + q < n && c[q] > mid) hit = q;
        if (hit < 8) {
            k = t + hit + 1;
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (q == hit) before = c[q] - v[q];
            break;
        }
        cum = c[7];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = nv[q];
    }
    if (prof) prof[1] += (long long)__builtin_amdgcn_s_memtime() - prof[2];
    if (!k) return __builtin_nan("");
    if (fabs(before - mid) < DBL_EPS) {
        if (k >= 2) return (ox[k - 2] + ox[k - 1]) / 2.0;
        return n == 1 ? ox[0] / 1.0 : __builtin_nan("");
    }
    return ox[k - 1];
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, xor_lane32<1>(v));
    v = max(v, xor_lane32<2>(v));
    v = max(v, xor_lane32<4>(v));
    v = max(v, xor_lane32<8>(v));
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return max(max(r0, r1), max(r2, r3));
}

// The prescreen of an interpolation median: the weighted median of the present
// values x under the weights rep / T, decided from 32-bit keys and single-precision sums of the
// unnormalised reputations, with no sort, no division and one LDS store.  Lane l holds row l's
// (x, rep, present); T is the SPEC's sequential total of the present reputations; wf[m] = (float)
// rep_m for every row (written once per round by the caller, every rep_m >= 0); kx: NR keys of
// scratch.  Returns true with the median in `med`, or false: the column takes wave_wmedian_rank.
//   bl_l = sum of wf[m] over the rows whose key is below lane l's (a missing row holds the largest
// key and is below nothing, so wf needs no per-column mask).  It is within 2^-17 T of the exact sum
// of those reputations, and the SPEC's own sums of rep / T and its mid within 2^-44 of that sum / T
// and of 1/2: against the margin M = 2^-16 T a lane with bl < T / 2 - M has the SPEC's running sum
// before its value group at or below mid, and a lane with bl > T / 2 + M above it.  No lane lies
// between (else: refused), the sums are monotone, so the SPEC's crossing element lies in the group
// of the largest key with bl < T / 2 - M, all of whose rows hold one value v (else: refused, a
// collision in the top 32 bits).  First of its group, its `before` is far under mid and the result
// is v; later in the group the half test may pass and the mean is (v + v) / 2 = v.  The SPEC's
// earlier exit (a weight above half the total) and everything near it stay with the sort, as do
// totals outside [2^-100, 2^100] (single precision would lose the small reputations), v = +-0
// (the group may mix the two) and |v| >= 2^1023 (v + v overflows).
template <int NR>
__device__ PCX_OUTLINE bool wave_wmedian_screen(double x, double rep, bool present, double T, int N, uint32_t* kx,
                                                const float* wf, double& med) {
    const int l = lane_id();
    const double half = 0.5 * T, M = 0x1p-16 * T, lo = half - M;
    const uint32_t key = present ? key_hi32(x) : 0xffffffffu;
    wsync();  // (the previous column's reads of kx)
    constexpr int KP = (NR + 3) & ~3;
    if (l < KP) kx[l] = key;  // (the lanes past the last row hold the largest key)
    wsync();
    // two rows per 8-byte LDS read (the scratch is 8-byte aligned in every layout), every read
    // unconditional: written as `kx[m] < key ? wf[m] : 0.f` the weight's read is sunk under the
    // compare, one dependent LDS round trip per row
    const uint2* const kx2 = reinterpret_cast<const uint2*>(kx);
    const float2* const wf2 = reinterpret_cast<const float2*>(wf);
    float bl = 0.f;
#pragma unroll
    for (int m = 0; m < (NR + 1) / 2; m++) {
        if (NR == 64 && 2 * m >= N) break;
        const uint2 k = kx2[m];
        const float2 w = wf2[m];
        bl += k.x < key ? w.x : 0.f;
        bl += k.y < key ? w.y : 0.f;
    }
    const double b = (double)bl;
    const bool range = T >= 0x1p-100 && T <= 0x1p100;  // (a NaN total fails)
    if (ballot(!range || (present && (rep >= lo || fabs(b - half) <= M)))) return false;
    const uint32_t vk = wave_max_u32(present && b < lo ? key : 0u);  // (no present value's key is 0)
    const uint64_t at = ballot(present && key == vk);
    if (!at) return false;
    const double v = bcast(x, __builtin_ctzll(at));
    if (ballot(present && key == vk && x != v)) return false;
    if (!(v != 0.0 && fabs(v) < 0x1p1023)) return false;
    med = v;
    return true;
}


// the N x E round in LDS (row pitch ES) -> dst [N][E] row-major, lane-contiguous: each store
// instruction covers 64 consecutive elements (16-byte pairs when N * E is even and the
// shape is compiled in)
__device__ __forceinline__ void round_to_global(double* dst, const double* F, int N, int E, int ES, int NT, int ET) {
    const int l = lane_id();
    if (NT > 0 && ET > 0 && (NT * ET) % 2 == 0 && ((uintptr_t)dst & 15) == 0) {
        const int tot2 = NT * ET / 2;
        for (int q = l; q < tot2; q += W) {
            const int idx = 2 * q;
            const int i0 = idx / ET, j0 = idx - i0 * ET;
            const int i1 = (idx + 1) / ET, j1 = idx + 1 - i1 * ET;
            reinterpret_cast<double2*>(dst)[q] = double2{F[i0 * ES + j0], F[i1 * ES + j1]};
        }
    } else {
        for (int idx = l; idx < N * E; idx += W) {
            const int i = idx / E, j = idx - i * E;
            dst[idx] = F[i * ES + j];
        }
    }
}

// scipy.stats.rankdata(method='average') of v[0..E) in LDS; lane j < E returns rank j
__device__ PCX_OUTLINE double rank_avg(const double* v, int E) {
    const int l = lane_id();
    double r = 0.0;
    if (l < E) {
        const double x = v[l];
        int lt = 0, eq = 0;
        for (int k = 0; k < E; k++) {
            const double y = v[k];
            lt += y < x;
            eq += y == x;
        }
        r = (double)lt + (double)(eq + 1) * 0.5;
        if (__builtin_isnan(x)) r = __builtin_nan("");  // rankdata propagates NaN: the rule's sums go NaN
    }
    return r;
}

// rank_avg of three vectors in one pass, 3 E <= 64: lane g * E + j ranks entry j of vector g with
// rank_avg's loop and NaN rule, every lane on its own base pointer; r0 is left on lanes [0, E) and
// r1, r2 come down to them by ds_bpermute (lane j + 2 E < 64).  The lanes from E on return values
// nobody reads.
__device__ PCX_OUTLINE void rank_avg3(const double* v0, const double* v1, const double* v2, int E, double& r0,
                                      double& r1, double& r2) {
    const int l = lane_id();
    const int g = (l >= E) + (l >= 2 * E);
    const double* v = g == 0 ? v0 : g == 1 ? v1 : v2;
    double r = 0.0;
    if (l < 3 * E) {
        const double x = v[l - g * E];
        int lt = 0, eq = 0;
        for (int k = 0; k < E; k++) {
            const double y = v[k];
            lt += y < x;
            eq += y == x;
        }
        r = (double)lt + (double)(eq + 1) * 0.5;
        if (__builtin_isnan(x)) r = __builtin_nan("");
    }
    r0 = r;
    r1 = bpermute_d(l + E, r);
    r2 = bpermute_d(l + 2 * E, r);
}

struct Smem {
    double* F;      // [N][ES] rescaled, then filled reports
    double* C;      // [E][ES] covariance (phase aliases: see carve; packed: runs on into M's region)
    double* M;      // [max(E*ES, MED_SCR)] power-iteration / Jacobi working matrix (packed: scratch only)
    double* rep;    // [N] (aliases C: dead once the covariance has its tokens)
    double* n1;     // [N] normalize(set1) (aliases C; packed: M)
    double* n2;     // [N] normalize(set2) (aliases C; packed: M)
    double* smooth; // [N] (aliases C)
    double* mu;     // [E] full layout only (the clusterings' mean; the rest read lane registers)
    double* tot;    // [E] present-reputation totals of the interpolation medians (aliases M)
    double* guess;  // [E] (aliases C)
    double* x;      // [E] full layout only: the Jacobi rotations' cos
    double* ld;     // [E] full layout only: the Jacobi rotations' sin
    double* old;    // [E] (aliases C)
    double* nv1;    // [E] (aliases M)
    double* nv2;    // [E] (aliases M)
    double* adj;    // [E] (aliases C)
    uint64_t* miss; // [E] bit i = report (i, j) is NaN or 0.0 (the per-row / per-column counts
                    // of each kind are lane registers)
};

// LDS per round, by phase.  The kernel is latency bound: throughput scales with the
// rounds resident per CU (tools/occupancy_batched.py), and LDS is what bounds them, so
// vectors whose lifetimes do not overlap the matrices' share their space:
//   C  (covariance, Jacobi V) is live from the covariance to the scores only; before
//      it holds guess | rep (load to fill | load to the covariance's tokens), after it
//      n1 | n2 | smooth | adj | old;
//   M  (squared matrix, Jacobi A) is dead in both median phases, where the median
//      scratch (med_scr doubles) lives, and after the eigenpairs, where nv1 | nv2 live;
//   the power-iteration vector, the loading and the weighted mean are lane registers, read
//      by other lanes through readlane / ds_bpermute (no LDS); the full layout keeps mu
//      (the clusterings read it) and x | ld as the Jacobi rotations' cos | sin.
// The packed layouts (PCA, plain and caller-scored rounds) square the iterated matrix in registers
// (square_scaled_reg) and write its triangle over C for the matrix-vector steps, C's operands
// waiting in registers meanwhile, so no region is sized for a matrix of its own:
//   "C" holds guess | rep before the covariance and smooth | adj | old after the scores;
//   "M" holds the median scratch and the totals in both median phases, n1 | n2 | nv1 | nv2
//      between the scores and the reputation update, then the certainty's hit masks;
//   C, the packed covariance, is live from the covariance to the scores only, when all of
//      those are dead, and spans both regions ("M" directly follows "C").
// 50 x 20: F 1,000 + "C" 90 + "M" 159 + miss 20 = 1,269 doubles = 10,152 bytes, eight units.
// The integer tokens are recomputed from rep where the covariance needs them.  Per-row
// vectors hold N entries, per-event vectors E (rounded up to even).  LDS is allocated in
// 1,280-byte units (160 KiB / 128; measured with PCX_BATCHED_LDS_PAD: a 50 x 20 round of
// 12,800 bytes ran twelve to a CU, one of 13,192 eleven).
__host__ __device__ inline int smem_rows(int N) { return (N + 1) & ~1; }
// F also holds the certainty phase's compacted hit lists, [E][cert_stride] (an odd stride with
// the odd row pitch; the compiled shapes' even pitch keeps N)
__host__ __device__ inline int cert_stride(int N, int ES) { return (ES & 1) ? (N | 1) : N; }
__host__ __device__ inline int smem_f_size(int N, int E, int ES) {
    return N * ES > E * cert_stride(N, ES) ? N * ES : E * cert_stride(N, ES);
}
__host__ __device__ inline int smem_evs(int E) { return (E + 1) & ~1; }
// C and M: full [E][ES] (the Jacobi eigenpairs of big-five / fixed-variance need a
// general V), or -- every other algorithm -- packed lower triangles (both are symmetric:
// the squared M bitwise too).
__host__ __device__ inline int smem_mat(int E, int ES, bool pk) { return pk ? E * (E + 1) / 2 : E * ES; }
// Packed layouts: the squared matrix has no LDS of its own (it shares C's), so one triangle needs
// LDS, from the covariance to the scores, when every vector of both regions is dead: C spans the
// "C" and "M" regions, which are contiguous (carve), and each region is sized for its vectors alone.
__host__ __device__ inline int smem_c_size(int N, int E, int ES, bool pk) {
    if (pk) return smem_rows(N) + 2 * smem_evs(E);  // smooth | adj | old (before: guess | rep)
    const int need = 3 * smem_rows(N) + 2 * smem_evs(E);
    return smem_mat(E, ES, pk) > need ? smem_mat(E, ES, pk) : need;
}
__host__ __device__ inline int smem_m_size(int N, int E, int ES, int NR, bool pk) {
    const int scr = med_scr(NR) + smem_evs(E);  // the median scratch and the totals beside it
    if (pk) {
        const int vec = 2 * smem_rows(N) + 2 * smem_evs(E);  // n1 | n2 | nv1 | nv2
        const int rest = smem_mat(E, ES, pk) - smem_c_size(N, E, ES, pk);  // C's tail past the "C" region
        const int need = scr > vec ? scr : vec;
        return need > rest ? need : rest;
    }
    const int need = scr > 2 * smem_evs(E) ? scr : 2 * smem_evs(E);
    return smem_mat(E, ES, pk) > need ? smem_mat(E, ES, pk) : need;
}

__host__ __device__ inline size_t smem_doubles(int N, int E, int ES, int NR, bool pk) {
    return (size_t)smem_f_size(N, E, ES) + smem_c_size(N, E, ES, pk) + smem_m_size(N, E, ES, NR, pk) +
           (pk ? 1 : 4) * (size_t)smem_evs(E);
}

// entry (j, k) of the symmetric C / M
template <bool PK>
__device__ __forceinline__ int sym_at(int j, int k, int ES) {
    if constexpr (PK)
        return j >= k ? j * (j + 1) / 2 + k : k * (k + 1) / 2 + j;
    else
        return j * ES + k;
}

__device__ Smem carve(double* base, int N, int E, int ES, int NR, bool pk) {
    const int nr = smem_rows(N), ne = smem_evs(E);
    Smem s;
    double* p = base;
    s.F = p; p += smem_f_size(N, E, ES);
    s.C = p; p += smem_c_size(N, E, ES, pk);
    s.M = p; p += smem_m_size(N, E, ES, NR, pk);
    s.miss = reinterpret_cast<uint64_t*>(p); p += ne;
    s.mu = s.x = s.ld = nullptr;
    if (!pk) {
        s.mu = p; p += ne;
        s.x = p; p += ne;
        s.ld = p; p += ne;
    }
    // phase aliases (see above)
    s.tot = s.M + med_scr(NR);
    s.rep = s.C + ne;  // (beside guess, C[0, E))
    s.guess = s.C;
    if (pk) {
        s.smooth = s.C;
        s.adj = s.C + nr;
        s.old = s.C + nr + ne;
        s.n1 = s.M;
        s.n2 = s.M + nr;
        s.nv1 = s.M + 2 * nr;
        s.nv2 = s.M + 2 * nr + ne;
    } else {
        s.n1 = s.C;
        s.n2 = s.C + nr;
        s.smooth = s.C + 2 * nr;
        s.adj = s.C + 3 * nr;
        s.old = s.C + 3 * nr + ne;
        s.nv1 = s.M;
        s.nv2 = s.M + ne;
    }
    return s;
}

// ---- broadcasts inside the 16-lane row, taken by the arithmetic instruction itself ------------
// gfx950's v_fmac_f64 (VOP2) accepts a DPP source with row_newbcast:K: every lane reads lane K of
// its own 16-lane row.  A column-phase vector v (v_k on lane k, E <= 32) is laid out for it once
// by row_spread2 (rows 0 and 1) or row_spread4 (all four rows): lo holds v_(l & 15) and hi holds
// v_(16 + (l & 15)), so column k is lane k & 15 of lo (k < 16) or of hi.  The compiler neither forms
// these instructions nor sees the DPP read inside the statement, so two things are the caller's:
//  (1) wait states: a VALU write of a register needs two wait states before a DPP read of it.  The
//      registers read through DPP here are written by row_spread2 / row_spread4 alone and pass
//      through dpp_ready() (s_nop 1, tied to them as operands) before any statement reads them.
//  (2) EXEC: a source lane that EXEC has switched off is not read, so the statements run with the
//      whole wave active: in wave-uniform control flow only (branches on ballots and scalars), never
//      under `if (col)` or `if (row)`.
struct RowSpread {
    double lo, hi;
};
__device__ __forceinline__ double pack_d(uint32_t lo, uint32_t hi) {
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ void dpp_ready(RowSpread& s) { asm("s_nop 1" : "+v"(s.lo), "+v"(s.hi)); }
// v_permlane16_swap(u, u): the first result is rows [0, 0, 2, 2] of u, the second rows [1, 1, 3, 3]
__device__ __forceinline__ RowSpread row_spread2(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const auto a = __builtin_amdgcn_permlane16_swap((uint32_t)u, (uint32_t)u, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap((uint32_t)(u >> 32), (uint32_t)(u >> 32), false, false);
    RowSpread s = {pack_d(a[0], b[0]), pack_d(a[1], b[1])};
    dpp_ready(s);
    return s;
}
// v_permlane32_swap(w, w): the first result is the lower half of w in both halves
__device__ __forceinline__ RowSpread row_spread4(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const auto a = __builtin_amdgcn_permlane16_swap((uint32_t)u, (uint32_t)u, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap((uint32_t)(u >> 32), (uint32_t)(u >> 32), false, false);
    const uint32_t ll = __builtin_amdgcn_permlane32_swap(a[0], a[0], false, false)[0];
    const uint32_t lh = __builtin_amdgcn_permlane32_swap(b[0], b[0], false, false)[0];
    const uint32_t hl = __builtin_amdgcn_permlane32_swap(a[1], a[1], false, false)[0];
    const uint32_t hh = __builtin_amdgcn_permlane32_swap(b[1], b[1], false, false)[0];
    RowSpread s = {pack_d(ll, lh), pack_d(hl, hh)};
    dpp_ready(s);
    return s;
}
// acc = fma(s_K, m, acc), s_K from the row (one v_fmac_f64: the fused operation of fma(m, s_K, acc));
// NEG: fma(-s_K, m, acc), the negation a source modifier (exact)
template <int K, bool NEG = false>
__device__ __forceinline__ void fmac_rowbcast(double& acc, const RowSpread& s, double m) {
    static_assert(K >= 0 && K < 32, "a column of a two-row vector");
    if constexpr (NEG)
        asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
            : "+v"(acc)
            : "v"(K < 16 ? s.lo : s.hi), "v"(m), "n"(K & 15));
    else
        asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
            : "+v"(acc)
            : "v"(K < 16 ? s.lo : s.hi), "v"(m), "n"(K & 15));
}
// f - s_K as fma(-s_K, 1.0, f): the product is exact, so this is one rounding of f + (-s_K), the
// subtraction's own operation on the same operands (signed zeros, infinities and a NaN s_K included).
// Only v_fmac_f64 has a DPP form among the 64-bit instructions: v_add_f64 and v_mul_f64 are VOP3 and
// take none.  `one` is 1.0 in a register (the instruction has no constant operand in this form).
template <int K>
__device__ __forceinline__ double sub_rowbcast(double f, const RowSpread& s, double one) {
    fmac_rowbcast<K, true>(f, s, one);
    return f;
}
template <int K, int ET, class F>
__device__ __forceinline__ void static_cols(F&& f) {  // f(column constant) for K, K + 1, .. ET - 1
    if constexpr (K < ET) {
        f(std::integral_constant<int, K>());
        static_cols<K + 1, ET>(f);
    }
}
// lane K of v <- the wave-uniform s (v_writelane_b32: a scalar source and a constant lane, so the one
// wait the instruction can need, after a VALU write of a lane-select register, does not arise); the
// other lanes keep v.  One instruction where `l == K ? s : v` is a move, a compare and a select.
template <int K>
__device__ __forceinline__ uint32_t write_lane(uint32_t v, uint32_t s) {
    static_assert(K >= 0 && K < W, "a lane of the wave");
    // (readfirstlane: the operand constraint alone does not keep a uniform value out of a vector register)
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(__builtin_amdgcn_readfirstlane((int)s)), "n"(K));
    return v;
}

// Entry (r, K) of the packed triangle for a constant column K: at tri(r) + K for K <= r, at tri(K) + r
// above the diagonal.  The LDS byte addresses of M[tri(r)] and M[r] are formed once per round
// (sym_base, outside the step loop) and column K selects between them: one compare, one add and one
// select, with 8 K left to the read's offset field.  From sym_at's expression the compiler forms
// max(r, K), min(r, K) and a product for every column, eight instructions each; the empty asm keeps
// it from seeing through the bases.
typedef const __attribute__((address_space(3))) double* LdsDoubles;
struct SymBase {
    uint32_t tri, row;
};
__device__ __forceinline__ SymBase sym_base(const double* M, int r) {
    const uint32_t m = (uint32_t)(uintptr_t)(LdsDoubles)M;
    SymBase b = {m + (uint32_t)(r * (r + 1) / 2 * 8), m + (uint32_t)(r * 8)};
    asm("" : "+v"(b.tri), "+v"(b.row));
    return b;
}
template <bool PK, int K>
__device__ __forceinline__ double sym_col(const double* M, const SymBase& b, int r, int ES) {
    if constexpr (!PK) return M[r * ES + K];
    const uint32_t at = K <= r ? b.tri : b.row + 8u * (K * (K + 1) / 2 - K);
    return ((LdsDoubles)(uintptr_t)at)[K];
}

// y = normalize(M x) for lane j < E, x_k on lane k; returns y_j (0 on other lanes)
// ET in 1..32 (a compiled shape): x is spread over rows 0 and 1 and each column's multiply-add takes
// its x_k by row_newbcast; the lanes of rows 2 and 3 multiply by their own rows' x (0.0: no event
// there) and are dropped like today's.  The sum's terms and their order are the loop's.
template <bool PK, int ROWS = 4, int ET = 0>
__device__ PCX_OUTLINE double matvec_unit(const double* M, int ES, double xv, int E, const SymBase& sb) {
    const int l = lane_id(), r = l < E ? l : 0;  // (every lane runs the chain: the broadcasts are wave-wide)
    double acc = 0.0;
    if constexpr (ET > 0 && ET <= 32) {
        const RowSpread x = row_spread2(xv);
        static_cols<0, ET>([&](auto k) { fmac_rowbcast<k.value>(acc, x, sym_col<PK, k.value>(M, sb, r, ES)); });
    } else {
        for (int k = 0; k < E; k++) acc = fma(M[sym_at<PK>(r, k, ES)], lane_value(xv, k), acc);
    }
    const double y = l < E ? acc : 0.0;
    const double ss = tree_sum<ROWS>(l < E ? y * y : 0.0);  // squares: no row sum is -0.0
    double nrm;
    if constexpr (ET > 0)  // (a compiled shape: the root without the library's range scaling)
        nrm = sqrt_uniform(ss);
    else
        nrm = sqrt(ss);
    return l < E ? y / nrm : 0.0;
}

typedef double d4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ d4v mfma_f64(double a, double b, d4v c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// M <- (M M) / max|M M| (SPEC square_scaled) on fp64 MFMA.  v_mfma_f64_16x16x4_f64
// accumulates exactly like the SPEC's fma chain over m (tools/probes/mfma_f64_order:
// bitwise equal), and the zero padding of the 32 x 32 tile adds exact zeros, so every
// entry is bit-identical to the VALU loop.  E <= 32: a 2 x 2 grid of 16 x 16 tiles.
// M symmetric: A[ml][mm] = B[mm][ml], one read per operand pair.
template <bool PK>
__device__ PCX_OUTLINE void square_scaled(double* M, int ES, int E) {
    const int l = lane_id(), ml = l & 15, kq = l >> 4;
    const bool two = E > 16;
    d4v t00 = {0, 0, 0, 0}, t01 = {0, 0, 0, 0}, t10 = {0, 0, 0, 0}, t11 = {0, 0, 0, 0};
    for (int m0 = 0; m0 < E; m0 += 4) {
        const int mm = m0 + kq;
        const bool ok = mm < E;
        const double a0 = (ok && ml < E) ? M[sym_at<PK>(ml, mm, ES)] : 0.0;
        const double b0 = a0;
        t00 = mfma_f64(a0, b0, t00);
        if (two) {
            const double a1 = (ok && 16 + ml < E) ? M[sym_at<PK>(16 + ml, mm, ES)] : 0.0;
            const double b1 = a1;
            // PK: the upper tile t01 = t10^T bit for bit (the same products in the same m
            // order), neither stored nor needed for the maximum (C3: 1.826 -> 1.786 ms)
            if (!PK) t01 = mfma_f64(a0, b1, t01);
            t10 = mfma_f64(a1, b0, t10);
            t11 = mfma_f64(a1, b1, t11);
        }
    }
    double mx = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int j0 = kq + 4 * r, j1 = 16 + kq + 4 * r, k0 = ml, k1 = 16 + ml;
        if (j0 < E && k0 < E) mx = fmax(mx, fabs(t00[r]));
        if (!PK && j0 < E && k1 < E) mx = fmax(mx, fabs(t01[r]));
        if (j1 < E && k0 < E) mx = fmax(mx, fabs(t10[r]));
        if (j1 < E && k1 < E) mx = fmax(mx, fabs(t11[r]));
    }
    mx = wave_max(mx);
    // SPEC: scale by the power of two that brings max|MM| into [1, 2) (exact); a zero,
    // subnormal or non-finite maximum divides instead
    const bool pow2 = mx >= DBL_MIN_ && __builtin_isfinite(mx);
    const double sc = pow2 ? ldexp(1.0, -ilogb(mx)) : 1.0;
    auto scaled = [&](double t) { return pow2 ? t * sc : (mx > 0.0 ? t / mx : t); };
    wsync();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int j0 = kq + 4 * r, j1 = 16 + kq + 4 * r, k0 = ml, k1 = 16 + ml;
        if (j0 < E && k0 < E && (!PK || k0 <= j0)) M[sym_at<PK>(j0, k0, ES)] = scaled(t00[r]);
        if (j0 < E && k1 < E && !PK) M[sym_at<PK>(j0, k1, ES)] = scaled(t01[r]);
        if (j1 < E && k0 < E) M[sym_at<PK>(j1, k0, ES)] = scaled(t10[r]);
        if (j1 < E && k1 < E && (!PK || k1 <= j1)) M[sym_at<PK>(j1, k1, ES)] = scaled(t11[r]);
    }
    wsync();
}

// ---- packed layouts: the iterated matrix in registers ----------------------------------------
// Lane (ml = l & 15, kq = l >> 4) holds the MFMA operands of k-step s (columns 4s .. 4s + 3) of a
// symmetric E x E matrix M, zero outside it:
//   a0[s] = M[ml][4s + kq]        (row tile 0)
//   a1[s] = M[16 + ml][4s + kq]   (row tile 1, E > 16 only)
// NS = k-steps held: ceil(E / 4) of a compiled shape, 8 otherwise.
template <int NS>
struct SymOps {
    double a0[NS], a1[NS];
};

// the operands of the packed lower triangle C in LDS (the reads square_scaled<true> makes)
template <int NS>
__device__ __forceinline__ void load_sym_ops(const double* C, int E, SymOps<NS>& m) {
    const int l = lane_id(), ml = l & 15, kq = l >> 4;
    const bool two = E > 16;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        m.a0[s] = 0.0;
        m.a1[s] = 0.0;
        if (4 * s < E) {
            const int mm = 4 * s + kq;
            const bool ok = mm < E;
            if (ok && ml < E) m.a0[s] = C[sym_at<true>(ml, mm, 0)];
            if (two && ok && 16 + ml < E) m.a1[s] = C[sym_at<true>(16 + ml, mm, 0)];
        }
    }
}

// the inverse: the operands' lower triangle back into the packed triangle C in LDS
template <int NS>
__device__ __forceinline__ void store_sym_ops(double* C, int E, const SymOps<NS>& m) {
    const int l = lane_id(), ml = l & 15, kq = l >> 4;
    const bool two = E > 16;
    wsync();
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (4 * s < E) {
            const int mm = 4 * s + kq;
            if (mm <= ml && ml < E) C[sym_at<true>(ml, mm, 0)] = m.a0[s];
            if (two && mm <= 16 + ml && 16 + ml < E) C[sym_at<true>(16 + ml, mm, 0)] = m.a1[s];
        }
    }
    wsync();
}

// square_scaled with M in registers, before and after.  The squared matrix is symmetric bit for
// bit (entry (j, k) and (k, j) are the same products in the same m order), and accumulator r of
// a tile is entry (kq + 4r, ml): read as entry (ml, 4r + kq) it IS the next squaring's operand of
// k-step r (t00), of k-step 4 + r in row tile 0 (t10) and in row tile 1 (t11).  Row tile 1's
// operands of the k-steps below 16 are the upper tile t01, a fourth MFMA chain.  No LDS store,
// reload, index arithmetic or wave barrier; the maximum and the scaling as in square_scaled.
template <int NS>
__device__ PCX_OUTLINE void square_scaled_reg(SymOps<NS>& m, int E) {
    const int l = lane_id(), ml = l & 15, kq = l >> 4;
    const bool two = E > 16;
    // E <= 20: t01's live entries (kq + 4r, 16 + ml), ml < 4, are t10's accumulator 0 of lane
    // (4r + kq, kq' = ml) -- four cross-lane moves instead of a fourth MFMA chain
    const bool t01_moves = E <= 20;
    d4v t00 = {0, 0, 0, 0}, t01 = {0, 0, 0, 0}, t10 = {0, 0, 0, 0}, t11 = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (4 * s < E) {
            t00 = mfma_f64(m.a0[s], m.a0[s], t00);
            if (two) {
                if (!t01_moves) t01 = mfma_f64(m.a0[s], m.a1[s], t01);
                t10 = mfma_f64(m.a1[s], m.a0[s], t10);
                t11 = mfma_f64(m.a1[s], m.a1[s], t11);
            }
        }
    }
    double mx = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {  // (t01 holds t10's values)
        const int j0 = kq + 4 * r, j1 = 16 + kq + 4 * r, k0 = ml, k1 = 16 + ml;
        if (j0 < E && k0 < E) mx = fmax(mx, fabs(t00[r]));
        if (j1 < E && k0 < E) mx = fmax(mx, fabs(t10[r]));
        if (j1 < E && k1 < E) mx = fmax(mx, fabs(t11[r]));
    }
    mx = wave_max(mx);
    const bool pow2 = mx >= DBL_MIN_ && __builtin_isfinite(mx);
    const double sc = pow2 ? ldexp(1.0, -ilogb(mx)) : 1.0;
    auto keep = [&](auto scaled) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j0 = kq + 4 * r, j1 = 16 + kq + 4 * r, k0 = ml, k1 = 16 + ml;
            if (r < NS) m.a0[r] = (j0 < E && k0 < E) ? scaled(t00[r]) : 0.0;
            if (two) {
                if (r < NS) {
                    if (t01_moves) {
                        const double s10 = (16 + kq < E && k0 < E) ? scaled(t10[0]) : 0.0;
                        const double v = bpermute_d(16 * (ml & 3) + 4 * r + kq, s10);
                        m.a1[r] = (j0 < E && k1 < E) ? v : 0.0;
                    } else {
                        m.a1[r] = (j0 < E && k1 < E) ? scaled(t01[r]) : 0.0;
                    }
                }
                if (4 + r < NS) {
                    m.a0[4 + r] = (j1 < E && k0 < E) ? scaled(t10[r]) : 0.0;
                    m.a1[4 + r] = (j1 < E && k1 < E) ? scaled(t11[r]) : 0.0;
                }
            }
        }
    };
    if (pow2)  // (wave-uniform: the division stays off the common path)
        keep([&](double t) { return t * sc; });
    else
        keep([&](double t) { return mx > 0.0 ? t / mx : t; });
}

// ---- "big-five" / "fixed-variance" eigenpairs: SPEC jacobi_eig of
// oracle/pcx_oracle_batched.c (cyclic two-sided Jacobi, round-robin pairs; each
// step's angles from the matrix at the step's start, rows then columns), one lane
// per (pair, row/column) element -- the same arithmetic, so bit-identical.
constexpr int JAC_MAXSWEEP = 30;
constexpr double JAC_TOL = 1e-15;

__device__ __forceinline__ void jac_pair(int i, int r, int n, int& p, int& q) {
    const int a = i == 0 ? 0 : 1 + (i - 1 + r) % (n - 1);
    const int b = 1 + (n - 2 - i + r) % (n - 1);
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// A (E x E, row stride ES) -> eigenvalues on its diagonal; V -> eigenvectors (columns).
// pc, ps: rotation cosines and sines, npair <= 16 doubles of LDS each.
__device__ void jacobi_eig_wave(double* A, double* V, int ES, int E, double* pc, double* ps) {
    const int l = lane_id();
    for (int o = l; o < E * E; o += W) {
        const int j = o / E, k = o - j * E;
        V[j * ES + k] = j == k ? 1.0 : 0.0;
    }
    wsync();
    if (E < 2) return;
    const int n = E + (E & 1), npair = n / 2;
    for (int sweep = 0; sweep < JAC_MAXSWEEP; sweep++) {
        double off = 0.0, dg = 0.0;  // max-norms: exact in any order
        for (int o = l; o < E * E; o += W) {
            const int j = o / E, k = o - j * E;
            const double v = fabs(A[j * ES + k]);
            if (j == k)
                dg = fmax(dg, v);
            else
                off = fmax(off, v);
        }
        off = wave_max(off);
        dg = wave_max(dg);
        if (!(off > JAC_TOL * dg)) break;
        for (int r = 0; r < n - 1; r++) {
            if (l < npair) {
                int p, q;
                jac_pair(l, r, n, p, q);
                double c = 1.0, s = 0.0;
                if (q < E) {
                    const double apq = A[p * ES + q];
                    if (apq != 0.0) {
                        const double app = A[p * ES + p], aqq = A[q * ES + q];
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                    }
                }
                pc[l] = c;
                ps[l] = s;
            }
            wsync();
            for (int o = l; o < npair * E; o += W) {  // rows p, q
                const int i = o / E, k = o - i * E;
                const double s = ps[i];
                if (s == 0.0) continue;
                int p, q;
                jac_pair(i, r, n, p, q);
                const double c = pc[i];
                const double apk = A[p * ES + k], aqk = A[q * ES + k];
                A[p * ES + k] = c * apk - s * aqk;
                A[q * ES + k] = s * apk + c * aqk;
            }
            wsync();
            for (int o = l; o < npair * E; o += W) {  // columns p, q of A and V
                const int i = o / E, j = o - i * E;
                const double s = ps[i];
                if (s == 0.0) continue;
                int p, q;
                jac_pair(i, r, n, p, q);
                const double c = pc[i];
                const double ajp = A[j * ES + p], ajq = A[j * ES + q];
                A[j * ES + p] = c * ajp - s * ajq;
                A[j * ES + q] = s * ajp + c * ajq;
                const double vjp = V[j * ES + p], vjq = V[j * ES + q];
                V[j * ES + p] = c * vjp - s * vjq;
                V[j * ES + q] = s * vjp + c * vjq;
            }
            wsync();
        }
    }
}

// ---- clustering algorithms (SPEC: oracle/pcx_oracle_batched.c) ------
// k-means (:392-405), hierarchical (:407-419) and clusterfeck (:148-242, :421-424) each
// turn the filled reports into the nonconformity vector; they run in their own kernel
// instantiation (CLUS = true) with an extra LDS region X, so the PCA kernel is untouched.
constexpr int KMAX = 8;  // k-means code books: ceil(sqrt(64))
constexpr int KMEANS_MAXIT = 4096;  // Lloyd steps per restart (a guard; scipy has none)

__host__ __device__ inline int cluster_lds_doubles(int N, int E, int ES) {
    const int nr = smem_rows(N), ne = smem_evs(E);
    const int feck = N * ES + 6 * nr + 2 * ne;                          // sums, 6 row vectors, outcomes
    const int km = N * ES + 2 * KMAX * ES + ne + 2 * nr + 2 * KMAX;     // obs, books, sd, labels, counts
    return feck > km ? feck : km;
}

// numpy pairwise add.reduce of get(0..n-1) on ONE lane (n <= 128: eight accumulators)
template <class G>
__device__ __forceinline__ double lane_pw_sum(G get, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; i++) r += get(i);
        return r;
    }
    double r0 = get(0), r1 = get(1), r2 = get(2), r3 = get(3), r4 = get(4), r5 = get(5), r6 = get(6), r7 = get(7);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += get(i); r1 += get(i + 1); r2 += get(i + 2); r3 += get(i + 3);
        r4 += get(i + 4); r5 += get(i + 5); r6 += get(i + 6); r7 += get(i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; i++) res += get(i);
    return res;
}

// (size - min size) / sum over the row lanes (:398-405); the integer sum is exact, and
// equal sizes give 0/0 = NaN as numpy does
__device__ __forceinline__ double nc_from_sizes(double size, bool row) {
    const double mn = -wave_max(row ? -size : -__builtin_inf());
    const double tot = tree_sum(row ? size - mn : 0.0);
    return row ? (size - mn) / tot : 0.0;
}

// hierarchical: single-linkage flat clusters at cophenetic distance <= t = connected
// components of {d_ij <= t}, d_ij = sqrt(sequential sum of squared wcd differences)
// (scipy pdist order).  Lane i owns row i's adjacency mask; masks are closed under
// "OR the masks of my members" until no lane changes.
__device__ __noinline__ double hier_nc(const double* F, const double* mu, int ES, int N, int E, double t,
                                       uint64_t* comp) {
    const int l = lane_id();
    const bool row = l < N;
    uint64_t adj = 0;
    if (row) {
        adj = 1ull << l;
        for (int j = 0; j < N; j++) {
            double d2 = 0.0;
            for (int k = 0; k < E; k++) {
                const double df = (F[l * ES + k] - mu[k]) - (F[j * ES + k] - mu[k]);
                d2 = d2 + df * df;
            }
            if (sqrt(d2) <= t) adj |= 1ull << j;
        }
        comp[l] = adj;
    }
    wsync();
    for (;;) {
        uint64_t nw = adj;
        if (row) {
            uint64_t m = adj;
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                nw |= comp[j];
            }
        }
        const bool changed = nw != adj;
        wsync();
        if (row) comp[l] = nw;
        adj = nw;
        wsync();
        if (!ballot(changed)) break;
    }
    return nc_from_sizes(row ? (double)popc(adj) : 0.0, row);
}

// scipy _vq.vq distance^2 as built in the goldens' container: naive for E < 5, else
// -2 x.c (OpenBLAS: one fma chain for K < 32, eight chains + tree at K = 32) + |x|^2 + |c|^2
__device__ __forceinline__ double vq_d2(const double* x, const double* c, int E, double xs, double cs) {
    if (E < 5) {
        double s = 0.0;
        for (int k = 0; k < E; k++) {
            const double d = x[k] - c[k];
            s = s + d * d;
        }
        return s;
    }
    double dot;
    if (E < 32) {
        dot = 0.0;
        for (int k = 0; k < E; k++) dot = fma(x[k], c[k], dot);
    } else {
        double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < E; k += 8)
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (k + u < E) q[u] = fma(x[k + u], c[k + u], q[u]);
        dot = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
    return (-2.0 * dot + xs) + cs;
}

__device__ __forceinline__ double sqsum(const double* x, int E) {
    double s = 0.0;
    for (int k = 0; k < E; k++) s = s + x[k] * x[k];
    return s;
}

// k-means: whiten(wcd), scipy kmeans(obs, k) over the host-drawn restarts (best mean
// distortion, strict <), vq labels, cluster sizes.  Lane i = observation i in vq;
// lanes take (code, feature) pairs in the mean update.
__device__ __noinline__ double kmeans_nc(const BatchArgs& a, int64_t b, const double* F, const double* mu, int ES,
                                         int N, int E, double* X) {
    const int l = lane_id();
    const bool row = l < N, col = l < E;
    const int nr = smem_rows(N), ne = smem_evs(E);
    double* obs = X;                       // [N][ES]
    double* book = obs + N * ES;           // [KMAX][ES]
    double* best = book + KMAX * ES;       // [KMAX][ES]
    double* sd = best + KMAX * ES;         // [E]
    int* lab = reinterpret_cast<int*>(sd + ne);  // [N]
    double* csq = sd + ne + 2 * nr;        // [KMAX]
    int* cntv = reinterpret_cast<int*>(csq + KMAX);  // [KMAX]
    // np.std(wcd, axis=0): sequential column sums (pairwise when E == 1); 0 -> 1
    double sdj = 0.0;
    if (E == 1) {
        const double w = row ? F[l * ES] - mu[0] : 0.0;
        const double m = wave_pw_sum(w, row) / (double)N;
        const double q = row ? (w - m) * (w - m) : 0.0;
        sdj = sqrt(wave_pw_sum(q, row) / (double)N);
    } else if (col) {
        double s = 0.0;
        for (int i = 0; i < N; i++) s = s + (F[i * ES + l] - mu[l]);
        const double m = s / (double)N;
        double v = 0.0;
        for (int i = 0; i < N; i++) {
            const double d = (F[i * ES + l] - mu[l]) - m;
            v = v + d * d;
        }
        sdj = sqrt(v / (double)N);
    }
    if (sdj == 0.0) sdj = 1.0;
    if (col) sd[l] = sdj;
    wsync();
    for (int o = l; o < N * E; o += W) {
        const int i = o / E, k = o - i * E;
        obs[i * ES + k] = (F[i * ES + k] - mu[k]) / sd[k];
    }
    wsync();
    const double xs = row ? sqsum(obs + l * ES, E) : 0.0;
    const int K = a.kmeans_k, RS = a.kmeans_restarts;
    const int32_t* init = a.kmeans_init + b * (int64_t)RS * K;
    double best_d = __builtin_inf();
    int best_n = 0;
    for (int r = 0; r < RS; r++) {
        for (int o = l; o < K * E; o += W) {
            const int c = o / E, k = o - c * E;
            const int row0 = init[r * K + c];
            book[c * ES + k] = obs[(row0 < 0 ? 0 : row0 >= N ? N - 1 : row0) * ES + k];
        }
        int nc = K;
        double prev0 = __builtin_inf(), prev1 = __builtin_inf();
        for (int it = 0;; it++) {
            wsync();
            if (l < nc) csq[l] = sqsum(book + l * ES, E);
            wsync();
            int li = 0;
            double low = __builtin_inf();
            if (row)
                for (int c = 0; c < nc; c++) {
                    const double d = vq_d2(obs + l * ES, book + c * ES, E, xs, csq[c]);
                    if (d < low) {
                        low = d;
                        li = c;
                    }
                }
            const double dist = row ? (low > 0 ? sqrt(low) : 0.0) : 0.0;
            prev0 = prev1;
            prev1 = wave_pw_sum(dist, row) / (double)N;
            if (row) lab[l] = li;
            wsync();
            // update_cluster_means: member sums in row order, / count; empty codes dropped
            int cnt = 0;
            if (l < nc)
                for (int i = 0; i < N; i++) cnt += lab[i] == l;
            const uint64_t nonempty = ballot(l < nc && cnt > 0);
            double nv[4];
            int nk[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int p = l + W * q;
                nk[q] = -1;
                if (p < nc * E) {
                    const int c = p / E, k = p - c * E;
                    double sm = 0.0;
                    int n = 0;
                    for (int i = 0; i < N; i++)
                        if (lab[i] == c) {
                            sm = sm + obs[i * ES + k];
                            n++;
                        }
                    if (n > 0) {
                        nv[q] = sm / (double)n;
                        nk[q] = popc(nonempty & ((1ull << c) - 1)) * ES + k;
                    }
                }
            }
            wsync();
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (nk[q] >= 0) book[nk[q]] = nv[q];
            nc = popc(nonempty);
            if (!(fabs(prev0 - prev1) > 1e-5) || it + 1 >= KMEANS_MAXIT) break;
        }
        wsync();
        if (prev1 < best_d) {
            best_d = prev1;
            best_n = nc;
            for (int o = l; o < nc * ES; o += W) best[o] = book[o];
        }
    }
    wsync();
    if (best_n == 0) return row ? __builtin_nan("") : 0.0;  // no finite distortion: the reference raises
    if (l < best_n) csq[l] = sqsum(best + l * ES, E);
    wsync();
    int li = 0;
    double low = __builtin_inf();
    if (row)
        for (int c = 0; c < best_n; c++) {
            const double d = vq_d2(obs + l * ES, best + c * ES, E, xs, csq[c]);
            if (d < low) {
                low = d;
                li = c;
            }
        }
    if (row) lab[l] = li;
    wsync();
    if (l < best_n) {
        int n = 0;
        for (int i = 0; i < N; i++) n += lab[i] == l;
        cntv[l] = n;
    }
    wsync();
    return nc_from_sizes(row ? (double)cntv[li] : 0.0, row);
}

// clusterfeck: leader clustering of the filled reports with the token weights (0 -> 1e-5),
// mode = heaviest cluster; a mode farther than 1.07 from the weighted outcomes re-clusters
// once at 3x the cut and the closer mode wins; nc = normalize(1 - dist(own cluster, mode) /
// (max + 1e-8)).  Rows are visited in order (wave-uniform); lane x = cluster x.
struct Feck {
    double* sum;   // [N][ES] sum(vec * repVec, axis=0), running in member order
    double* crep;  // [N] running member weight
    int* first;    // [N] founding row (a singleton's meanVec)
    int* count;    // [N]
    int* of;       // [N] cluster of each row, -1 = none
    double* dx;    // [N] per-cluster distance to the mode
    const double* F;
    int ES, E;
    __device__ double mean(int x, int k) const {
        return count[x] == 1 ? F[first[x] * ES + k] : sum[x * ES + k] / crep[x];
    }
};

// one cluster() pass (:194-230); returns the mode (:162-165) and, through dm, the row
// distances of process() (:177-183) for that mode, and the mode's distance to outc
__device__ __noinline__ void feck_pass(Feck& f, const double* wv, int N, double thr, const double* outc, double& dmode,
                                       double& dm) {
    const int l = lane_id(), E = f.E, ES = f.ES;
    const bool col = l < E;
    int ncl = 0;
    for (int i = 0; i < N; i++) {
        const double* Fi = f.F + i * ES;
        const bool valid = l < ncl;
        double d = 0.0;
        if (valid)
            d = sqrt(lane_pw_sum([&](int k) { const double t = Fi[k] - f.mean(l, k); return t * t; }, E));
        const bool cand = valid && d < 0x1p255;
        const double dmin = -wave_max(cand ? -d : -__builtin_inf());
        const uint64_t at = ballot(cand && d == dmin);
        const double wi = wv[i];
        if (at && dmin < thr) {
            const int bx = __builtin_ctzll(at);
            if (col) f.sum[bx * ES + l] = f.sum[bx * ES + l] + Fi[l] * wi;
            wsync();
            if (l == 0) {
                f.crep[bx] = f.crep[bx] + wi;
                f.count[bx] += 1;
                f.of[i] = bx;
            }
        } else if (!ballot(col && __builtin_isnan(Fi[l]))) {
            const int x = ncl++;
            if (col) f.sum[x * ES + l] = Fi[l] * wi;
            if (l == 0) {
                f.first[x] = i;
                f.count[x] = 1;
                f.crep[x] = wi;
                f.of[i] = x;
            }
        } else if (l == 0) {
            f.of[i] = -1;
        }
        wsync();
    }
    const bool valid = l < ncl;
    const double r = valid ? f.crep[l] : 0.0;
    const double top = wave_max(valid ? r : -__builtin_inf());
    const uint64_t tm = ballot(valid && r == top && r > 0.0);
    const int mode = tm ? __builtin_ctzll(tm) : 0;
    dmode = sqrt(lane_pw_sum([&](int k) { const double t = f.mean(mode, k) - outc[k]; return t * t; }, E));
    if (valid) f.dx[l] = sqrt(lane_pw_sum([&](int k) { const double t = f.mean(mode, k) - f.mean(l, k); return t * t; }, E));
    wsync();
    dm = 0.0;
    if (l < N) {
        const int o = f.of[l];
        dm = o >= 0 ? f.dx[o] : 0.0;
    }
    wsync();
}

__device__ __noinline__ double feck_nc(const BatchArgs& a, const double* F, int ES, int N, int E, double rep,
                                       double* X) {
    const int l = lane_id();
    const bool row = l < N, col = l < E;
    const int nr = smem_rows(N), ne = smem_evs(E);
    Feck f;
    f.F = F;
    f.ES = ES;
    f.E = E;
    f.sum = X;
    f.crep = X + N * ES;
    f.first = reinterpret_cast<int*>(f.crep + nr);
    f.count = reinterpret_cast<int*>(f.crep + 2 * nr);
    f.of = reinterpret_cast<int*>(f.crep + 3 * nr);
    f.dx = f.crep + 4 * nr;
    double* wv = f.crep + 5 * nr;
    double* outc = wv + nr;  // [E]
    const double tok = trunc(rep * 1e6);
    const double w = row ? (tok == 0.0 ? 0.00001 : tok) : 0.0;  // :202-204
    if (row) wv[l] = w;
    double thr = a.cluster_threshold;
    if (!(thr > 0.0)) {
        thr = log10((double)E) / 1.77;
        if (thr == 0.0) thr = 0.3;
    }
    // outcomes = np.ma.average(features, axis=0, weights=rep) (:167)
    const double scl = wave_pw_sum(w, row);
    if (E == 1) {
        const double num = wave_pw_sum(row ? F[l * ES] * w : 0.0, row);
        if (l == 0) outc[0] = num / scl;
    }
    wsync();
    if (E > 1 && col) {
        double num = F[l] * wv[0];
        for (int i = 1; i < N; i++) num = num + F[i * ES + l] * wv[i];
        outc[l] = num / scl;
    }
    wsync();
    (void)ne;
    double d1, dm;
    feck_pass(f, wv, N, thr, outc, d1, dm);
    if (d1 > 1.07) {  // :174-176
        double d2, dm2;
        feck_pass(f, wv, N, thr * 3, outc, d2, dm2);
        if (d2 < d1) dm = dm2;
    }
    const double mx = wave_max(row ? dm : -__builtin_inf());
    const double rv = 1.0 - dm / (mx + 0.00000001);
    double u = row ? fabs(rv) : 0.0;
    double Su = wave_pw_sum(u, row);
    if (Su == 0) {
        u += 1.0;
        Su = wave_pw_sum(u, row);
    }
    return row ? u / Su : 0.0;
}

}  // namespace

// The compiled shapes' row pitch: E, not the dynamic shapes' E | 1.  The odd pitch spreads a row-phase
// column read over the banks, but 50 x 20 rounds at the even one fit nine LDS units instead of ten -- 14
// rounds a CU instead of 12 with the 128-VGPR budget of PACKED_WAVES (C3: 1.53 -> 1.46 ms, 42.5 -> 44.6 M
// rounds/s; the even pitch under the three-wave budget, 12 a CU, ran 1.534-1.546 ms against the odd
// pitch's 1.530-1.540: its bank conflicts cost little).
__host__ __device__ constexpr int compiled_es(int E) { return E; }

// wave-uniform 64-bit value into scalar registers
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// (pcx_batched_params.hip includes this file for the helpers above alone: the per-round-parameter
// kernel is a translation unit of its own, so that this unit's kernels keep the code they have)
#ifndef PCX_BATCHED_HELPERS_ONLY
// the round kernel, under its two names (see pcx_batched_round.inc)
#define PCX_ROUND_RAGGED 0
#include "pcx_batched_round.inc"
#undef PCX_ROUND_RAGGED
#define PCX_ROUND_RAGGED 1
#include "pcx_batched_round.inc"
#undef PCX_ROUND_RAGGED

// the launch's instantiation: <50, 20> for the C3 shape, else the dynamic one; packed
// C / M unless the algorithm needs the Jacobi eigenpairs (big-five, fixed-variance) or
// is a clustering one
static bool shape_50x20(int N, int E, int ES) { return N == 50 && E == 20 && ES == 21; }
static bool packed_alg(int alg) { return alg == 0 || alg == 1 || alg == 4; }

size_t batched_lds_bytes(int N, int E, int alg) {
    const bool c50 = shape_50x20(N, E, E | 1) && alg < 5;  // the <50, 20> instantiation
    const int ES = c50 ? compiled_es(E) : E | 1;
    const int NR = c50 ? 50 : 64;
    return smem_doubles(N, E, ES, NR, packed_alg(alg)) * sizeof(double);
}

hipError_t launch_batched(const BatchArgs& a, hipStream_t stream) {
    // PCX_BATCHED_LDS_PAD (diagnostic): extra dynamic LDS bytes per round, to measure
    // throughput against resident rounds per CU (tools/occupancy_batched.py)
    static const size_t pad = [] {
        const char* e = getenv("PCX_BATCHED_LDS_PAD");
        return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)0;
    }();
    size_t lds = batched_lds_bytes(a.N, a.E, a.algorithm) + pad;
    if (a.B <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.B), block(64);
    const bool pk = packed_alg(a.algorithm);
    if (a.algorithm >= 5) {  // clustering algorithms: their own instantiation and LDS region
        lds += sizeof(double) * (size_t)cluster_lds_doubles(a.N, a.E, a.ES);
        static bool attr = [] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&batched_round_kernel<0, 0, true, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        }();
        (void)attr;
        hipLaunchKernelGGL((batched_round_kernel<0, 0, true, false>), grid, block, lds, stream, a);
    } else if (shape_50x20(a.N, a.E, a.ES)) {
        if (pk)
            hipLaunchKernelGGL((batched_round_kernel<50, 20, false, true>), grid, block, lds, stream, a);
        else
            hipLaunchKernelGGL((batched_round_kernel<50, 20, false, false>), grid, block, lds, stream, a);
    } else if (pk) {
        hipLaunchKernelGGL((batched_round_kernel<0, 0, false, true>), grid, block, lds, stream, a);
    } else {
        hipLaunchKernelGGL((batched_round_kernel<0, 0, false, false>), grid, block, lds, stream, a);
    }
    return hipGetLastError();
}

// one N x E round on the generic instantiation (odd pitch, 64 median rows), with the clusterings' region
size_t ragged_lds_bytes(int N, int E, int alg) {
    const int ES = E | 1;
    size_t d = smem_doubles(N, E, ES, 64, packed_alg(alg));
    if (alg >= 5) d += (size_t)cluster_lds_doubles(N, E, ES);
    return d * sizeof(double);
}

hipError_t launch_ragged(const BatchArgs& a, const RaggedDesc* desc, size_t lds, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.B), block(64);
    if (a.algorithm >= 5) {
        static bool attr = [] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&ragged_round_kernel<0, 0, true, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        }();
        (void)attr;
        hipLaunchKernelGGL((ragged_round_kernel<0, 0, true, false>), grid, block, lds, stream, a, desc);
    } else if (packed_alg(a.algorithm)) {
        hipLaunchKernelGGL((ragged_round_kernel<0, 0, false, true>), grid, block, lds, stream, a, desc);
    } else {
        hipLaunchKernelGGL((ragged_round_kernel<0, 0, false, false>), grid, block, lds, stream, a, desc);
    }
    return hipGetLastError();
}
#endif  // PCX_BATCHED_HELPERS_ONLY

}  // namespace pcx
