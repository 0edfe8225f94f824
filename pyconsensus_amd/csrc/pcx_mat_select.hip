// pcx_mat_select.hip -- the weighted medians of the scaled events (M_SEL_*, sel_hist, sel_step).
//
// weightedstats.weighted_median (:303 over the present reports of a scaled event with
// weights rep/sum(rep); :520-523 over the filled column with smooth_rep) in three tiers:
//
//  1. exact selection: an order-preserving u64 key per value, weights as exact fixed-point
//     limbs; 8-bit histogram passes narrow the key range to the run of equal values where
//     the exact prefix crosses half the total.  Every per-rank partial reduces with a plain
//     SUM / MIN / MAX, so the result does not depend on the sharding.
//  2. equal weights (reputation=None: every weight of the column is one double): the
//     reference's float walk depends on the count alone, and pcx_seqsum.h replays it in
//     O(log n) -- crossing index k* and the DBL_EPSILON half test -- after which an exact
//     count selection fetches the k*-th value (and its predecessor for an exact half).
//  3. the exact crossing is decisive unless the prefix at either end of the run lies
//     within the sequential-sum error bound of half the total; such events (and dominant
//     weights at the bound) are "hard" and are replayed in the reference's own float order
//     (k_hard_*: gather in row order, sequential totals, (value, weight) sort, walk).
#include "pcx_mat_device.h"
#include "pcx_seqsum.h"

namespace pcx {
namespace {

constexpr int NB = SEL_NB;       // selection buckets
// rows per load batch of the weight-mode column passes, and the minimum waves per SIMD their
// registers are held to (build parameters for A/B runs).  Measured at C5 (round 6, the phase-2
// first pass): 8 rows, 107 VGPRs, 3.85-3.98 ms; 12 rows (139 VGPRs, 3 waves) 7.44 ms; 16 rows
// (171 VGPRs, 2 waves) 7.77 ms, or held to 4 waves (58 VGPRs spilled) 7.65 ms.
#ifndef PCX_SEL_WUNROLL
#define PCX_SEL_WUNROLL 8
#endif
constexpr int SEL_WUNROLL = PCX_SEL_WUNROLL;
#ifndef PCX_SEL_WWAVES
#define PCX_SEL_WWAVES 1
#endif
constexpr int SEL_HC = 2;  // copies of each k_sel_hist bucket (4: 12.3 vs 9.0 ms at C5; 1: 9.37 vs 8.66 ms, round 5)

// x - y for x >= y (both normalised)
__device__ __forceinline__ L3 l3_sub(L3 x, L3 y) {
    const uint64_t M = (1ull << 43);
    uint64_t c = x.c, b = x.b, a = x.a;
    if (c < y.c) {
        c += M;
        if (b == 0) {
            b += M;
            a -= 1;
        }
        b -= 1;
    }
    c -= y.c;
    if (b < y.b) {
        b += M;
        a -= 1;
    }
    b -= y.b;
    a -= y.a;
    return l3_norm({a, b, c});
}
__device__ __forceinline__ L3 l3_absdiff(L3 x, L3 y) { return l3_cmp(x, y) >= 0 ? l3_sub(x, y) : l3_sub(y, x); }

// |2 P - T| within the sequential-sum error bound of T?  The reference's cumulative
// weights and midpoint are float sums of n terms (each <= (n-1) u sum|w|, weights >= 0;
// phase 1 also divides every weight by a float total): both sides move by < (2n + 2) u T.
// The bound doubles that and adds the weightedstats DBL_EPSILON test (weights sum to ~1).
__device__ __forceinline__ bool near_half(L3 P, L3 T, uint64_t n) {
    const double d = l3_to_double(l3_absdiff(l3_twice(P), T));
    const double t = l3_to_double(T);
    const double bound = t * ((4.0 * (double)n + 64.0) * 0x1p-53) + 16.0 * 0x1p-52;
    return d <= bound;
}

__device__ __forceinline__ XW sel_load(const pcx_mat& m, int s, int64_t i) {
    // phase 1 with reputation=None: every weight is rep = 1 / N (k_rep_local) -- not loaded
    if (m.sel_phase == 1 && !m.rep_raw) return XW{m.T[(int64_t)s * m.n_rows + i], 1.0 / (double)m.n_total};
    return XW{m.T[(int64_t)s * m.n_rows + i], m.sel_phase == 1 ? m.rep[i] : m.rowv[RV_SMOOTH * m.n_rows + i]};
}

__device__ __forceinline__ bool sel_decode(const pcx_mat& m, int s, XW v, double& x, double& w) {
    if (m.sel_phase == 1) {
        if (__builtin_isnan(v.x)) return false;
        x = v.x;
    } else {
        x = __builtin_isnan(v.x) ? m.ev[EV_GUESS * m.n_events + m.scaled_cols[s]] : v.x;
        if (__builtin_isnan(x)) return false;
    }
    w = v.w;
    return true;
}

__device__ __forceinline__ bool sel_elem(const pcx_mat& m, int s, int64_t i, double& x, double& w) {
    return sel_decode(m, s, sel_load(m, s, i), x, w);
}

// phase setup: which scaled events run a selection (phase 1: those with missing reports)
__global__ void __launch_bounds__(BT) k_sel_setup(pcx_mat m) {
    const int s = blockIdx.x * BT + threadIdx.x;
    if (s >= m.n_scaled) return;
    if (s == 0) m.info[IN_SEL_WLIMB] = 0;  // (k_sel_wlimbs ORs this phase's limb use in)
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    const int c = m.scaled_cols[s];
    const bool need = m.sel_phase == 1 ? m.ev[EV_MISS * m.n_events + c] > 0 : true;
    for (int k = 0; k < SELS; k++) st[k] = 0;
    st[SW_STATUS] = need ? 1 : 0;
    st[SW_NEED] = need ? 1 : 0;
    if (m.sel_phase == 2 || need) m.hard[c] = HARD_NONE;
}

__device__ __forceinline__ int shift_for(uint64_t lo, uint64_t hi) {
    const uint64_t d = hi - lo;
    if (d == 0) return 0;
    const int bits = 64 - __clzll(d);
    return bits > 8 ? bits - 8 : 0;
}

// PCX selection init: the key range of every needed event without reading the column --
// phase 1: the present values' extremes (M_COLSTATS, all ranks); phase 2: those and the fill
// value (every missing row takes it, :310-312).  The first histogram pass (sel_first) then
// covers that range and also collects what the reference's walk needs first: the exact total
// weight, the count, the weight extremes and the filled rows' sums.  reputation=None in
// phase 1: every weight is the same double, so that pass counts only (count mode).
__global__ void __launch_bounds__(BT) k_sel_range(pcx_mat m) {
    const int s = blockIdx.x * BT + threadIdx.x;
    if (s >= m.n_scaled) return;
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    if (st[SW_STATUS] != 1) return;
    const int E = (int)m.n_events;
    const int c = m.scaled_cols[s];
    double mn = m.ev[EV_MINX * E + c], mx = m.ev[EV_MAXX * E + c];
    if (m.sel_phase == 2 && m.ev[EV_MISS * E + c] > 0) {
        const double g = m.ev[EV_GUESS * E + c];
        if (!__builtin_isnan(g)) {
            mn = fmin(mn, g);
            mx = fmax(mx, g);
        }
    }
    uint64_t lo = 1, hi = 0;  // no element: an empty range
    if (mn <= mx) {
        lo = dkey(mn);
        hi = dkey(mx);
    }
    st[SW_LO] = lo;
    st[SW_HI] = hi;
    st[SW_SHIFT] = lo <= hi ? shift_for(lo, hi) : 0;
    st[SW_INRANGE] = 0;  // (with SW_COUNT = 0: the first pass never compacts)
    st[SW_COUNT] = 0;
    st[SW_MODE] = (m.sel_phase == 1 && !m.rep_raw) ? 1 : 0;
}


__device__ __forceinline__ void mark_hard(const pcx_mat& m, int s, uint64_t* st) {
    st[SW_STATUS] = 3;
    m.hard[m.scaled_cols[s]] = HARD_MEDIAN;
}

// start: totals of all ranks (already reduced); empty / no positive weight -> None (NaN);
// equal weights -> the reference's walk by pcx_seqsum.h, then a count selection; else the
// dominant-weight test (:any(w > midpoint)) and the exact weight selection
// The totals come from the first pass's histogram (all ranks, reduced): exact integer sums of
// its bucket counts and weight limbs, the extreme keys of its buckets; one thread per event of
// that pass (active index a), whose histogram row k_sel_step then narrows in the same pass.
// One wave per event: the lanes read the histogram row's buckets (coalesced) and reduce the
// exact integer totals and key extremes; lane 0 then decides.
__global__ void __launch_bounds__(BT) k_sel_start(pcx_mat m) {
    const int a = blockIdx.x * (BT / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (a >= (int)m.info[IN_SEL_ACTIVE]) return;  // wave-uniform
    const int s = m.sel_act[a];
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    if (st[SW_STATUS] != 1) return;
    const bool wsum = st[SW_MODE] == 0;  // the first pass summed weight limbs
    const int64_t o = (int64_t)a * NB;
    uint64_t ta = 0, tb = 0, tc = 0, n = 0, kmin = ~0ull, kmax = 0;
    for (int b = lane; b < NB; b += WAVE) {
        const uint64_t c = m.hist_n[o + b];
        if (!c) continue;
        n += c;
        if (wsum) {
            ta += m.hist_w[(o + b) * 3 + 0];
            tb += m.hist_w[(o + b) * 3 + 1];
            tc += m.hist_w[(o + b) * 3 + 2];
        }
        const uint64_t bmin = ~m.hist_min[o + b];  // (stored complemented: one MAX reduce, pcx_internal.h)
        kmin = bmin < kmin ? bmin : kmin;
        kmax = m.hist_max[o + b] > kmax ? m.hist_max[o + b] : kmax;
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {  // exact integer sums: any order
        ta += __shfl_xor(ta, d, WAVE);
        tb += __shfl_xor(tb, d, WAVE);
        tc += __shfl_xor(tc, d, WAVE);
        n += __shfl_xor(n, d, WAVE);
        const uint64_t omn = __shfl_xor(kmin, d, WAVE), omx = __shfl_xor(kmax, d, WAVE);
        kmin = omn < kmin ? omn : kmin;
        kmax = omx > kmax ? omx : kmax;
    }
    if (lane != 0) return;
    const uint64_t wminb = ~m.sel_imin[s * 2 + 1], wmaxb = m.sel_imax[s * 2 + 1];
    // weights outside [0, 2^8) -- a negative reputation (rep / sum(rep) keeps its sign,
    // __init__.py:142-145; smooth_rep inherits it, :472) or one above 256 times the total: the
    // exact limbs hold only [0, 2^8) (pcx_device.h to_limbs), so replay in the reference's order.
    // Over bit patterns (the MAX reduce): a sign bit, or [bits(256), bits(+inf)]; NaN keeps the
    // limb path (NaN limbs are zero, as the generic conversion gives).
    if (wsum && ((wmaxb >> 63) || (wmaxb >= 0x4070000000000000ull && wmaxb <= 0x7ff0000000000000ull))) {
        mark_hard(m, s, st);
        return;
    }
    // count mode known up front (equal weights): the total only needs to be nonzero
    const L3 tot = wsum ? l3_norm({ta, tb, tc}) : L3{n && wmaxb ? 1ull : 0ull, 0, 0};
    if (!wsum && wminb != wmaxb) {  // (cannot happen: reputation=None gives one weight) exact replay
        mark_hard(m, s, st);
        return;
    }
    st_l3(st + SW_TOT0, tot);
    st_l3(st + SW_BELOW0, {0, 0, 0});
    st[SW_BELOW_MAX] = 0;
    st[SW_HAS_BELOW] = 0;
    st[SW_CNT_BELOW] = 0;
    st[SW_WMAX] = wmaxb;
    st[SW_COUNT] = n;
    // SW_LO / SW_HI / SW_SHIFT stay the first pass's (k_sel_step narrows that histogram)
    st[SW_INRANGE] = n;
    if (n == 0 || !(tot.a | tot.b | tot.c)) {  // weighted_median returns None -> NaN
        sel_done(st, __builtin_nan(""));
        return;
    }
    if (wminb == wmaxb) {
        // equal weights: W0 = w (phase 1: w / sequential total, :294-302); mid = 0.5 * sum
        const double w = __longlong_as_double(wmaxb);
        const double W0 = m.sel_phase == 1 ? w / seqsum_const(w, (int64_t)n) : w;
        const double mid = 0.5 * seqsum_const(W0, (int64_t)n);
        if (W0 > mid) {  // dominant weight: data[first argmax] = the first element
            st[SW_STATUS] = 2;
            atomicAdd((unsigned long long*)&m.info[IN_SEL_ARGMAX], 1ull);
            return;
        }
        if (!(W0 > 0.0)) {
            sel_done(st, __builtin_nan(""));
            return;
        }
        const int64_t ks = seqsum_first_above(W0, mid, (int64_t)n);
        const double before = seqsum_const(W0, ks) - W0;
        const bool half = fabs(before - mid) < 2.220446049250313080847e-16;
        st[SW_MODE] = 1;
        st[SW_TARGET] = (uint64_t)(ks - 1);
        st[SW_HALF] = half ? (ks >= 2 ? 1 : (n == 1 ? 0 : 2)) : 0;
    } else {
        const L3 wmax = l3_of(__longlong_as_double(wmaxb));
        if (near_half(wmax, tot, n)) {
            mark_hard(m, s, st);
            return;
        }
        if (l3_cmp(l3_twice(wmax), tot) > 0) {  // any(w > mid)
            st[SW_STATUS] = 2;
            atomicAdd((unsigned long long*)&m.info[IN_SEL_ARGMAX], 1ull);
            return;
        }
        st[SW_MODE] = 0;
    }
    if (kmin == kmax) {  // one distinct value: every crossing returns it
        sel_done(st, st[SW_HALF] == 2 ? __builtin_nan("") : dkey_inv(kmin));
    }
}

// dominant weight: first global row (data order) holding the max weight -> sel_arg[s][0] (MIN)
__global__ void __launch_bounds__(BT) k_sel_argmax(pcx_mat m) {
    const int s = blockIdx.x;
    const uint64_t* st = m.sel_state + (int64_t)s * SELS;
    if (st[SW_STATUS] != 2) return;
    const uint64_t wmaxb = st[SW_WMAX];
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) best = ~0ull;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < m.n_rows; i += BT) {
        double x, w;
        if (sel_elem(m, s, i, x, w) && (uint64_t)__double_as_longlong(w) == wmaxb) {
            atomicMin(&best, (unsigned long long)(m.row_offset + i));
            break;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        m.sel_arg[s] = best;
        m.sel_arg[m.n_scaled + s] = 0;
    }
}

// the rank owning that row publishes its value key -> sel_arg[s][1] (MAX)
__global__ void __launch_bounds__(BT) k_sel_value(pcx_mat m) {
    const int s = blockIdx.x * BT + threadIdx.x;
    if (s >= m.n_scaled) return;
    const uint64_t* st = m.sel_state + (int64_t)s * SELS;
    if (st[SW_STATUS] != 2) return;
    const uint64_t gi = m.sel_arg[s];
    uint64_t key = 0;
    if (gi != ~0ull && (int64_t)gi >= m.row_offset && (int64_t)gi < m.row_offset + m.n_rows) {
        double x, w;
        sel_elem(m, s, (int64_t)gi - m.row_offset, x, w);
        key = dkey(x);
    }
    m.sel_arg[m.n_scaled + s] = key;
}

__global__ void __launch_bounds__(BT) k_sel_value_finish(pcx_mat m) {
    const int s = blockIdx.x * BT + threadIdx.x;
    if (s >= m.n_scaled) return;
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    if (st[SW_STATUS] != 2) return;
    const uint64_t key = m.sel_arg[m.n_scaled + s];
    sel_done(st, key ? dkey_inv(key) : __builtin_nan(""));
}

// active events (status 1) in event order -> sel_act, count -> info[IN_SEL_ACTIVE]; how many
// of them walk weights (not counts) -> info[IN_SEL_WACTIVE] (their limb histograms are exchanged)
__global__ void __launch_bounds__(1024) k_sel_compact(pcx_mat m) {
    __shared__ unsigned long long nw;
    if (threadIdx.x == 0) nw = 0;
    __syncthreads();
    const int64_t cnt = block_compact(
        m.n_scaled, [&](int64_t s) { return m.sel_state[s * SELS + SW_STATUS] == 1; },
        [&](int64_t s, int64_t pos) {
            m.sel_act[pos] = (int32_t)s;
            if (m.sel_state[s * SELS + SW_MODE] == 0) atomicAdd(&nw, 1ull);
        });
    if (threadIdx.x == 0) {
        m.info[IN_SEL_ACTIVE] = cnt;
        m.info[IN_SEL_WACTIVE] = (int64_t)nw;
    }
    // and the events marked for the exact replay so far (k_hard_list's list): after the pass that
    // leaves no event active, the host's one read of info[IN_SEL_ACTIVE ..] also has their count
    if (m.hard_cols) {
        __syncthreads();  // (every thread has read block_compact's count before it is reset)
        const int64_t nh = block_compact(
            m.n_events, [&](int64_t c) { return m.hard[c] != HARD_NONE; },
            [&](int64_t c, int64_t pos) {
                m.hard_cols[pos] = (int32_t)c;
                m.hard_modes[pos] = m.hard[c];
            });
        if (threadIdx.x == 0) m.info[IN_HARD] = nh;
    }
}

// which of the three weight limbs any of this rank's rows uses in this phase (bit 0: L0, bit 2:
// L2; bit 3: computed) -> info[IN_SEL_WLIMB].  k_sel_hist skips the LDS sums of a limb that is zero
// for every row (C5's phase-2 weights, ~1e-6, leave L2 empty): a local saving, the histograms
// and their exchange are unchanged.  (Measured, not kept: the counts carried in L0's sums from
// bit 40 up when both fit, one atomic per element fewer -- 4.16 vs 4.14 ms at C5.)
__global__ void __launch_bounds__(BT) k_sel_wlimbs(pcx_mat m) {
    const double* w = m.sel_phase == 1 ? m.rep : m.rowv + RV_SMOOTH * m.n_rows;
    uint64_t any0 = 0, any2 = 0;
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < m.n_rows; i += (int64_t)gridDim.x * BT) {
        const limbs3 L = to_limbs(w[i]);
        any0 |= L.l0;
        any2 |= L.l2;
    }
    __shared__ unsigned long long bits;
    if (threadIdx.x == 0) bits = 8;
    __syncthreads();
    const bool b0 = __ballot(any0 != 0) != 0, b2 = __ballot(any2 != 0) != 0;
    if (threadIdx.x % WAVE == 0 && (b0 || b2)) atomicOr(&bits, (b0 ? 1ull : 0ull) | (b2 ? 4ull : 0ull));
    __syncthreads();
    // one global atomic per block, and only when it adds a bit (thousands of ORs into one word
    // serialise at its L2 channel: 50 us)
    if (threadIdx.x == 0) {
        unsigned long long* f = (unsigned long long*)&m.info[IN_SEL_WLIMB];
        if ((__atomic_load_n(f, __ATOMIC_RELAXED) & bits) != bits) atomicOr(f, bits);
    }
}

// The first pass's window: a sample of the column (1 / SEL_SAMPLE of its rows, all ranks'
// samples summed) histogrammed in the first pass's buckets; the bucket where the sample's
// weight crosses half, +- SEL_WIN buckets, is the window the first pass also gathers into cbuf.
// When the exact crossing bucket lies inside it (nearly always) the later passes read only
// cbuf -- one read of the column per phase instead of two.  A miss (or a cbuf overflow) only
// falls back to the plain passes: the sample never decides a result.
constexpr int SEL_SAMPLE = 64;
constexpr int SEL_WIN = 3;
__device__ __forceinline__ double* sel_sample_row(const pcx_mat& m, int a) {
    return reinterpret_cast<double*>(m.hist_w) + (int64_t)a * NB * 3;  // [NB] weight, [NB] count
}

__global__ void __launch_bounds__(BT) k_sel_sample(pcx_mat m) {
    const int a = blockIdx.x;
    if (a >= (int)m.info[IN_SEL_ACTIVE]) return;
    const int s = m.sel_act[a];
    const uint64_t* st = m.sel_state + (int64_t)s * SELS;
    __shared__ double sw[NB], sn[NB];
    for (int b = threadIdx.x; b < NB; b += BT) sw[b] = sn[b] = 0.0;
    __syncthreads();
    const uint64_t lo = st[SW_LO], hi = st[SW_HI];
    const int sh = (int)st[SW_SHIFT];
    // runs of SEL_RUN consecutive rows every SEL_RUN * SEL_SAMPLE rows (the same 1/64 of the column
    // as every 64th row, in whole cache lines: a strided sample read a line per element)
    constexpr int SEL_RUN = 16;
    const int64_t span = (int64_t)SEL_RUN * SEL_SAMPLE, full = m.n_rows / span;
    const int64_t rem = m.n_rows - full * span;
    const int64_t ns = full * SEL_RUN + (rem < SEL_RUN ? rem : SEL_RUN);
    for (int64_t j = threadIdx.x; j < ns; j += BT) {
        double x, w;
        const XW v = sel_load(m, s, (j / SEL_RUN) * span + (j % SEL_RUN));
        if (!sel_decode(m, s, v, x, w)) continue;
        const uint64_t k = dkey(x);
        if (k < lo || k > hi) continue;
        const int b = (int)((k - lo) >> sh);
        atomicAdd(&sw[b], w);
        // phase 2: a filled row (all at the fill value) is binned once by k_sel_hist, never
        // gathered into cbuf -- it weighs in the crossing, not in the window's size estimate
        if (!(m.sel_phase == 2 && __builtin_isnan(v.x))) atomicAdd(&sn[b], 1.0);
    }
    __syncthreads();
    double* o = sel_sample_row(m, a);
    for (int b = threadIdx.x; b < NB; b += BT) {
        o[b] = sw[b];
        o[NB + b] = sn[b];
    }
}

// exact weight / count histogram of the keys inside [lo, hi] (NB buckets) of active event a
// One block per active event.  Once the key range holds at most ccap elements (all ranks),
// the pass that reads the whole column also compacts this rank's in-range (key, weight)
// pairs into cbuf; later passes read only those (the histogram is a set of exact integer
// sums / minima / maxima, so the compacted order does not matter).
// NT threads per event: 256, or 1,024 when the active events leave CUs idle (C4: 250 events on 256
// CUs -- one 256-thread workgroup per CU kept four waves streaming each column)
// CM: phase 1 under reputation=None, where every pass counts (every weight is 1 / N): no weight
// loads, limbs or weight extremes, 32-bit counts (n_rows < 2^32, sel_hist), a 16-row load batch
// held to 64 VGPRs (eight waves per SIMD: 2.30 -> 2.03 ms at C5 against 8-row batches; 65 VGPRs
// unforced cost a wave per SIMD)
template <int NT, bool CM>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(CM ? 8 : PCX_SEL_WWAVES))) k_sel_hist(pcx_mat m) {
    const int a = blockIdx.x;
    if (a >= (int)m.info[IN_SEL_ACTIVE]) return;  // the first pass is launched for every scaled event
    const int s = m.sel_act[a];
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    // SEL_HC copies of every bucket, bucket b's copy c at b SEL_HC + c and a thread binning into
    // copy threadIdx.x % SEL_HC: lanes of a wave whose keys share a bucket split over the copies
    // (same-address LDS atomics serialise); the copies merge exactly (integer sums, min, max)
    constexpr int HC = CM ? 4 : SEL_HC;  // (count mode, half the arrays: four copies, 2.38 -> 2.26 ms at C5)
    constexpr int HW = CM ? 1 : NB * HC;
    __shared__ unsigned long long ha[HW], hb[HW], hc[HW], hmin[NB * HC], hmax[NB * HC];
    // (32-bit LDS counts in the weight-mode kernel measured: no faster)
    typedef typename std::conditional<CM, unsigned int, unsigned long long>::type hn_t;
    __shared__ hn_t hn[NB * HC];
    __shared__ unsigned long long gcount, f_wlo, f_whi, f_ga, f_gb, f_gc, f_gn;
    for (int b = threadIdx.x; b < NB * HC; b += NT) {
        if constexpr (!CM) ha[b] = hb[b] = hc[b] = 0;
        hn[b] = 0;
        hmin[b] = ~0ull;
        hmax[b] = 0;
    }
    if (threadIdx.x == 0) {
        gcount = 0;
        f_wlo = ~0ull;
        f_whi = 0;
        f_ga = f_gb = f_gc = f_gn = 0;
    }
    __syncthreads();
    // first pass (sel_first): the weight extremes of every element, and in phase 2 the filled
    // rows (all at the fill value) summed apart and binned once at the end
    const bool first = m.sel_first != 0;
    const bool gfirst = !CM && first && m.sel_phase == 2;
    uint64_t wlo = ~0ull, whi = 0, ga = 0, gb = 0, gc = 0, gn = 0;
    __shared__ int win_s[2];
    if (first && threadIdx.x == 0) {  // the sampled window (k_sel_sample, all ranks)
        const double* smp = sel_sample_row(m, a);
        const bool wm = st[SW_MODE] == 0;
        double tot = 0.0;
        for (int b = 0; b < NB; b++) tot += wm ? smp[b] : smp[NB + b];
        int b0 = 1, b1 = 0;  // empty
        if (tot > 0.0 && m.cbuf) {
            double cum = 0.0;
            int bx = NB - 1;
            for (int b = 0; b < NB; b++) {
                cum += wm ? smp[b] : smp[NB + b];
                if (2.0 * cum >= tot) {
                    bx = b;
                    break;
                }
            }
            // widen by up to SEL_WIN buckets a side while this rank's estimated share of the
            // window (sampled count x SEL_SAMPLE / world) stays within half of cbuf; a crossing
            // bucket denser than that gets no window (the plain passes narrow it first)
            // (and within 1/8 of the column: a wider window re-reads about as much from cbuf
            // as the plain pass reads from the column, after paying for the gather)
            const double share = fmin(0.5 * (double)m.ccap, (double)m.n_rows / 8.0);
            const double cap = share * (double)m.world / (double)SEL_SAMPLE;
            double est = smp[NB + bx];
            if (est <= cap) {
                b0 = b1 = bx;
                for (int r = 1; r <= SEL_WIN; r++) {
                    const double l = bx - r >= 0 ? smp[NB + bx - r] : 0.0;
                    const double h = bx + r < NB ? smp[NB + bx + r] : 0.0;
                    if (est + l + h > cap) break;
                    est += l + h;
                    b0 = bx - r >= 0 ? bx - r : 0;
                    b1 = bx + r < NB ? bx + r : NB - 1;
                }
            }
        }
        win_s[0] = b0;
        win_s[1] = b1;
        st[SW_WB0] = (uint64_t)b0;
        st[SW_WB1] = (uint64_t)b1;
    }
    __syncthreads();
    const int wb0 = first ? win_s[0] : 1, wb1 = first ? win_s[1] : 0;
    const bool wgather = first && wb0 <= wb1;
    const uint64_t lo = st[SW_LO], hi = st[SW_HI];
    const int sh = (int)st[SW_SHIFT];
    const bool wmode = !CM && st[SW_MODE] == 0;
    const bool from_buf = st[SW_CMODE] == 1;
    // phase 2: the filled rows all sit at the fill value -- binned once, not per element
    const bool gties = !CM && m.sel_phase == 2 && st[SW_GN] > 0;
    const uint64_t gk = gties ? dkey(m.ev[EV_GUESS * m.n_events + m.scaled_cols[s]]) : 0;
    const bool gin = gties && gk >= lo && gk <= hi;
    const uint64_t ties_all = gin ? (uint64_t)m.ev[EV_MISS * m.n_events + m.scaled_cols[s]] : 0;  // all ranks
    const uint64_t need = st[SW_INRANGE] > ties_all ? st[SW_INRANGE] - ties_all : 0;
    // gather only once the range has narrowed: later passes then read 16 B per in-range element
    // instead of the column, which pays when the range holds a small part of it (a shard whose
    // whole column fits cbuf would otherwise gather everything and re-read it per pass)
    const bool gather = !from_buf && m.cbuf && st[SW_INRANGE] > 0 && need <= (uint64_t)m.ccap &&
                        8 * need <= st[SW_COUNT];
    uint64_t* cb = m.cbuf ? m.cbuf + (int64_t)s * m.ccap * 2 : nullptr;
    const int hcp = HC > 1 ? (int)(threadIdx.x % HC) : 0;
    const int64_t wl = CM ? 0 : m.info[IN_SEL_WLIMB];  // (k_sel_wlimbs: a limb no row uses is not summed)
    const bool use0 = !(wl & 8) || (wl & 1), use2 = !(wl & 8) || (wl & 4);
    // Phase 2's first pass bins the present values of phase 1's first pass (the same rows, the
    // same keys) plus the filled rows, which it bins apart: over the same range and shift the
    // buckets' counts and key extremes of the present values are the ones phase 1 counted.  Phase
    // 1's first pass keeps them (this rank's, before the reduction: vsave), and phase 2's takes
    // them instead of three LDS atomics per element -- the weight limbs are new, the rest is not.
    // (A filled row's fill value may lie outside phase 1's range, int_dtype truncating it: a
    // changed range recounts.)
    uint64_t* const vkey = m.vsave ? m.vsave + (int64_t)m.n_scaled * NB * 3 + (int64_t)s * 4 : nullptr;
    const bool vput = first && m.sel_phase == 1 && vkey;
    const bool vreuse = !CM && first && m.sel_phase == 2 && vkey && vkey[3] == 1 && vkey[0] == lo &&
                        vkey[1] == hi && vkey[2] == (uint64_t)sh;
    auto bin = [&](uint64_t k, double w) {
        const int b = (int)((k - lo) >> sh) * HC + hcp;
        if constexpr (!CM) {
            if (wmode) {
                const limbs3 L = to_limbs(w);
                if (use0) atomicAdd(&ha[b], (unsigned long long)L.l0);
                atomicAdd(&hb[b], (unsigned long long)L.l1);
                if (use2) atomicAdd(&hc[b], (unsigned long long)L.l2);
            }
        }
        if (!CM && vreuse) return;
        atomicAdd(&hn[b], (hn_t)1);
        // (measured: reading the extremes first and skipping the atomics that cannot change them
        // is slower, 9.4 -> 12.0 ms at C5 -- the read's latency sits in every element's path,
        // where the no-return atomics are fire-and-forget; min / max interleaved in one array,
        // 9.4 -> 9.7 ms -- twice the bank conflicts of two arrays; exact extremes only inside the
        // sampled window, nominal bounds elsewhere, 9.4 -> 9.7 ms)
        atomicMin(&hmin[b], (unsigned long long)k);
        atomicMax(&hmax[b], (unsigned long long)k);
    };
    if (from_buf) {
        const int64_t nc = m.ccount[s];
        for (int64_t j = threadIdx.x; j < nc; j += NT) {
            const uint64_t k = cb[2 * j];
            if (k < lo || k > hi) continue;
            bin(k, __longlong_as_double(cb[2 * j + 1]));
        }
    } else {
        const double* const tcol = m.T + (int64_t)s * m.n_rows;
        const double wc = 1.0 / (double)m.n_total;  // (CM: sel_load's weight)
        rows_strided<(CM ? 16 : SEL_WUNROLL)>(threadIdx.x, NT, m.n_rows, [&](int64_t i) {
                                     if constexpr (CM) return XW{tcol[i], wc};
                                     else return sel_load(m, s, i);
                                 },
                                 [&](int64_t, XW v) {
            double x, w;
            if (gties && __builtin_isnan(v.x)) return;  // a filled row
            if constexpr (CM) {
                if (__builtin_isnan(v.x)) return;
                x = v.x;
                w = v.w;
            } else if (!sel_decode(m, s, v, x, w)) return;
            if (!CM && first) {
                const uint64_t wb = (uint64_t)__double_as_longlong(w);  // weights >= 0 order like their bits
                wlo = wb < wlo ? wb : wlo;
                whi = wb > whi ? wb : whi;
                if (gfirst && __builtin_isnan(v.x)) {  // a filled row: summed here, binned once below
                    if (wmode) {
                        const limbs3 L = to_limbs(w);
                        ga += L.l0;
                        gb += L.l1;
                        gc += L.l2;
                    }
                    gn++;
                    return;
                }
            }
            const uint64_t k = dkey(x);
            if (k < lo || k > hi) return;
            bin(k, w);
            if (wgather || gather) {
                const int b = (int)((k - lo) >> sh);
                const bool put = gather || (b >= wb0 && b <= wb1);
                // one LDS atomic per wave: the lanes that append take consecutive slots
                const uint64_t pm = __ballot(put);
                if (pm) {
                    const int lead = __ffsll((long long)pm) - 1;
                    const int lane = threadIdx.x % WAVE;
                    unsigned long long base = 0;
                    if (lane == lead) base = atomicAdd(&gcount, (unsigned long long)__popcll(pm));
                    base = (unsigned long long)__shfl((long long)base, lead, WAVE);
                    const unsigned long long j = base + __popcll(pm & ((1ull << lane) - 1ull));
                    if (put && j < (unsigned long long)m.ccap) {
                        cb[2 * j] = k;
                        cb[2 * j + 1] = (uint64_t)__double_as_longlong(w);
                    }
                }
            }
        });
    }
    if (first) {
        if (CM) wlo = whi = (uint64_t)__double_as_longlong(1.0 / (double)m.n_total);
        atomicMin(&f_wlo, (unsigned long long)wlo);
        atomicMax(&f_whi, (unsigned long long)whi);
        if (gn) {
            atomicAdd(&f_ga, (unsigned long long)ga);
            atomicAdd(&f_gb, (unsigned long long)gb);
            atomicAdd(&f_gc, (unsigned long long)gc);
            atomicAdd(&f_gn, (unsigned long long)gn);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            m.sel_imin[s * 2 + 1] = ~f_wlo;  // all ranks: (complemented) MAX before k_sel_start
            m.sel_imax[s * 2 + 1] = f_whi;
            if (!CM && f_gn) {  // this rank's filled rows, all at the fill value (inside [lo, hi])
                st[SW_GN] = f_gn;
                st[SW_GW0] = f_ga;
                st[SW_GW1] = f_gb;
                st[SW_GW2] = f_gc;
                const uint64_t fk = dkey(m.ev[EV_GUESS * m.n_events + m.scaled_cols[s]]);
                const int b = (int)((fk - lo) >> sh) * HC;
                if constexpr (!CM) {
                    if (wmode) {
                        atomicAdd(&ha[b], f_ga);
                        atomicAdd(&hb[b], f_gb);
                        atomicAdd(&hc[b], f_gc);
                    }
                }
                atomicAdd(&hn[b], (hn_t)f_gn);
                atomicMin(&hmin[b], (unsigned long long)fk);
                atomicMax(&hmax[b], (unsigned long long)fk);
            }
        }
    }
    if (gin && threadIdx.x == 0) {
        const int b = (int)((gk - lo) >> sh) * HC;
        if constexpr (!CM) {
            if (wmode) {
                atomicAdd(&ha[b], (unsigned long long)st[SW_GW0]);
                atomicAdd(&hb[b], (unsigned long long)st[SW_GW1]);
                atomicAdd(&hc[b], (unsigned long long)st[SW_GW2]);
            }
        }
        atomicAdd(&hn[b], (hn_t)st[SW_GN]);
        atomicMin(&hmin[b], (unsigned long long)gk);
        atomicMax(&hmax[b], (unsigned long long)gk);
    }
    __syncthreads();
    if (gather && threadIdx.x == 0) {
        m.ccount[s] = (int64_t)gcount;
        st[SW_CMODE] = 1;
    }
    if (wgather && threadIdx.x == 0) {  // pending: valid once the crossing bucket is inside the window
        const bool fits = gcount <= (unsigned long long)m.ccap;
        m.ccount[s] = fits ? (int64_t)gcount : 0;
        st[SW_CMODE] = fits ? 2 : 0;
    }
    if (vput && threadIdx.x == 0) {
        vkey[0] = lo;
        vkey[1] = hi;
        vkey[2] = (uint64_t)sh;
        vkey[3] = 1;
    }
    const int64_t o = (int64_t)a * NB;
    for (int b = threadIdx.x; b < NB; b += NT) {
        unsigned long long sa = 0, sb = 0, sc = 0, mn = ~0ull, mx = 0;
        uint64_t sn = 0;
#pragma unroll
        for (int c = 0; c < HC; c++) {
            if constexpr (!CM) {
                sa += ha[b * HC + c];
                sb += hb[b * HC + c];
                sc += hc[b * HC + c];
            }
            sn += (uint64_t)hn[b * HC + c];
            mn = hmin[b * HC + c] < mn ? hmin[b * HC + c] : mn;
            mx = hmax[b * HC + c] > mx ? hmax[b * HC + c] : mx;
        }
        uint64_t* const vs = m.vsave ? m.vsave + ((int64_t)s * NB + b) * 3 : nullptr;
        if (vput) {  // this rank's present values of the range (before the reduction over ranks)
            vs[0] = sn;
            vs[1] = mn;
            vs[2] = mx;
        } else if (vreuse) {
            sn += vs[0];
            mn = vs[1] < mn ? vs[1] : mn;
            mx = vs[2] > mx ? vs[2] : mx;
        }
        if (wmode) {
            m.hist_w[(o + b) * 3 + 0] = sa;
            m.hist_w[(o + b) * 3 + 1] = sb;
            m.hist_w[(o + b) * 3 + 2] = sc;
        }
        m.hist_n[o + b] = sn;
        m.hist_min[o + b] = ~mn;  // complemented: the ranks' minima and maxima reduce in one MAX
        m.hist_max[o + b] = mx;
    }
}

// walk the buckets (reduced over ranks): weight mode keeps the bucket where the exact
// prefix crosses half the total, count mode the one holding rank `target`; a single-key
// bucket resolves (weight mode: unless the crossing is near a rounding-decided half)
// one wave per active event: lane l owns buckets PB*l .. PB*l+PB-1.  The exact prefix sums
// of the bucket counts and weight limbs come from a wave scan (integer limbs: order-free), the
// first bucket whose prefix crosses the half (weights) / target (counts) by ballot, and that
// bucket's lane applies the narrowing (a 256-step serial scan per event before).
constexpr int SEL_PB = NB / WAVE;
__device__ __forceinline__ uint64_t scan_add_u64(uint64_t v, int lane) {  // inclusive
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint64_t u = __shfl_up(v, d, WAVE);
        if (lane >= d) v += u;
    }
    return v;
}
__device__ __forceinline__ uint64_t scan_max_u64(uint64_t v, int lane) {  // inclusive
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint64_t u = __shfl_up(v, d, WAVE);
        if (lane >= d) v = u > v ? u : v;
    }
    return v;
}

__global__ void __launch_bounds__(BT) k_sel_step(pcx_mat m, int n_active) {
    const int a = blockIdx.x * (BT / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (a >= n_active || a >= (int)m.info[IN_SEL_ACTIVE]) return;  // wave-uniform
    const int s = m.sel_act[a];
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    if (st[SW_STATUS] != 1) return;  // the first pass's start may have finished it
    const bool wmode = st[SW_MODE] == 0;
    const L3 tot = ld_l3(st + SW_TOT0);
    const uint64_t n_all = st[SW_COUNT], target = st[SW_TARGET];
    const L3 below0 = ld_l3(st + SW_BELOW0);
    const uint64_t cbelow0 = st[SW_CNT_BELOW], below_max0 = st[SW_BELOW_MAX];
    const bool has_below0 = st[SW_HAS_BELOW] != 0;
    const int64_t o = (int64_t)a * NB;
    uint64_t nb[SEL_PB], kmn[SEL_PB], kmx[SEL_PB];
    L3 hw[SEL_PB];
    uint64_t sc = 0, sa = 0, sb = 0, sl = 0, smax = 0;  // lane totals (counts, limbs), last key
#pragma unroll
    for (int j = 0; j < SEL_PB; j++) {
        const int b = lane * SEL_PB + j;
        nb[j] = m.hist_n[o + b];
        const uint64_t* hs = m.hist_w + (o + b) * 3;
        hw[j] = (wmode && nb[j]) ? l3_norm({hs[0], hs[1], hs[2]}) : L3{0, 0, 0};
        kmn[j] = ~m.hist_min[o + b];
        kmx[j] = m.hist_max[o + b];
        sc += nb[j];
        sa += hw[j].a;
        sb += hw[j].b;
        sl += hw[j].c;
        if (nb[j]) smax = kmx[j];  // keys rise with the bucket index
    }
    // exclusive prefixes over the lanes below
    const uint64_t ic = scan_add_u64(sc, lane), ia = scan_add_u64(sa, lane), ib = scan_add_u64(sb, lane),
                   il = scan_add_u64(sl, lane), imax = scan_max_u64(smax, lane);
    uint64_t pc = ic - sc, pa = ia - sa, pb = ib - sb, pl = il - sl;
    uint64_t pmax = __shfl_up(imax, 1, WAVE);
    if (lane == 0) pmax = 0;
    int first = SEL_PB;  // this lane's first crossing bucket
    L3 below{}, upto{};
    uint64_t cbelow = 0, below_max = 0;
    bool has_below = false;
#pragma unroll
    for (int j = 0; j < SEL_PB; j++) {
        const L3 bl = l3_norm({below0.a + pa, below0.b + pb, below0.c + pl});
        const L3 up = l3_norm({bl.a + hw[j].a, bl.b + hw[j].b, bl.c + hw[j].c});
        const bool cross = nb[j] && (wmode ? l3_cmp(l3_twice(up), tot) > 0 : cbelow0 + pc + nb[j] > target);
        if (cross && first == SEL_PB) {
            first = j;
            below = bl;
            upto = up;
            cbelow = cbelow0 + pc;
            const bool any = pmax != 0 || pc != 0;  // nonempty buckets passed in this pass
            below_max = any ? pmax : below_max0;
            has_below = has_below0 || any;
        }
        pc += nb[j];
        pa += hw[j].a;
        pb += hw[j].b;
        pl += hw[j].c;
        if (nb[j]) pmax = kmx[j];
    }
    const uint64_t mask = __ballot(first < SEL_PB);
    if (mask == 0) {  // no crossing (cannot happen with exact sums)
        if (lane == 0) sel_done(st, __builtin_nan(""));
        return;
    }
    if (lane != __ffsll((long long)mask) - 1) return;
    const uint64_t n = nb[first], kmin = kmn[first], kmax = kmx[first];
    if (kmin == kmax) {
        const double xs = dkey_inv(kmin);
        if (wmode) {
            if (near_half(below, tot, n_all) || near_half(upto, tot, n_all)) {
                mark_hard(m, s, st);
                return;
            }
            if (m.sel_phase == 2) {  // every element equal to the outcome is in this bucket
                st[SW_CERTN] = n;
                st_l3(st + SW_CW0, hw[first]);
            }
            sel_done(st, xs);
        } else {
            double r = xs;
            if (st[SW_HALF] == 2) {
                r = __builtin_nan("");
            } else if (st[SW_HALF] == 1) {
                const double pred = target >= cbelow + 1 ? xs : dkey_inv(below_max);
                r = (pred + xs) / 2.0;  // sum(bounds) / float(len(bounds))
            }
            sel_done(st, r);
        }
    } else {
        // the first pass's window holds this rank's elements of the crossing bucket when the
        // bucket lies inside it: later passes read cbuf (else the column, as without a window)
        if (st[SW_CMODE] == 2) {
            const int b = lane * SEL_PB + first;
            st[SW_CMODE] = (b >= (int)st[SW_WB0] && b <= (int)st[SW_WB1]) ? 1 : 0;
        }
        st[SW_LO] = kmin;
        st[SW_HI] = kmax;
        st[SW_SHIFT] = shift_for(kmin, kmax);
        st[SW_INRANGE] = n;
        st_l3(st + SW_BELOW0, below);
        st[SW_CNT_BELOW] = cbelow;
        st[SW_BELOW_MAX] = below_max;
        st[SW_HAS_BELOW] = has_below ? 1 : 0;
    }
}

// results into guess (phase 1; int dtype truncates, :312) / outcomes (phase 2, :537-538)
__global__ void __launch_bounds__(BT) k_sel_finish(pcx_mat m) {
    const int s = blockIdx.x * BT + threadIdx.x;
    if (s >= m.n_scaled) return;
    const int E = (int)m.n_events;
    const int c = m.scaled_cols[s];
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    const double r = __longlong_as_double(st[SW_RESULT]);
    if (m.sel_phase == 1) {
        if (st[SW_NEED]) m.ev[EV_GUESS * E + c] = m.int_dtype ? trunc(r) : r;
    } else {
        m.ev[EV_RAW * E + c] = r;
        m.ev[EV_ADJ * E + c] = r;
        double f = r * (m.hi[c] - m.lo[c]);  // :537-538, two roundings
        f = f + m.lo[c];
        m.ev[EV_FIN * E + c] = f;
    }
}

// Exact replay of weightedstats.weighted_median with the reference's float arithmetic,
// for one scaled event whose element count fits the block (n <= SEL_EXACT_MAX; single
// rank).  Phase 1 (:287-303): weights rep_j / (sequential sum of present rep), over the
// present reports in row order.  Phase 2 (:520-523): weights smooth_rep over all rows.
// mid = 0.5 * builtin sum (row order); dominant weight -> first argmax; else bitonic sort
// by (value, weight) and the sequential walk with the DBL_EPSILON exact-half test.
__global__ void __launch_bounds__(1024) k_sel_exact(pcx_mat m) {
    const int s = blockIdx.x;
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    if (st[SW_STATUS] == 0) return;
    __shared__ double xs[SEL_EXACT_MAX];
    __shared__ double ws[SEL_EXACT_MAX];
    __shared__ uint32_t pres[SEL_EXACT_MAX / 32];  // the rows' present bits (phase 1: a report; 2: a value)
    __shared__ int cnt;
    __shared__ double mid_s, wmax_s;
    __shared__ int first_s;
    const int tid = threadIdx.x;
    const int n_rows = (int)m.n_rows;
    // the column's (x, w) in row order into LDS by every thread (coalesced; thread 0 read them one
    // dependent global load at a time: 0.7 ms of a 1k x 100 consensus), the present bits beside;
    // an absent row holds (+inf, +inf), which the sort puts after every present pair, so nothing is
    // compacted (an in-place compaction by one thread waited on its own LDS stores)
    const bool ph1 = m.sel_phase == 1;
    for (int k = tid; k < SEL_EXACT_MAX / 32; k += 1024) pres[k] = 0;
    __syncthreads();
    for (int i = tid; i < n_rows; i += 1024) {
        double x = 0.0, w = 0.0;
        const bool ok = sel_elem(m, s, i, x, w);
        if (ok) atomicOr(&pres[i >> 5], 1u << (i & 31));
        xs[i] = ok ? x : __builtin_inf();
        ws[i] = ok ? w : __builtin_inf();
    }
    __syncthreads();
    auto present = [&](int i) { return ((pres[i >> 5] >> (i & 31)) & 1u) != 0; };
    __shared__ double tot_s;
    if (ph1 && tid == 0) {  // the present total, sequential in row order (read only: the loads pipeline)
        double tot = 0.0;
        for (int i = 0; i < n_rows; i++)
            if (present(i)) tot += ws[i];
        tot_s = tot;
    }
    __syncthreads();
    if (ph1)  // rep_j / tot, each its own division
        for (int i = tid; i < n_rows; i += 1024)
            if (present(i)) ws[i] = ws[i] / tot_s;
    __syncthreads();
    if (tid == 0) {
        int k = 0;
        double W = 0.0;
        for (int i = 0; i < n_rows; i++)
            if (present(i)) {
                W += ws[i];
                k++;
            }
        cnt = k;
        mid_s = 0.5 * W;
        first_s = n_rows;
        wmax_s = 0.0;
    }
    __syncthreads();
    const int n = cnt;
    const double mid = mid_s;
    // dominance: any(w > mid) -> data[first index of max(w)]; any positive weight (exact
    // reductions over the present rows, spread over the block)
    {
        __shared__ double red[1024];
        __shared__ int dom_s, first_p;
        if (tid == 0) {
            dom_s = 0;
            first_p = n_rows;
        }
        double mx = -__builtin_inf();
        bool dom = false, pos = false;
        for (int i = tid; i < n_rows; i += 1024) {
            if (!present(i)) continue;
            mx = fmax(mx, ws[i]);
            dom |= ws[i] > mid;
            pos |= ws[i] > 0.0;
            atomicMin(&first_p, i);
        }
        red[tid] = mx;
        dom = __syncthreads_or(dom);
        pos = __syncthreads_or(pos);
        for (int h = 512; h >= 1; h >>= 1) {
            if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
            __syncthreads();
        }
        // (the sequential max of the SPEC starts at the first present weight: a NaN there stays,
        // and nothing equals it)
        const double mxa = (n > 0 && __builtin_isnan(ws[first_p])) ? __builtin_nan("") : red[0];
        if (dom)
            for (int i = tid; i < n_rows; i += 1024)
                if (present(i) && ws[i] == mxa) atomicMin(&first_s, i);
        if (tid == 0) {
            dom_s = dom ? 1 : 0;
            wmax_s = pos ? 1.0 : 0.0;
        }
        __syncthreads();
        if (tid == 0 && !dom_s) first_s = -1;
        __syncthreads();
    }
    if (first_s >= 0) {
        if (tid == 0) sel_done(st, xs[first_s]);
        return;
    }
    if (wmax_s == 0.0) {  // no positive weight: None
        if (tid == 0) sel_done(st, __builtin_nan(""));
        return;
    }
    // bitonic sort of (x, w) pairs, padded to a power of two with +inf (the absent rows are too)
    int P = 1;
    while (P < n_rows) P <<= 1;
    for (int k = n_rows + tid; k < P; k += 1024) {
        xs[k] = __builtin_inf();
        ws[k] = __builtin_inf();
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += 1024) {
                const int lo = 2 * stride * (t / stride) + (t % stride);
                const int hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const double xa = xs[lo], xb = xs[hi], wa = ws[lo], wb = ws[hi];
                const bool gt = (xa > xb) || (xa == xb && wa > wb);
                if (gt == up) {
                    xs[lo] = xb;
                    xs[hi] = xa;
                    ws[lo] = wb;
                    ws[hi] = wa;
                }
            }
            __syncthreads();
        }
    if (tid == 0) {
        double cum = 0.0;
        int k = 0;
        bool fail = false;
        while (cum <= mid) {
            if (k == n) {
                fail = true;
                break;
            }
            cum += ws[k];
            k++;
        }
        double res;
        if (fail) {
            res = __builtin_nan("");
        } else {
            const double before = cum - ws[k - 1];
            if (fabs(before - mid) < 2.220446049250313080847e-16) {
                if (k >= 2)
                    res = (xs[k - 2] + xs[k - 1]) / 2.0;
                else
                    res = n == 1 ? xs[0] / 1.0 : __builtin_nan("");
            } else {
                res = xs[k - 1];
            }
        }
        sel_done(st, res);
    }
}

}  // namespace

hipError_t select_stage(pcx_mat& m, int stage, hipStream_t st, std::string& err) {
    const int sg = (m.n_scaled + BT - 1) / BT;
    switch (stage) {
        case M_SEL_INIT:  // status, key range and the active list of the first histogram pass
            if (m.n_scaled == 0) break;
            hipLaunchKernelGGL(k_sel_setup, dim3(sg), dim3(BT), 0, st, m);
            if (m.sel_phase == 2 || m.rep_raw) {
                const int64_t wb = (m.n_rows + BT - 1) / BT;
                hipLaunchKernelGGL(k_sel_wlimbs, dim3(wb < 512 ? (wb > 0 ? wb : 1) : 512), dim3(BT), 0, st, m);
            }
            hipLaunchKernelGGL(k_sel_range, dim3(sg), dim3(BT), 0, st, m);
            hipLaunchKernelGGL(k_sel_compact, dim3(1), dim3(1024), 0, st, m);
            hipLaunchKernelGGL(k_sel_sample, dim3(m.n_scaled), dim3(BT), 0, st, m);
            break;
        case M_SEL_EXACT:
            if (m.n_scaled == 0) break;
            if (m.world != 1 || m.n_rows > SEL_EXACT_MAX) {
                err = "M_SEL_EXACT needs one rank and n_rows <= 8192";
                return hipErrorInvalidValue;
            }
            hipLaunchKernelGGL(k_sel_setup, dim3(sg), dim3(BT), 0, st, m);
            hipLaunchKernelGGL(k_sel_exact, dim3(m.n_scaled), dim3(1024), 0, st, m);
            break;
        case M_SEL_START:
            if (m.n_scaled == 0) break;
            info_clear(m, (int)IN_SEL_ARGMAX, st);
            hipLaunchKernelGGL(k_sel_start, dim3((unsigned)((m.n_scaled + BT / WAVE - 1) / (BT / WAVE))), dim3(BT), 0,
                               st, m);
            break;
        case M_SEL_ARGMAX:
            if (m.n_scaled == 0) break;
            hipLaunchKernelGGL(k_sel_argmax, dim3(m.n_scaled), dim3(BT), 0, st, m);
            break;
        case M_SEL_VALUE:
            if (m.n_scaled == 0) break;
            hipLaunchKernelGGL(k_sel_value, dim3(sg), dim3(BT), 0, st, m);
            break;
        case M_SEL_VALUE_FINISH:
            if (m.n_scaled == 0) break;
            hipLaunchKernelGGL(k_sel_value_finish, dim3(sg), dim3(BT), 0, st, m);
            break;
        case M_SEL_COMPACT:
            hipLaunchKernelGGL(k_sel_compact, dim3(1), dim3(1024), 0, st, m);
            break;
        case M_SEL_FINISH:
            if (m.n_scaled == 0) break;
            hipLaunchKernelGGL(k_sel_finish, dim3(sg), dim3(BT), 0, st, m);
            break;
    }
    return hipGetLastError();
}

hipError_t sel_hist(pcx_mat& m, int n_active, hipStream_t st) {
    if (n_active <= 0) return hipSuccess;
    static int ncu = 0;
    if (!ncu) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
            ncu = n;
        if (ncu <= 0) ncu = 256;
    }
    const bool cm = m.sel_phase == 1 && !m.rep_raw && m.n_rows < (1ll << 32);  // (every pass of this phase counts)
    if (n_active <= ncu) {
        if (cm)
            hipLaunchKernelGGL((k_sel_hist<1024, true>), dim3(n_active), dim3(1024), 0, st, m);
        else
            hipLaunchKernelGGL((k_sel_hist<1024, false>), dim3(n_active), dim3(1024), 0, st, m);
    } else if (cm) {  // (49 VGPRs: eight waves per SIMD, so 512 threads an event at four events a CU)
        hipLaunchKernelGGL((k_sel_hist<512, true>), dim3(n_active), dim3(512), 0, st, m);
    } else {
        // (weight mode: 107 VGPRs, four waves per SIMD; with 75 VGPRs and 384 threads an event the
        // weight passes ran 5.1 vs 4.5 ms at C5 -- more waves contend for the LDS atomics)
        hipLaunchKernelGGL((k_sel_hist<BT, false>), dim3(n_active), dim3(BT), 0, st, m);
    }
    return hipGetLastError();
}

hipError_t sel_step(pcx_mat& m, int n_active, hipStream_t st) {
    if (n_active <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sel_step, dim3((n_active + BT / WAVE - 1) / (BT / WAVE)), dim3(BT), 0, st, m, n_active);
    return hipGetLastError();
}

}  // namespace pcx
