// pcx_mat_device.h -- what the translation units of the single-matrix path (pcx_matrix.hip,
// pcx_mat_select.hip, pcx_mat_hard.hip) share: the host entry points they call across and the device
// helpers that more than one of them uses.  The helpers sit in each unit's anonymous namespace; no
// kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pcx.h"
#include "pcx_device.h"
#include "pcx_fastdiv.h"
#include "pcx_internal.h"
#include "pcx_mat_layout.h"

namespace pcx {

// (between libpcx's own translation units only: not part of the library's dynamic symbols)
#pragma GCC visibility push(hidden)
// the M_SEL_* stages of mat_stage (pcx_mat_select.hip)
hipError_t select_stage(pcx_mat& m, int stage, hipStream_t st, std::string& err);
// info[slot] = 0 (k_info_clear, pcx_matrix.hip)
void info_clear(const pcx_mat& m, int slot, hipStream_t st);
#pragma GCC visibility pop

namespace {

// ------------------------------------------------------------------ element transform
struct ColParam {
    bool scaled;
    double lo, range, guess, mu;
    double rr;  // RN(1 / range); NaN when range lies outside [2^-100, 2^100] (quotients then divide)
};

// (div_rn and range_rcp, the rescale's division through the range's reciprocal: pcx_fastdiv.h)
__device__ __forceinline__ double rescale(double r, const ColParam& p, int int_dtype) {
    if (!p.scaled) return r;
    double x = div_rn(r - p.lo, p.range, p.rr);
    if (int_dtype) x = trunc(x);
    return x;
}

__device__ __forceinline__ bool missing(double x) { return __builtin_isnan(x) || x == 0.0; }

__device__ __forceinline__ ColParam col_param(const pcx_mat& m, int c, bool with_fill) {
    ColParam p;
    p.scaled = m.scaled && m.scaled[c] && !m.rescaled;  // (in place already: the identity)
    p.lo = p.scaled ? m.lo[c] : 0.0;
    p.range = p.scaled ? (m.hi[c] - m.lo[c]) : 1.0;
    p.guess = with_fill ? m.ev[EV_GUESS * m.n_events + c] : 0.0;
    p.mu = with_fill ? m.ev[EV_MU * m.n_events + c] : 0.0;
    p.rr = p.scaled ? range_rcp(p.range) : 1.0;
    return p;
}

// filled value F_ic (:310-312)
__device__ __forceinline__ double filled(double r, const ColParam& p, int int_dtype) {
    const double x = rescale(r, p, int_dtype);
    return missing(x) ? p.guess : x;
}

// ------------------------------------------------------------------ limbs (exact sums)
struct L3 {
    uint64_t a, b, c;  // value = a*2^-35 + b*2^-78 + c*2^-121
};

__device__ __forceinline__ L3 l3_norm(L3 x) {  // carry so that b, c < 2^43
    const uint64_t M = (1ull << 43) - 1;
    x.b += x.c >> 43;
    x.c &= M;
    x.a += x.b >> 43;
    x.b &= M;
    return x;
}
__device__ __forceinline__ L3 l3_add(L3 x, L3 y) { return l3_norm({x.a + y.a, x.b + y.b, x.c + y.c}); }
__device__ __forceinline__ L3 l3_twice(L3 x) { return l3_norm({x.a * 2, x.b * 2, x.c * 2}); }
__device__ __forceinline__ int l3_cmp(L3 x, L3 y) {  // both normalised
    if (x.a != y.a) return x.a < y.a ? -1 : 1;
    if (x.b != y.b) return x.b < y.b ? -1 : 1;
    if (x.c != y.c) return x.c < y.c ? -1 : 1;
    return 0;
}
__device__ __forceinline__ L3 l3_of(double w) {
    const limbs3 t = to_limbs(w);
    return {t.l0, t.l1, t.l2};
}
__device__ __forceinline__ double l3_to_double(L3 x) {
    return ldexp((double)x.a, -35) + (ldexp((double)x.b, -78) + ldexp((double)x.c, -121));
}

__device__ __forceinline__ L3 ld_l3(const uint64_t* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void st_l3(uint64_t* p, L3 v) {
    p[0] = v.a;
    p[1] = v.b;
    p[2] = v.c;
}

// the row loop of the column passes (rows_unrolled, pcx_matrix.hip) over a strided row set i = first,
// first + stride, ... < n: U loads issued before any is consumed
template <int U, class LOAD, class PROC>
__device__ __forceinline__ void rows_strided(int64_t first, int64_t stride, int64_t n, LOAD load, PROC proc) {
    int64_t i = first;
    for (; i + (U - 1) * stride < n; i += U * stride) {
        decltype(load(i)) v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = load(i + u * stride);
#pragma unroll
        for (int u = 0; u < U; u++) proc(i + u * stride, v[u]);
    }
    for (; i < n; i += stride) proc(i, load(i));
}

struct XW {
    double x, w;
};

__device__ __forceinline__ void sel_done(uint64_t* st, double r) {
    st[SW_RESULT] = __double_as_longlong(r);
    st[SW_STATUS] = 0;
}

// ordered compaction of [0, n) by pred into out[] (block-wide, order preserving); returns count
template <class PRED, class EMIT>
__device__ int64_t block_compact(int64_t n, PRED pred, EMIT emit) {
    __shared__ int wsum[16];
    __shared__ int64_t base_s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < n; c0 += blockDim.x) {
        const int64_t i = c0 + tid;
        const bool p = i < n && pred(i);
        const uint64_t bal = __ballot(p);
        const int before_lane = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(bal);
        __syncthreads();
        int off = 0;
        for (int k = 0; k < wv; k++) off += wsum[k];
        const int64_t base = base_s;
        if (p) emit(i, base + off + before_lane);
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int k = 0; k < nw; k++) t += wsum[k];
            base_s = base + t;
        }
        __syncthreads();
    }
    return base_s;
}

}  // namespace
}  // namespace pcx
