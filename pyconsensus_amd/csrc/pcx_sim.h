// pcx_sim.h -- the Monte Carlo simulator's round generator ("Simulator"), one
// source for the CPU (pcx_sim_generate_host) and the GPU (k_sim_generate, pcx_sim.hip).
//
// Counter-based: every draw is Philox4x32-10 of (event j, reporter i, round b, stream << 24 |
// timestep t) under the key (seed low, seed high), so a cell's value depends on nothing but its
// own indices -- no launch geometry, no draw order.  Integer and fp64 +, -, * only (each rounded
// on its own: the library is built with -ffp-contract=off), so both sides agree bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCX_SIM_HD __host__ __device__ inline
#else
#define PCX_SIM_HD inline
#endif

namespace pcx {
namespace sim {

enum stream { EVENT_A = 0, EVENT_B = 1, EVENT_C = 2, REPORTER = 3, CELL = 4, KMEANS = 5 };
enum liar_bit { LIAR = 1, COLLUDES = 2 };  // the liar[B][N] flags

// What the generator needs of a pcx_sim: the key and the decision thresholds
// thr = floor(p * 2^32), a decision being (uint64)w < thr (p = 1: always, p = 0: never).
struct Gen {
    uint32_t key0, key1;
    uint64_t thr_liar, thr_collude, thr_distort, thr_na, thr_scaled;
};

struct U4 {
    uint32_t w0, w1, w2, w3;
};

PCX_SIM_HD U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

// counter = (j, i, b, stream << 24 | t); an index a stream does not use is 0
PCX_SIM_HD U4 draw(const Gen& g, uint32_t j, uint32_t i, uint32_t b, uint32_t stream, uint32_t t) {
    return philox4x32_10(j, i, b, stream << 24 | t, g.key0, g.key1);
}

PCX_SIM_HD bool decide(uint32_t w, uint64_t thr) { return (uint64_t)w < thr; }

// 53-bit uniform in [0, 1): 27 bits of a, 26 of b (every step exact)
PCX_SIM_HD double u53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// position inside an event's range, never 0: a rescaled report is never the reference's NA 0.0
PCX_SIM_HD double frac(double u) {
    const double m = 0.999 * u;
    return 0.001 + m;
}

PCX_SIM_HD double in_range(double lo, double hi, double f) {
    const double w = hi - lo;
    const double m = w * f;
    return lo + m;
}

struct Event {
    double lo, hi, truth, lie;
    uint8_t scaled;
};

PCX_SIM_HD Event event(const Gen& g, uint32_t b, uint32_t j, uint32_t t) {
    Event e;
    const U4 a = draw(g, j, 0, b, EVENT_A, t);
    e.scaled = decide(a.w0, g.thr_scaled) ? 1 : 0;
    if (!e.scaled) {
        e.lo = 1.0;
        e.hi = 2.0;
        e.truth = 1.0 + (double)(a.w1 >> 31);
        e.lie = 3.0 - e.truth;
        return e;
    }
    const U4 q = draw(g, j, 0, b, EVENT_B, t);
    const U4 c = draw(g, j, 0, b, EVENT_C, t);
    const double m = 100.0 * u53(a.w2, a.w3);
    e.lo = -100.0 + m;
    const double wm = 199.0 * u53(q.w0, q.w1);
    const double w = 1.0 + wm;
    e.hi = e.lo + w;
    e.truth = in_range(e.lo, e.hi, frac(u53(q.w2, q.w3)));
    e.lie = in_range(e.lo, e.hi, frac(u53(c.w0, c.w1)));
    return e;
}

// bit 0: liar; bit 1: a liar that colludes (reports the event's shared lie).  The same person
// through a whole trajectory: no timestep in the counter.
PCX_SIM_HD uint8_t reporter(const Gen& g, uint32_t b, uint32_t i) {
    const U4 r = draw(g, 0, i, b, REPORTER, 0);
    if (!decide(r.w0, g.thr_liar)) return 0;
    return decide(r.w1, g.thr_collude) ? (LIAR | COLLUDES) : LIAR;
}

PCX_SIM_HD double nan_report() {
    union {
        uint64_t u;
        double d;
    } v;
    v.u = 0x7ff8000000000000ull;
    return v.d;
}

// One Philox call per cell.
PCX_SIM_HD double cell(const Gen& g, const Event& e, uint8_t who, uint32_t b, uint32_t i, uint32_t j, uint32_t t) {
    const U4 c = draw(g, j, i, b, CELL, t);
    if (decide(c.w0, g.thr_na)) return nan_report();
    const double u = u53(c.w2, c.w3);
    const double rv = e.scaled ? in_range(e.lo, e.hi, frac(u)) : (u < 0.5 ? 1.0 : 2.0);
    if (who & LIAR) return (who & COLLUDES) ? e.lie : rv;
    return decide(c.w1, g.thr_distort) ? rv : e.truth;
}

// The initial code book of k-means restart r of round b at timestep t: k distinct
// rows of [0, N) by Floyd's sampling, one draw of the KMEANS stream per code -- for c = 0 .. k - 1,
// j = N - k + c, v = (w * (j + 1)) >> 32 a row of [0, j], and the code is v unless an earlier code
// is v already, then j (which no earlier code can be).  Every k-subset is equally likely up to the
// multiply-shift's bias of at most (j + 1) / 2^32.  Integers only.  1 <= k <= N.
PCX_SIM_HD void kmeans_book(const Gen& g, uint32_t b, uint32_t r, uint32_t t, int N, int k, int32_t* book) {
    for (int c = 0; c < k; c++) {
        const uint32_t j = (uint32_t)(N - k + c);
        const uint32_t w = draw(g, (uint32_t)c, r, b, KMEANS, t).w0;
        const int32_t v = (int32_t)(((uint64_t)w * (j + 1)) >> 32);
        bool seen = false;
        for (int q = 0; q < c; q++) seen |= book[q] == v;
        book[c] = seen ? (int32_t)j : v;
    }
}

}  // namespace sim
}  // namespace pcx
