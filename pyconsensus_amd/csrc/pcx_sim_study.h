// pcx_sim_study.h -- simulator studies (include/pcx.h "Simulator studies"): the
// detail metrics of a round and the per-cell statistics, one source for the CPU
// (pcx_sim_*detail_host, pcx_sim_sweep_stats_host) and the GPU (pcx_sim_study.hip), and the launchers.
//
// Integer counts, fp64 +, -, *, / and one sqrt, each rounded on its own (the library is built with
// -ffp-contract=off), so both sides agree bit for bit.  A ratio with a zero denominator is NaN.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pcx.h"
#include "pcx_sim.h"
#include "pcx_sim_sweep.h"

namespace pcx {
namespace study {

constexpr int NV = PCX_SIM_NMETRICS + PCX_SIM_NDETAIL;  // values per round: the metrics, then the detail
constexpr int LANES = 256;                              // "threads" of a cell's reduction (k_sim_sweep_summary's)
constexpr int GROUP = 6;                                // values a workgroup reduces together: 12 KB of LDS
constexpr int NGROUPS = NV / GROUP;
static_assert(NGROUPS * GROUP == NV, "the values go in whole groups");

PCX_SIM_HD bool is_nan(double x) { return x != x; }
PCX_SIM_HD double ratio(double a, double b) { return b == 0.0 ? sim::nan_report() : a / b; }

// detail[PCX_SIM_NDETAIL] of one round; every pointer is at the round's first element
PCX_SIM_HD void detail_round(int64_t N, int64_t E, double scaled_tol, const uint8_t* scaled, const double* lo,
                             const double* hi, const double* truth, const uint8_t* liar, const double* old_rep,
                             const double* smooth_rep, const double* outcomes_final, double* d) {
    int64_t n_bin = 0, n_sc = 0, ok_bin = 0, ok_sc = 0, indet = 0, flip = 0, n_nan = 0, n_err = 0;
    double err = 0.0;
    for (int64_t j = 0; j < E; j++) {  // events in increasing j
        const double out = outcomes_final[j], tr = truth[j];
        n_nan += is_nan(out);
        if (scaled[j]) {
            const double w = hi[j] - lo[j];
            const double bound = scaled_tol * w;
            const double dist = fabs(out - tr);
            n_sc++;
            ok_sc += dist <= bound;  // false for a NaN outcome
            if (!is_nan(out)) {
                const double q = dist / w;
                err += q;
                n_err++;
            }
        } else {
            const double lie = 3.0 - tr;
            n_bin++;
            ok_bin += out == tr;
            indet += out == 1.5;
            flip += out == lie;
        }
    }
    int64_t tp = 0, fn = 0, fp = 0, tn = 0;
    double colluders = 0.0;
    for (int64_t i = 0; i < N; i++) {  // reporters in increasing i
        const bool punished = smooth_rep[i] < old_rep[i];  // false when either is NaN
        if (liar[i] & sim::LIAR) {
            tp += punished;
            fn += !punished;
            if (liar[i] & sim::COLLUDES) colluders += smooth_rep[i];
        } else {
            fp += punished;
            tn += !punished;
        }
    }
    d[0] = ratio((double)ok_bin, (double)n_bin);
    d[1] = ratio((double)ok_sc, (double)n_sc);
    d[2] = ratio((double)indet, (double)n_bin);
    d[3] = ratio((double)flip, (double)n_bin);
    d[4] = ratio((double)n_nan, (double)E);
    d[5] = ratio(err, (double)n_err);
    const double TP = (double)tp, FN = (double)fn, FP = (double)fp, TN = (double)tn;
    d[6] = TP;
    d[7] = FN;
    d[8] = FP;
    d[9] = TN;
    // with N <= 1024 every product is an exact integer (a, b, p, q <= 2^20, pq <= 2^40 < 2^53): the
    // sqrt and the division round
    const double a = TP * TN, b = FP * FN;
    const double p = (TP + FP) * (TP + FN), q = (TN + FP) * (TN + FN);
    const double pq = p * q;
    d[10] = ratio(a - b, sqrt(pq));
    d[11] = colluders;
}

// ---------------------------------------------------------------- per-cell statistics
// Value v of the cell's round b at timestep t: p[b * stride].
struct Column {
    const double* p;
    int64_t stride;
};

// B = the sweep's rounds, round0 = the cell's first
PCX_SIM_HD Column column(const double* metrics, const double* detail, int64_t t, int64_t B, int64_t round0, int v) {
    if (v < PCX_SIM_NMETRICS) return Column{metrics + (t * B + round0) * PCX_SIM_NMETRICS + v, PCX_SIM_NMETRICS};
    return Column{detail + (t * B + round0) * PCX_SIM_NDETAIL + (v - PCX_SIM_NMETRICS), PCX_SIM_NDETAIL};
}

// the value a statistic runs over: the column's, or with a base column the paired difference; false = skipped
PCX_SIM_HD bool value(const Column& c, const Column* base, int64_t b, double* x) {
    const double v = c.p[b * c.stride];
    if (is_nan(v)) return false;
    if (!base) {
        *x = v;
        return true;
    }
    const double w = base->p[b * base->stride];
    if (is_nan(w)) return false;
    *x = v - w;
    return true;
}

struct Partial {
    double n, sum, mn, mx;  // (n: a count, exact as a double)
};

PCX_SIM_HD double op_sum(double a, double b) { return a + b; }
PCX_SIM_HD double op_min(double a, double b) { return b < a ? b : a; }
PCX_SIM_HD double op_max(double a, double b) { return b > a ? b : a; }

// first pass of lane `tid`: the rounds tid, tid + LANES, ... from 0.0
PCX_SIM_HD Partial lane_first(const Column& c, const Column* base, int64_t R, int tid) {
    Partial a{0.0, 0.0, HUGE_VAL, -HUGE_VAL};
    for (int64_t b = tid; b < R; b += LANES) {
        double x;
        if (!value(c, base, b, &x)) continue;
        a.n += 1.0;
        a.sum += x;
        a.mn = op_min(a.mn, x);
        a.mx = op_max(a.mx, x);
    }
    return a;
}

// second pass: the squares of the distances from the mean, multiply, then add
PCX_SIM_HD double lane_second(const Column& c, const Column* base, int64_t R, int tid, double mean) {
    double acc = 0.0;
    for (int64_t b = tid; b < R; b += LANES) {
        double x;
        if (!value(c, base, b, &x)) continue;
        const double d = x - mean;
        const double dd = d * d;
        acc += dd;
    }
    return acc;
}

PCX_SIM_HD double mean_of(double n, double sum) { return n == 0.0 ? sim::nan_report() : sum / n; }
PCX_SIM_HD double var_of(double n, double squares) { return n < 2.0 ? sim::nan_report() : squares / (n - 1.0); }
PCX_SIM_HD double extreme_of(double n, double x) { return n == 0.0 ? sim::nan_report() : x; }

}  // namespace study

// detail [B][PCX_SIM_NDETAIL] of scored rounds.  s.cells NULL: s.B equal-shape rounds of N x E
// (pcx_sim_detail_f64); otherwise the sweep's flat layout and N, E are not read.
hipError_t launch_sim_study_detail(const SweepTables& s, int32_t N, int32_t E, double scaled_tol,
                                   const pcx_sim_rounds& r, const double* old_rep, const double* smooth_rep,
                                   const double* outcomes_final, double* detail, hipStream_t st);
// the same on the host: `cells` is a HOST table (or NULL: B equal-shape rounds)
void sim_study_detail_host(const SweepCell* cells, int64_t C, int64_t B, int32_t N, int32_t E, double scaled_tol,
                           const pcx_sim_rounds& r, const double* old_rep, const double* smooth_rep,
                           const double* outcomes_final, double* detail);
// stats [T][C][NV][5] and, with pair_base (DEVICE int32 [C]) and paired, paired [T][C][NV][3]: one launch
hipError_t launch_sim_study_stats(const SweepTables& s, int64_t T, const double* metrics, const double* detail,
                                  const int32_t* pair_base, double* stats, double* paired, hipStream_t st);
// the same on the host: HOST tables and arrays, the lanes and the tree replayed in a loop
void sim_study_stats_host(const SweepCell* cells, int64_t C, int64_t B, int64_t T, const double* metrics,
                          const double* detail, const int32_t* pair_base, double* stats, double* paired);

}  // namespace pcx
