// pcx_sim_study.hip -- kernels of the simulator's studies (include/pcx.h "Simulator studies",
// DESIGN.md 5.4.2), a translation unit of its own: the sweep's kernels keep their code objects.
//
//   k_sim_study_detail  one lane per round, pcx_sim_study.h's detail_round with the round's own
//                       offsets (the sums are sequential by definition).  The flat layout finds the
//                       round's cell by k_sim_sweep_metrics' prefix search; without a cell table the
//                       rounds have one shape.
//   k_sim_study_stats   one 256-thread workgroup per (cell, timestep, group of six values):
//                       k_sim_sweep_summary's order -- lane tau takes the rounds tau, tau + 256, ...,
//                       then the LDS tree with strides 128 .. 1 -- for the count, the sum, the
//                       extremes and, in a second pass, the squares; then the same for the paired
//                       differences against the cell's base.  No atomics: the bytes do not depend on
//                       the launch geometry.  One launch covers every timestep.
#include <hip/hip_runtime.h>

#include "pcx_internal.h"
#include "pcx_sim_study.h"

namespace pcx {

namespace {
constexpr int ST_TB = study::LANES;

__global__ __launch_bounds__(ST_TB) void k_sim_study_detail(const SweepTables s, const int32_t N0, const int32_t E0,
                                                            const double scaled_tol, const pcx_sim_rounds r,
                                                            const double* __restrict__ old_rep,
                                                            const double* __restrict__ smooth_rep,
                                                            const double* __restrict__ outcomes_final,
                                                            double* __restrict__ detail) {
    const int64_t b = (int64_t)blockIdx.x * ST_TB + threadIdx.x;
    if (b >= s.B) return;
    int64_t N = N0, E = E0, row = b * N0, ev = b * E0;
    if (s.cells) {
        const SweepCell* cp = s.cells + sweep_cell_of(s.prefix, s.C, b);
        const int64_t rb = b - cp->round0;
        N = cp->N;
        E = cp->E;
        row = cp->row0 + rb * N;
        ev = cp->ev0 + rb * E;
    }
    double d[PCX_SIM_NDETAIL];
    study::detail_round(N, E, scaled_tol, r.scaled + ev, r.lo + ev, r.hi + ev, r.truth + ev, r.liar + row,
                        old_rep + row, smooth_rep + row, outcomes_final + ev, d);
    double* out = detail + b * PCX_SIM_NDETAIL;
    for (int k = 0; k < PCX_SIM_NDETAIL; k++) out[k] = d[k];
}

// v[k] of every lane reduced by the tree into out[k] (in every lane); sh is free again on return
template <double (*OP)(double, double)>
__device__ __forceinline__ void tree(double (*sh)[ST_TB], int tid, const double v[study::GROUP],
                                     double out[study::GROUP]) {
    for (int k = 0; k < study::GROUP; k++) sh[k][tid] = v[k];
    __syncthreads();
    for (int stride = ST_TB / 2; stride >= 1; stride >>= 1) {
        if (tid < stride)
            for (int k = 0; k < study::GROUP; k++) sh[k][tid] = OP(sh[k][tid], sh[k][tid + stride]);
        __syncthreads();
    }
    for (int k = 0; k < study::GROUP; k++) out[k] = sh[k][0];
    __syncthreads();
}

// {n, mean, var} and, where wanted, {min, max} of the group's values (base NULL) or paired differences
__device__ __forceinline__ void reduce_group(double (*sh)[ST_TB], int tid, const study::Column col[study::GROUP],
                                             const study::Column* base, int64_t R, double n[study::GROUP],
                                             double mean[study::GROUP], double var[study::GROUP],
                                             double mn[study::GROUP], double mx[study::GROUP]) {
    double a[study::GROUP], b[study::GROUP], c[study::GROUP], d[study::GROUP];
    for (int k = 0; k < study::GROUP; k++) {
        const study::Partial p = study::lane_first(col[k], base ? base + k : nullptr, R, tid);
        a[k] = p.n;
        b[k] = p.sum;
        c[k] = p.mn;
        d[k] = p.mx;
    }
    double sum[study::GROUP];
    tree<study::op_sum>(sh, tid, a, n);
    tree<study::op_sum>(sh, tid, b, sum);
    if (mn) {
        tree<study::op_min>(sh, tid, c, mn);
        tree<study::op_max>(sh, tid, d, mx);
    }
    for (int k = 0; k < study::GROUP; k++) {
        mean[k] = study::mean_of(n[k], sum[k]);
        a[k] = study::lane_second(col[k], base ? base + k : nullptr, R, tid, mean[k]);
    }
    tree<study::op_sum>(sh, tid, a, b);
    for (int k = 0; k < study::GROUP; k++) {
        var[k] = study::var_of(n[k], b[k]);
        if (mn) {
            mn[k] = study::extreme_of(n[k], mn[k]);
            mx[k] = study::extreme_of(n[k], mx[k]);
        }
    }
}

__global__ __launch_bounds__(ST_TB) void k_sim_study_stats(const SweepTables s, const double* __restrict__ metrics,
                                                           const double* __restrict__ detail,
                                                           const int32_t* __restrict__ pair_base,
                                                           double* __restrict__ stats, double* __restrict__ paired) {
    __shared__ double sh[study::GROUP][ST_TB];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x, t = blockIdx.y;
    const int v0 = (int)blockIdx.z * study::GROUP;
    const int64_t R = s.cells[c].R;
    study::Column col[study::GROUP];
    for (int k = 0; k < study::GROUP; k++) col[k] = study::column(metrics, detail, t, s.B, s.cells[c].round0, v0 + k);
    double n[study::GROUP], mean[study::GROUP], var[study::GROUP], mn[study::GROUP], mx[study::GROUP];
    reduce_group(sh, tid, col, nullptr, R, n, mean, var, mn, mx);
    const int64_t at = (t * s.C + c) * study::NV + v0;
    if (tid == 0)
        for (int k = 0; k < study::GROUP; k++) {
            double* o = stats + (at + k) * 5;
            o[0] = n[k];
            o[1] = mean[k];
            o[2] = var[k];
            o[3] = mn[k];
            o[4] = mx[k];
        }
    if (!paired) return;
    const int64_t base_cell = pair_base[c];  // (checked on the host: -1, or a cell of the same R)
    if (base_cell < 0) {
        for (int k = 0; k < study::GROUP; k++) {
            n[k] = 0.0;
            mean[k] = var[k] = sim::nan_report();
        }
    } else {
        study::Column base[study::GROUP];
        for (int k = 0; k < study::GROUP; k++)
            base[k] = study::column(metrics, detail, t, s.B, s.cells[base_cell].round0, v0 + k);
        reduce_group(sh, tid, col, base, R, n, mean, var, nullptr, nullptr);
    }
    if (tid == 0)
        for (int k = 0; k < study::GROUP; k++) {
            double* o = paired + (at + k) * 3;
            o[0] = n[k];
            o[1] = mean[k];
            o[2] = var[k];
        }
}
}  // namespace

hipError_t launch_sim_study_detail(const SweepTables& s, int32_t N, int32_t E, double scaled_tol,
                                   const pcx_sim_rounds& r, const double* old_rep, const double* smooth_rep,
                                   const double* outcomes_final, double* detail, hipStream_t st) {
    if (s.B <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((s.B + ST_TB - 1) / ST_TB);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_sim_study_detail, dim3(grid), dim3(ST_TB), 0, st, s, N, E, scaled_tol, r, old_rep, smooth_rep,
                       outcomes_final, detail);
    return hipGetLastError();
}

void sim_study_detail_host(const SweepCell* cells, int64_t C, int64_t B, int32_t N, int32_t E, double scaled_tol,
                           const pcx_sim_rounds& r, const double* old_rep, const double* smooth_rep,
                           const double* outcomes_final, double* detail) {
    if (!cells) {
        for (int64_t b = 0; b < B; b++) {
            const int64_t row = b * N, ev = b * E;
            study::detail_round(N, E, scaled_tol, r.scaled + ev, r.lo + ev, r.hi + ev, r.truth + ev, r.liar + row,
                                old_rep + row, smooth_rep + row, outcomes_final + ev, detail + b * PCX_SIM_NDETAIL);
        }
        return;
    }
    for (int64_t c = 0; c < C; c++) {
        const SweepCell& k = cells[c];
        for (int64_t rb = 0; rb < k.R; rb++) {
            const int64_t row = k.row0 + rb * k.N, ev = k.ev0 + rb * k.E;
            study::detail_round(k.N, k.E, scaled_tol, r.scaled + ev, r.lo + ev, r.hi + ev, r.truth + ev, r.liar + row,
                                old_rep + row, smooth_rep + row, outcomes_final + ev,
                                detail + (k.round0 + rb) * PCX_SIM_NDETAIL);
        }
    }
}

hipError_t launch_sim_study_stats(const SweepTables& s, int64_t T, const double* metrics, const double* detail,
                                  const int32_t* pair_base, double* stats, double* paired, hipStream_t st) {
    if (s.C <= 0 || T <= 0) return hipSuccess;
    (void)hipGetLastError();
    // (grid y is a timestep: at most 65535 a launch)
    for (int64_t t0 = 0; t0 < T; t0 += 65535) {
        const int64_t nt = T - t0 < 65535 ? T - t0 : 65535;
        const int64_t at = t0 * s.B, out = t0 * s.C * study::NV;
        hipLaunchKernelGGL(k_sim_study_stats, dim3((unsigned)s.C, (unsigned)nt, study::NGROUPS), dim3(ST_TB), 0, st, s,
                           metrics + at * PCX_SIM_NMETRICS, detail + at * PCX_SIM_NDETAIL, pair_base, stats + out * 5,
                           paired ? paired + out * 3 : nullptr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace {
// the tree of k_sim_study_stats over the lanes' values, replayed
template <double (*OP)(double, double)>
double host_tree(double* lane) {
    for (int stride = study::LANES / 2; stride >= 1; stride >>= 1)
        for (int tid = 0; tid < stride; tid++) lane[tid] = OP(lane[tid], lane[tid + stride]);
    return lane[0];
}

void host_reduce(const study::Column& col, const study::Column* base, int64_t R, double* n, double* mean, double* var,
                 double* mn, double* mx) {
    double a[study::LANES], b[study::LANES], c[study::LANES], d[study::LANES];
    for (int tid = 0; tid < study::LANES; tid++) {
        const study::Partial p = study::lane_first(col, base, R, tid);
        a[tid] = p.n;
        b[tid] = p.sum;
        c[tid] = p.mn;
        d[tid] = p.mx;
    }
    *n = host_tree<study::op_sum>(a);
    *mean = study::mean_of(*n, host_tree<study::op_sum>(b));
    if (mn) {
        *mn = study::extreme_of(*n, host_tree<study::op_min>(c));
        *mx = study::extreme_of(*n, host_tree<study::op_max>(d));
    }
    for (int tid = 0; tid < study::LANES; tid++) a[tid] = study::lane_second(col, base, R, tid, *mean);
    *var = study::var_of(*n, host_tree<study::op_sum>(a));
}
}  // namespace

void sim_study_stats_host(const SweepCell* cells, int64_t C, int64_t B, int64_t T, const double* metrics,
                          const double* detail, const int32_t* pair_base, double* stats, double* paired) {
    for (int64_t t = 0; t < T; t++)
        for (int64_t c = 0; c < C; c++)
            for (int v = 0; v < study::NV; v++) {
                const study::Column col = study::column(metrics, detail, t, B, cells[c].round0, v);
                double* o = stats + ((t * C + c) * study::NV + v) * 5;
                host_reduce(col, nullptr, cells[c].R, o + 0, o + 1, o + 2, o + 3, o + 4);
                if (!paired) continue;
                double* q = paired + ((t * C + c) * study::NV + v) * 3;
                if (pair_base[c] < 0) {
                    q[0] = 0.0;
                    q[1] = q[2] = sim::nan_report();
                    continue;
                }
                const study::Column base = study::column(metrics, detail, t, B, cells[pair_base[c]].round0, v);
                host_reduce(col, &base, cells[c].R, q + 0, q + 1, q + 2, nullptr, nullptr);
            }
}

}  // namespace pcx
