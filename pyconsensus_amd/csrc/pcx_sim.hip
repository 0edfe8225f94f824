// pcx_sim.hip -- kernels of the Monte Carlo simulator (include/pcx.h "Monte Carlo simulator",
// DESIGN.md "Simulator"): the round generator, the per-round metrics and their summary.
//
//   k_sim_generate  streaming writer of one timestep's rounds.  A work item is (round b, chunk of
//                   up to SIM_ROWS reporters); a 256-thread workgroup takes work items grid-stride.
//                   It stages the chunk's reporter flags and, per tile of up to SIM_EVENTS events,
//                   the events' parameters in LDS, then walks the chunk's cells in memory order
//                   (along E within a row, then across rows), one 8-byte store per lane and 512
//                   contiguous bytes per wave store.  With E <= SIM_EVENTS and N <= SIM_ROWS a
//                   round is one work item and one contiguous run of N * E doubles.
//   k_sim_metrics   one lane per round (sequential sums over the liars in reporter order).
//   k_sim_summary   one 256-thread workgroup: thread tau adds rounds tau, tau + 256, ... from 0.0,
//                   an LDS tree (strides 128 .. 1) follows, then / B.  No atomics, so the means do
//                   not depend on any launch geometry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pcx_internal.h"

namespace pcx {

namespace {
constexpr int SIM_TB = 256;      // threads per workgroup
constexpr int SIM_ROWS = 1024;   // reporters per work item (their flags in LDS)
constexpr int SIM_EVENTS = 256;  // events per LDS tile (<= SIM_TB: one thread draws one event)
constexpr int SIM_GRID = 8192;   // workgroups at most; the work items beyond are taken grid-stride

__global__ __launch_bounds__(SIM_TB) void k_sim_generate(const sim::Gen g, const int64_t N, const int64_t E,
                                                         const uint32_t t, const pcx_sim_rounds out,
                                                         const int64_t row_chunks, const int64_t items) {
    __shared__ double s_lo[SIM_EVENTS], s_hi[SIM_EVENTS], s_truth[SIM_EVENTS], s_lie[SIM_EVENTS];
    __shared__ uint8_t s_scaled[SIM_EVENTS], s_who[SIM_ROWS];
    const int tid = threadIdx.x;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t b = item / row_chunks;
        const int64_t i0 = (item % row_chunks) * SIM_ROWS;
        const int rows = (int)std::min<int64_t>(SIM_ROWS, N - i0);
        // reporters from the last thread down: at the headline shape (50 x 20) another wave than
        // the one that draws the events (up to three Philox calls each) takes them
        for (int r = SIM_TB - 1 - tid; r < rows; r += SIM_TB) {
            const uint8_t who = sim::reporter(g, (uint32_t)b, (uint32_t)(i0 + r));
            s_who[r] = who;
            if (out.liar) out.liar[b * N + i0 + r] = who;
        }
        for (int64_t j0 = 0; j0 < E; j0 += SIM_EVENTS) {
            const int ew = (int)std::min<int64_t>(SIM_EVENTS, E - j0);
            if (tid < ew) {
                const sim::Event e = sim::event(g, (uint32_t)b, (uint32_t)(j0 + tid), t);
                s_lo[tid] = e.lo;
                s_hi[tid] = e.hi;
                s_truth[tid] = e.truth;
                s_lie[tid] = e.lie;
                s_scaled[tid] = e.scaled;
                if (i0 == 0) {  // the round's first chunk writes the event vectors
                    const int64_t o = b * E + j0 + tid;
                    if (out.scaled) out.scaled[o] = e.scaled;
                    if (out.lo) out.lo[o] = e.lo;
                    if (out.hi) out.hi[o] = e.hi;
                    if (out.truth) out.truth[o] = e.truth;
                }
            }
            __syncthreads();
            if (out.reports) {
                // cell c of the rows x ew block is (c / ew, c % ew); c steps by SIM_TB, so (i, j)
                // step by (SIM_TB / ew, SIM_TB % ew) with a carry: no division per cell
                const int cells = rows * ew;
                const int di = SIM_TB / ew, dj = SIM_TB % ew;
                int i = tid / ew, j = tid % ew;
                double* base = out.reports + (b * N + i0) * E + j0;
                for (int c = tid; c < cells; c += SIM_TB) {
                    sim::Event e;
                    e.lo = s_lo[j];
                    e.hi = s_hi[j];
                    e.truth = s_truth[j];
                    e.lie = s_lie[j];
                    e.scaled = s_scaled[j];
                    base[(int64_t)i * E + j] =
                        sim::cell(g, e, s_who[i], (uint32_t)b, (uint32_t)(i0 + i), (uint32_t)(j0 + j), t);
                    i += di;
                    j += dj;
                    if (j >= ew) {
                        j -= ew;
                        i++;
                    }
                }
            }
            __syncthreads();  // the next tile / work item overwrites the LDS
        }
    }
}

__global__ __launch_bounds__(SIM_TB) void k_sim_metrics(const int64_t B, const int64_t N, const int64_t E,
                                                        const double scaled_tol, const pcx_sim_rounds r,
                                                        const double* __restrict__ old_rep,
                                                        const double* __restrict__ smooth_rep,
                                                        const double* __restrict__ outcomes_final,
                                                        double* __restrict__ metrics) {
    const int64_t b = (int64_t)blockIdx.x * SIM_TB + threadIdx.x;
    if (b >= B) return;
    int64_t ok = 0;
    for (int64_t j = 0; j < E; j++) {
        const int64_t o = b * E + j;
        const double out = outcomes_final[o], truth = r.truth[o];
        if (r.scaled[o]) {
            const double w = r.hi[o] - r.lo[o];
            const double bound = scaled_tol * w;
            ok += fabs(out - truth) <= bound;  // false for a NaN outcome
        } else {
            ok += out == truth;
        }
    }
    double before = 0.0, after = 0.0;
    int64_t n = 0;
    for (int64_t i = 0; i < N; i++) {  // sequential, in reporter order
        const int64_t o = b * N + i;
        if (r.liar[o] & sim::LIAR) {
            before += old_rep[o];
            after += smooth_rep[o];
            n++;
        }
    }
    double* m = metrics + b * PCX_SIM_NMETRICS;
    m[0] = (double)ok / (double)E;
    m[1] = before;
    m[2] = after;
    m[3] = after - before;
    m[4] = after > before ? 1.0 : 0.0;
    m[5] = (double)n;
}

__global__ __launch_bounds__(SIM_TB) void k_sim_summary(const double* __restrict__ metrics, const int64_t B,
                                                        double* __restrict__ summary) {
    __shared__ double s[PCX_SIM_NMETRICS][SIM_TB];
    const int tid = threadIdx.x;
    double acc[PCX_SIM_NMETRICS];
    for (int k = 0; k < PCX_SIM_NMETRICS; k++) acc[k] = 0.0;
    for (int64_t b = tid; b < B; b += SIM_TB)
        for (int k = 0; k < PCX_SIM_NMETRICS; k++) acc[k] += metrics[b * PCX_SIM_NMETRICS + k];
    for (int k = 0; k < PCX_SIM_NMETRICS; k++) s[k][tid] = acc[k];
    __syncthreads();
    for (int stride = SIM_TB / 2; stride >= 1; stride >>= 1) {
        if (tid < stride)
            for (int k = 0; k < PCX_SIM_NMETRICS; k++) s[k][tid] += s[k][tid + stride];
        __syncthreads();
    }
    if (tid < PCX_SIM_NMETRICS) summary[tid] = s[tid][0] / (double)B;
}
}  // namespace

hipError_t launch_sim_generate(const sim::Gen& g, int64_t B, int64_t N, int64_t E, uint32_t t,
                               const pcx_sim_rounds& out, hipStream_t st) {
    const int64_t row_chunks = (N + SIM_ROWS - 1) / SIM_ROWS;
    const int64_t items = B * row_chunks;
    if (items <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<int64_t>(items, SIM_GRID);
    hipLaunchKernelGGL(k_sim_generate, dim3(grid), dim3(SIM_TB), 0, st, g, N, E, t, out, row_chunks, items);
    return hipGetLastError();
}

void sim_generate_host(const sim::Gen& g, int64_t B, int64_t N, int64_t E, uint32_t t, const pcx_sim_rounds& out) {
    std::vector<uint8_t> who((size_t)N);
    for (int64_t b = 0; b < B; b++) {
        for (int64_t i = 0; i < N; i++) {
            who[i] = sim::reporter(g, (uint32_t)b, (uint32_t)i);
            if (out.liar) out.liar[b * N + i] = who[i];
        }
        for (int64_t j = 0; j < E; j++) {
            const sim::Event e = sim::event(g, (uint32_t)b, (uint32_t)j, t);
            const int64_t o = b * E + j;
            if (out.scaled) out.scaled[o] = e.scaled;
            if (out.lo) out.lo[o] = e.lo;
            if (out.hi) out.hi[o] = e.hi;
            if (out.truth) out.truth[o] = e.truth;
            if (!out.reports) continue;
            for (int64_t i = 0; i < N; i++)
                out.reports[(b * N + i) * E + j] = sim::cell(g, e, who[i], (uint32_t)b, (uint32_t)i, (uint32_t)j, t);
        }
    }
}

hipError_t launch_sim_metrics(int64_t B, int64_t N, int64_t E, double scaled_tol, const pcx_sim_rounds& r,
                              const double* old_rep, const double* smooth_rep, const double* outcomes_final,
                              double* metrics, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((B + SIM_TB - 1) / SIM_TB);
    hipLaunchKernelGGL(k_sim_metrics, dim3(grid), dim3(SIM_TB), 0, st, B, N, E, scaled_tol, r, old_rep, smooth_rep,
                       outcomes_final, metrics);
    return hipGetLastError();
}

hipError_t launch_sim_summary(const double* metrics, int64_t B, double* summary, hipStream_t st) {
    hipLaunchKernelGGL(k_sim_summary, dim3(1), dim3(SIM_TB), 0, st, metrics, B, summary);
    return hipGetLastError();
}

}  // namespace pcx
