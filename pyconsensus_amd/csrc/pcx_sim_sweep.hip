// pcx_sim_sweep.hip -- kernels of the simulator's sweeps (include/pcx.h "Simulator sweeps",
// DESIGN.md 5.4.1): cells of different shapes, rates and seeds in pcx_ragged's flat layout.
//
//   k_sim_sweep_generate  one timestep's rounds.  A work item is one round and one WAVE takes it: with
//                         N <= 256 and E <= 64 a round is a single reporter chunk and a single event
//                         tile of k_sim_generate's scheme, and an event tile is no wider than a wave.
//                         The four waves of a 256-thread workgroup take rounds grid-stride on their
//                         own (no workgroup barrier: a round of one cell costs no idle waves).  A wave
//                         finds its round's cell by a search over the round prefix sums, keeps the
//                         cell's entry in scalar registers, stages the round's reporter flags and event
//                         parameters in its own LDS region, then walks the round's N E cells in memory
//                         order with the carry step, one 8-byte store per lane.
//   k_sim_sweep_metrics   one lane per round, k_sim_metrics' arithmetic with the round's own offsets.
//   k_sim_sweep_summary   one 256-thread workgroup per cell, k_sim_summary's order over the cell's rounds.
//
// The draws are pcx_sim.h's; the round counter is the round's index inside its cell and the key is
// the cell's seed, so a cell's slice is what k_sim_generate writes for that cell alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "pcx_internal.h"
#include "pcx_sim_sweep.h"

namespace pcx {

namespace {
constexpr int SW_TB = 256;     // threads per workgroup
constexpr int SW_WAVE = 64;    // a wave takes a round
constexpr int SW_WAVES = SW_TB / SW_WAVE;
constexpr int SW_MAXN = 256;   // the wide ragged entry's limits
constexpr int SW_TALLN = 1024;  // the tall study's (a sweep with a cell above SW_MAXN reporters)
constexpr int SW_MAXE = 64;    // (<= SW_WAVE: one lane draws one event)
constexpr int SW_GRID = 4096;  // workgroups at most; the rounds beyond are taken grid-stride

// a wave-uniform value into scalar registers
__device__ __forceinline__ int suniform32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t suniform64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// MAXN: the reporters a round may have (its flags' LDS): SW_MAXN, or SW_TALLN for a tall study
template <int MAXN>
__global__ __launch_bounds__(SW_TB) void k_sim_sweep_generate(const SweepTables s, const uint32_t t,
                                                              const pcx_sim_rounds out) {
    __shared__ double s_lo[SW_WAVES][SW_MAXE], s_hi[SW_WAVES][SW_MAXE], s_truth[SW_WAVES][SW_MAXE],
        s_lie[SW_WAVES][SW_MAXE];
    __shared__ uint8_t s_scaled[SW_WAVES][SW_MAXE], s_who[SW_WAVES][MAXN];
    const int lane = threadIdx.x & (SW_WAVE - 1);
    const int w = suniform32(threadIdx.x / SW_WAVE);
    const int64_t step = (int64_t)gridDim.x * SW_WAVES;
    for (int64_t b = (int64_t)blockIdx.x * SW_WAVES + w; b < s.B; b += step) {
        const SweepCell* cp = s.cells + suniform32(sweep_cell_of(s.prefix, s.C, b));
        const int N = suniform32(cp->N), E = suniform32(cp->E);
        const int64_t rb = b - suniform64(cp->round0);  // the round inside its cell: the draws' counter
        const int64_t row = suniform64(cp->row0) + rb * N, ev = suniform64(cp->ev0) + rb * E;
        sim::Gen g;
        g.key0 = (uint32_t)suniform32((int)cp->g.key0);
        g.key1 = (uint32_t)suniform32((int)cp->g.key1);
        g.thr_liar = (uint64_t)suniform64((int64_t)cp->g.thr_liar);
        g.thr_collude = (uint64_t)suniform64((int64_t)cp->g.thr_collude);
        g.thr_distort = (uint64_t)suniform64((int64_t)cp->g.thr_distort);
        g.thr_na = (uint64_t)suniform64((int64_t)cp->g.thr_na);
        g.thr_scaled = (uint64_t)suniform64((int64_t)cp->g.thr_scaled);
        // reporters from the last lane down, the events from the first up (up to three Philox calls
        // each): in a small round other lanes take them
        for (int r = SW_WAVE - 1 - lane; r < N; r += SW_WAVE) {
            const uint8_t who = sim::reporter(g, (uint32_t)rb, (uint32_t)r);
            s_who[w][r] = who;
            if (out.liar) out.liar[row + r] = who;
        }
        if (lane < E) {
            const sim::Event e = sim::event(g, (uint32_t)rb, (uint32_t)lane, t);
            s_lo[w][lane] = e.lo;
            s_hi[w][lane] = e.hi;
            s_truth[w][lane] = e.truth;
            s_lie[w][lane] = e.lie;
            s_scaled[w][lane] = e.scaled;
            const int64_t o = ev + lane;
            if (out.scaled) out.scaled[o] = e.scaled;
            if (out.lo) out.lo[o] = e.lo;
            if (out.hi) out.hi[o] = e.hi;
            if (out.truth) out.truth[o] = e.truth;
        }
        wave_sync();
        if (out.reports) {
            // cell c of the round is (c / E, c % E); c steps by the wave, so (i, j) step by
            // (SW_WAVE / E, SW_WAVE % E) with a carry: no division per cell
            const int cells = N * E;
            const int di = SW_WAVE / E, dj = SW_WAVE % E;
            int i = lane / E, j = lane % E;
            double* base = out.reports + (suniform64(cp->cell0) + rb * cells);
            for (int c = lane; c < cells; c += SW_WAVE) {
                sim::Event e;
                e.lo = s_lo[w][j];
                e.hi = s_hi[w][j];
                e.truth = s_truth[w][j];
                e.lie = s_lie[w][j];
                e.scaled = s_scaled[w][j];
                base[c] = sim::cell(g, e, s_who[w][i], (uint32_t)rb, (uint32_t)i, (uint32_t)j, t);
                i += di;
                j += dj;
                if (j >= E) {
                    j -= E;
                    i++;
                }
            }
        }
        wave_sync();  // the wave's next round overwrites its LDS
    }
}

__global__ __launch_bounds__(SW_TB) void k_sim_sweep_metrics(const SweepTables s, const double scaled_tol,
                                                             const pcx_sim_rounds r,
                                                             const double* __restrict__ old_rep,
                                                             const double* __restrict__ smooth_rep,
                                                             const double* __restrict__ outcomes_final,
                                                             double* __restrict__ metrics) {
    const int64_t b = (int64_t)blockIdx.x * SW_TB + threadIdx.x;
    if (b >= s.B) return;
    const SweepCell* cp = s.cells + sweep_cell_of(s.prefix, s.C, b);
    const int64_t N = cp->N, E = cp->E, rb = b - cp->round0;
    const int64_t row = cp->row0 + rb * N, ev = cp->ev0 + rb * E;
    int64_t ok = 0;
    for (int64_t j = 0; j < E; j++) {
        const int64_t o = ev + j;
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
        const int64_t o = row + i;
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

__global__ __launch_bounds__(SW_TB) void k_sim_sweep_summary(const SweepTables s, const double* __restrict__ metrics,
                                                             double* __restrict__ summary) {
    __shared__ double sh[PCX_SIM_NMETRICS][SW_TB];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int64_t R = s.cells[c].R;
    const double* m = metrics + s.cells[c].round0 * PCX_SIM_NMETRICS;
    double acc[PCX_SIM_NMETRICS];
    for (int k = 0; k < PCX_SIM_NMETRICS; k++) acc[k] = 0.0;
    for (int64_t b = tid; b < R; b += SW_TB)
        for (int k = 0; k < PCX_SIM_NMETRICS; k++) acc[k] += m[b * PCX_SIM_NMETRICS + k];
    for (int k = 0; k < PCX_SIM_NMETRICS; k++) sh[k][tid] = acc[k];
    __syncthreads();
    for (int stride = SW_TB / 2; stride >= 1; stride >>= 1) {
        if (tid < stride)
            for (int k = 0; k < PCX_SIM_NMETRICS; k++) sh[k][tid] += sh[k][tid + stride];
        __syncthreads();
    }
    if (tid < PCX_SIM_NMETRICS) summary[c * PCX_SIM_NMETRICS + tid] = sh[tid][0] / (double)R;
}
}  // namespace

hipError_t launch_sim_sweep_generate(const SweepTables& s, uint32_t t, const pcx_sim_rounds& out, hipStream_t st,
                                     bool tall) {
    if (s.B <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<int64_t>((s.B + SW_WAVES - 1) / SW_WAVES, SW_GRID);
    (void)hipGetLastError();
    if (tall)
        hipLaunchKernelGGL(k_sim_sweep_generate<SW_TALLN>, dim3(grid), dim3(SW_TB), 0, st, s, t, out);
    else
        hipLaunchKernelGGL(k_sim_sweep_generate<SW_MAXN>, dim3(grid), dim3(SW_TB), 0, st, s, t, out);
    return hipGetLastError();
}

void sim_sweep_generate_host(const SweepCell* cells, int64_t C, uint32_t t, const pcx_sim_rounds& out) {
    for (int64_t c = 0; c < C; c++) {
        const SweepCell& k = cells[c];
        pcx_sim_rounds o;
        o.reports = out.reports ? out.reports + k.cell0 : nullptr;
        o.scaled = out.scaled ? out.scaled + k.ev0 : nullptr;
        o.lo = out.lo ? out.lo + k.ev0 : nullptr;
        o.hi = out.hi ? out.hi + k.ev0 : nullptr;
        o.truth = out.truth ? out.truth + k.ev0 : nullptr;
        o.liar = out.liar ? out.liar + k.row0 : nullptr;
        sim_generate_host(k.g, k.R, k.N, k.E, t, o);
    }
}

hipError_t launch_sim_sweep_metrics(const SweepTables& s, double scaled_tol, const pcx_sim_rounds& r,
                                    const double* old_rep, const double* smooth_rep, const double* outcomes_final,
                                    double* metrics, hipStream_t st) {
    if (s.B <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((s.B + SW_TB - 1) / SW_TB);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_sim_sweep_metrics, dim3(grid), dim3(SW_TB), 0, st, s, scaled_tol, r, old_rep, smooth_rep,
                       outcomes_final, metrics);
    return hipGetLastError();
}

hipError_t launch_sim_sweep_summary(const SweepTables& s, const double* metrics, double* summary, hipStream_t st) {
    if (s.C <= 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_sim_sweep_summary, dim3((unsigned)s.C), dim3(SW_TB), 0, st, s, metrics, summary);
    return hipGetLastError();
}

}  // namespace pcx
