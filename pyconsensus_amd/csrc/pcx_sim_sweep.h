// pcx_sim_sweep.h -- simulator sweeps (include/pcx.h "Simulator sweeps"): the
// device tables of a sweep and the launchers of pcx_sim_sweep.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pcx.h"
#include "pcx_sim.h"

namespace pcx {

// One cell of a sweep: where its first round starts in the flat arrays, its shape, its number of
// rounds and its generator.  Round b of the sweep, in cell c, is round b - round0 of the cell (the
// generator's round counter) and starts at cell0 + (b - round0) N E, row0 + (b - round0) N,
// ev0 + (b - round0) E.
struct SweepCell {
    int64_t round0;  // sum of R over earlier cells
    int64_t cell0;   // sum of R N E: reports
    int64_t row0;    // sum of R N: liar, the per-reporter arrays
    int64_t ev0;     // sum of R E: scaled / lo / hi / truth, the per-event arrays
    int64_t R;
    int32_t N, E;
    sim::Gen g;
};
static_assert(sizeof(SweepCell) == 96, "sweep cell table entry");

// The tables as the kernels read them: `cells` [C] and `prefix` [C + 1], prefix[c] = cells[c].round0,
// prefix[C] = B (the search of a round's cell runs over it).
struct SweepTables {
    const SweepCell* cells;
    const int64_t* prefix;
    int32_t C;
    int64_t B;
};

// the cell of round b: the largest c with prefix[c] <= b (prefix[0] = 0 <= b < B = prefix[C])
__device__ __forceinline__ int sweep_cell_of(const int64_t* __restrict__ prefix, int C, int64_t b) {
    int lo = 0, hi = C;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// one timestep's rounds of every cell, flat layout (any pointer of `out` may be NULL).  tall: a cell
// has more than 256 reporters (up to 1024) -- the instantiation with that many reporter flags in LDS
hipError_t launch_sim_sweep_generate(const SweepTables& s, uint32_t t, const pcx_sim_rounds& out, hipStream_t st,
                                     bool tall = false);
// the same on the host: `cells` is a HOST table
void sim_sweep_generate_host(const SweepCell* cells, int64_t C, uint32_t t, const pcx_sim_rounds& out);
// metrics [B][PCX_SIM_NMETRICS] of the sweep's scored rounds
hipError_t launch_sim_sweep_metrics(const SweepTables& s, double scaled_tol, const pcx_sim_rounds& r,
                                    const double* old_rep, const double* smooth_rep, const double* outcomes_final,
                                    double* metrics, hipStream_t st);
// summary [C][PCX_SIM_NMETRICS]: each cell's means over its rounds, in k_sim_summary's order
hipError_t launch_sim_sweep_summary(const SweepTables& s, const double* metrics, double* summary, hipStream_t st);


// k-means code books from the generator's KMEANS stream (pcx_sim_kmeans.hip), on the
// device and on the host, bit for bit.  Rounds of one shape: books [B][restarts][k].  A sweep: round
// b's [restarts][tab[b].k] rows at tab[b].offset of the flat array (k = 0: no book), drawn under its
// cell's key with the round's index inside the cell.
struct KmeansEntry;
hipError_t launch_sim_kmeans_books(const sim::Gen& g, int64_t B, int N, int k, int restarts, uint32_t t,
                                   int32_t* books, hipStream_t st);
void sim_kmeans_books_host(const sim::Gen& g, int64_t B, int N, int k, int restarts, uint32_t t, int32_t* books);
hipError_t launch_sim_sweep_kmeans_books(const SweepTables& s, const KmeansEntry* tab, int restarts, uint32_t t,
                                         int32_t* books, hipStream_t st);
void sim_sweep_kmeans_books_host(const SweepCell* cells, int64_t C, const KmeansEntry* tab, int restarts, uint32_t t,
                                 int32_t* books);

}  // namespace pcx
