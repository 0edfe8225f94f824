// pcx_sim_kmeans.hip -- the simulator's k-means code books (include/pcx.h "k-means in the simulator",
// DESIGN.md 5.4.4): every (round, restart)'s initial code book drawn from the generator's KMEANS
// stream (pcx_sim.h kmeans_book, one source for both sides) into a flat int32 array that the round
// kernels read.
//
//   k_kmeans_books        rounds of one shape: thread (b, r) writes books[b][r][0 .. k).
//   k_kmeans_books_sweep  a sweep's rounds: thread (b, r) finds round b's cell as the sweep generator
//                         does (the search over the round prefix sums), draws under the cell's key with
//                         the round's index inside its cell, and writes through the per-round table
//                         {offset, k} (k = 0: the round has no book).
//
// A book is at most 16 rows: the serial Floyd loop of one thread costs 16 Philox calls, next to the
// tens of microseconds of Lloyd steps that read it.
#include <hip/hip_runtime.h>

#include "pcx_internal.h"
#include "pcx_sim_sweep.h"

namespace pcx {

namespace {
constexpr int KB_TB = 256;

__global__ __launch_bounds__(KB_TB) void k_kmeans_books(const sim::Gen g, const int64_t B, const int N, const int k,
                                                        const int restarts, const uint32_t t,
                                                        int32_t* __restrict__ books) {
    const int64_t id = (int64_t)blockIdx.x * KB_TB + threadIdx.x;
    if (id >= B * restarts) return;
    const int64_t b = id / restarts;
    const int r = (int)(id - b * restarts);
    sim::kmeans_book(g, (uint32_t)b, (uint32_t)r, t, N, k, books + id * k);
}

__global__ __launch_bounds__(KB_TB) void k_kmeans_books_sweep(const SweepTables s, const KmeansEntry* __restrict__ tab,
                                                              const int restarts, const uint32_t t,
                                                              int32_t* __restrict__ books) {
    const int64_t id = (int64_t)blockIdx.x * KB_TB + threadIdx.x;
    if (id >= s.B * restarts) return;
    const int64_t b = id / restarts;
    const int r = (int)(id - b * restarts);
    const int k = tab[b].k;
    if (k == 0) return;
    const SweepCell* cp = s.cells + sweep_cell_of(s.prefix, s.C, b);
    sim::kmeans_book(cp->g, (uint32_t)(b - cp->round0), (uint32_t)r, t, cp->N, k, books + tab[b].offset + (int64_t)r * k);
}
}  // namespace

hipError_t launch_sim_kmeans_books(const sim::Gen& g, int64_t B, int N, int k, int restarts, uint32_t t,
                                   int32_t* books, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((B * restarts + KB_TB - 1) / KB_TB);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_kmeans_books, dim3(grid), dim3(KB_TB), 0, st, g, B, N, k, restarts, t, books);
    return hipGetLastError();
}

void sim_kmeans_books_host(const sim::Gen& g, int64_t B, int N, int k, int restarts, uint32_t t, int32_t* books) {
    for (int64_t b = 0; b < B; b++)
        for (int r = 0; r < restarts; r++)
            sim::kmeans_book(g, (uint32_t)b, (uint32_t)r, t, N, k, books + (b * restarts + r) * k);
}

hipError_t launch_sim_sweep_kmeans_books(const SweepTables& s, const KmeansEntry* tab, int restarts, uint32_t t,
                                         int32_t* books, hipStream_t st) {
    if (s.B <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((s.B * restarts + KB_TB - 1) / KB_TB);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_kmeans_books_sweep, dim3(grid), dim3(KB_TB), 0, st, s, tab, restarts, t, books);
    return hipGetLastError();
}

void sim_sweep_kmeans_books_host(const SweepCell* cells, int64_t C, const KmeansEntry* tab, int restarts, uint32_t t,
                                 int32_t* books) {
    for (int64_t c = 0; c < C; c++) {
        const SweepCell& cell = cells[c];
        for (int64_t rb = 0; rb < cell.R; rb++) {
            const KmeansEntry& e = tab[cell.round0 + rb];
            for (int r = 0; r < restarts && e.k > 0; r++)
                sim::kmeans_book(cell.g, (uint32_t)rb, (uint32_t)r, t, cell.N, e.k, books + e.offset + (int64_t)r * e.k);
        }
    }
}

}  // namespace pcx
