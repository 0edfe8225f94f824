// pcx_mat_layout.h -- the slot layout of the single-matrix path's shared buffers (pcx_mat: ev, rowv,
// scal, info, pvec, sel_state, wdig), one definition for the runner that allocates and exchanges them
// (pcx_runner.cpp) and the kernels that index them (pcx_matrix.hip, pcx_mat_*.hip).  Of cstat and cmax
// only the strides: their slots are still numbers in the kernels (cst(m, c, k)) and in the runner's
// gather_slots calls.  Plain C++.
#pragma once
#include <stdint.h>

namespace pcx {

constexpr int BT = 256;          // threads per block for row/column passes
constexpr int CS = 16;           // dd slots per column in cstat
constexpr int SS = 16;           // dd slots in scal
constexpr int CM = 8;            // doubles per column in mpart / cmax
constexpr int SELS = 40;         // sel_state words per scaled event
constexpr int COV_TILE = 128;    // covariance tile edge: wcd_ld and cov_jb count tiles of it
constexpr int CT = COV_TILE;     // (the kernels' name for it)

// E-sized rows of ev
enum ev_slot { EV_GUESS = 0, EV_MU, EV_OLD, EV_LD, EV_D1, EV_D2, EV_RAW, EV_ADJ, EV_FIN, EV_CERT, EV_PC,
               EV_MINX, EV_MAXX, EV_MISS, EV_NZERO, EV_SPARE, EV_LDP, EV_K, EV_MUP, EV_NSLOT };
// n_rows-sized rows of rowv
enum row_slot { RV_S = 0, RV_U, RV_THIS, RV_SMOOTH, RV_N1, RV_N2, RV_NSLOT };
// dd slots of scal (SC_BIGTOK: count of tokens outside [0, 63])
enum scal_slot { SC_TOK = 0, SC_REP, SC_A1, SC_A1P, SC_A2, SC_A2P, SC_U, SC_UP, SC_AR, SC_ARP, SC_BIGTOK, SC_MAXTOK };
static_assert(SC_MAXTOK < SS, "scal slots");
// header words of wdig: the largest |w| bits of normalize(set1), normalize(set2), smooth_rep
enum wdig_slot { WD_N1 = 0, WD_N2, WD_SMOOTH };
// info[] words (host-visible status; the runner reads them)
enum info_slot { IN_BRANCH = 0, IN_PI_ITERS, IN_FLAGS, IN_SEL_ACTIVE, IN_SEL_ARGMAX, IN_PICK1, IN_HARD, IN_SEL_WACTIVE,
                 IN_COV_GENERAL, IN_COV_MIXED, IN_COV_TOK1, IN_SEL_WLIMB, IN_COV_GUARD, IN_COV_GUARD_COLS,
                 IN_COV_GUARD_BOUND,
                 IN_PI_MAXBITS,  // M_POWER's squaring scratch: max |M M| bits (word 8 holds the plan's general
                                 // count, which the compact passes after that stage read)
                 IN_NSLOT };

// pvec: PV_NROW rows of pv_stride(E) doubles -- the power iteration's x and y (M_DECIDE: y holds
// normalize(set2) . F, PV_RAW1 normalize(set1) . F) and a row of scalars
enum pv_row { PV_X = 0, PV_Y, PV_RAW1, PV_S, PV_NROW };
// words of the PV_S row: the power iteration's delta = max |x_new - x_old| of the last step, 1 once
// delta <= its tolerance, steps run; M_FINAL's 1 - participation; M_DECIDE's rank-rule reference sum
enum pv_scalar { PS_DELTA = 0, PS_DONE, PS_STEPS, PS_PNA = 4, PS_RANKREF = 8 };
constexpr int64_t pv_stride(int64_t E) { return E + 64; }

// sel_state words of one scaled event
enum sel_word {
    SW_STATUS = 0,   // 0 done, 1 histogram pass pending, 2 dominant weight (first argmax row), 3 hard
    SW_LO, SW_HI, SW_SHIFT,           // current key range and bucket shift
    SW_BELOW0, SW_BELOW1, SW_BELOW2,  // exact weight before the range
    SW_TOT0, SW_TOT1, SW_TOT2,        // exact total weight
    SW_BELOW_MAX, SW_HAS_BELOW,       // largest key before the range
    SW_RESULT,                        // result bits (status 0)
    SW_WMAX,                          // max weight bits
    SW_MODE,                          // 0 weight walk, 1 count rank (equal weights)
    SW_NEED,                          // phase 1: the event has missing reports
    SW_COUNT,                         // elements
    SW_TARGET,                        // count mode: 0-based rank of the crossing element
    SW_CNT_BELOW,                     // count mode: elements before the range
    SW_HALF,                          // count mode: 1 exact half (mean with predecessor), 2 half at k*=1
    SW_INRANGE,                       // elements (all ranks) in [LO, HI] after the last step
    SW_CMODE,                         // 1: this rank's in-range elements are compacted in cbuf
    SW_GN, SW_GW0, SW_GW1, SW_GW2,    // phase 2, this rank: filled (missing) rows -- all at the fill
                                      // value -- count and raw weight limb sums, binned once per pass
    SW_WB0, SW_WB1,                   // first pass: the bucket window gathered into cbuf (sampled)
    SW_CERTN, SW_CW0, SW_CW1, SW_CW2, // phase 2, weight walk ended on one key: the elements (all ranks)
                                      // holding it and their exact weight -- the certainty (:540-546)
    SW_NWORDS
};
static_assert(SW_NWORDS <= SELS, "sel_state words");

// blocks of a grid-stride pass over n items, per_block each (at most 4096)
inline int grid_rows(int64_t n, int per_block) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (int)g;
}

}  // namespace pcx
