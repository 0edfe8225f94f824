// pcx_mat_hard.hip -- the hard replay of the medians and fills in the reference's own float order,
// with its bitonic sort (hard_stage, hard_list).
#include "pcx_mat_device.h"

namespace pcx {
namespace {

// ------------------------------------------------------------------ hard replay
// Events whose decision sits within rounding of a threshold are replayed in the
// reference's own order.  Phase 1 (interpolate, :287-309): the present reports of the
// event in row order with weights rep_j / (sequential total); binary events: the
// sequential weighted mean then catch; scaled events: weightedstats on those pairs.
// Phase 2 (:519-523): weightedstats over the filled column with smooth_rep.

// this rank's elements of hard event j in row order -> send[j][0 .. cnt)
__global__ void __launch_bounds__(1024) k_hard_gather(pcx_mat m, HardArgs h) {
    const int j = blockIdx.x;
    const int c = h.cols[j];
    const ColParam p = col_param(m, c, true);
    double* out = h.send + (int64_t)j * h.cap * 2;
    const double* wsrc = m.sel_phase == 1 ? m.rep : m.rowv + RV_SMOOTH * m.n_rows;
    const int64_t E = m.n_events;
    const int sidx = m.scaled_index ? m.scaled_index[c] : -1;
    if (h.modes[j] == HARD_MEDIAN && sidx >= 0) {
        // a median's values come from T (k_colstats: the rescaled present value, NaN where missing,
        // one contiguous column) instead of a strided column of the row-major reports
        const double* Tc = m.T + (int64_t)sidx * m.n_rows;
        const double g = p.guess;
        const int64_t nt = block_compact(
            m.n_rows,
            [&](int64_t i) {
                const double v = Tc[i];
                if (m.sel_phase == 1) return !__builtin_isnan(v);
                return !__builtin_isnan(__builtin_isnan(v) ? g : v);
            },
            [&](int64_t i, int64_t pos) {
                const double v = Tc[i];
                out[pos * 2 + 0] = __builtin_isnan(v) ? g : v;
                out[pos * 2 + 1] = wsrc[i];
            });
        if (threadIdx.x == 0) h.send_cnt[j] = nt;
        return;
    }
    const int64_t n = block_compact(
        m.n_rows,
        [&](int64_t i) {
            const double x = rescale(m.reports[i * E + c], p, m.int_dtype);
            if (m.sel_phase == 1) return !missing(x);
            return !__builtin_isnan(missing(x) ? p.guess : x);
        },
        [&](int64_t i, int64_t pos) {
            const double x = rescale(m.reports[i * E + c], p, m.int_dtype);
            out[pos * 2 + 0] = missing(x) ? p.guess : x;
            out[pos * 2 + 1] = wsrc[i];
        });
    if (threadIdx.x == 0) h.send_cnt[j] = n;
}

// The hard replay's sequential fp64 chains (weightedstats' builtin sums and its walk) run on one
// lane: a dependent add per element is the floor (~8 cycles).  The lane reads its operands from
// an LDS tile in 16-element chunks, the next chunk's loads issued before the current chunk's adds,
// so the LDS latency (~50-60 cycles) hides behind the chain instead of stalling it every 8
// elements; the tiles are double-buffered: waves 1.. fill tile t+1 while lane 0 chains tile t.
constexpr int CHAIN = 16;

// acc + t[0] + t[1] + ... + t[len-1], left to right
__device__ __forceinline__ double chain_add(const double* t, int len, double acc) {
    double a[CHAIN], b[CHAIN];
    int k = 0;
    if (len >= CHAIN) {
#pragma unroll
        for (int j = 0; j < CHAIN; j++) a[j] = t[j];
        for (; k + 2 * CHAIN <= len; k += 2 * CHAIN) {
#pragma unroll
            for (int j = 0; j < CHAIN; j++) b[j] = t[k + CHAIN + j];
#pragma unroll
            for (int j = 0; j < CHAIN; j++) acc = acc + a[j];
            if (k + 3 * CHAIN <= len) {
#pragma unroll
                for (int j = 0; j < CHAIN; j++) a[j] = t[k + 2 * CHAIN + j];
            }
#pragma unroll
            for (int j = 0; j < CHAIN; j++) acc = acc + b[j];
        }
        if (k + CHAIN <= len) {  // a chunk loaded into a[] and not yet added
#pragma unroll
            for (int j = 0; j < CHAIN; j++) acc = acc + a[j];
            k += CHAIN;
        }
    }
    for (; k < len; k++) acc = acc + t[k];
    return acc;
}

// sequential left-to-right fp64 sum of f(k), k in [0, n): lane 0 chains, waves 1.. stage the
// tiles (tile: 2 * TILE doubles of LDS)
template <class F>
__device__ double block_serial_sum(int64_t n, F f, double* tile, int TILE) {
    __shared__ double acc_s;
    double acc = 0.0;
    const int loaders = (int)blockDim.x - WAVE;
    for (int k = threadIdx.x; k < TILE && k < n; k += blockDim.x) tile[k] = f(k);
    __syncthreads();
    int it = 0;
    for (int64_t t0 = 0; t0 < n; t0 += TILE, it++) {
        const int len = (int)(n - t0 < TILE ? n - t0 : TILE);
        const double* cur = tile + (it & 1) * TILE;
        double* nxt = tile + ((it + 1) & 1) * TILE;
        if (threadIdx.x == 0) {
            acc = chain_add(cur, len, acc);
        } else if ((int)threadIdx.x >= WAVE) {
            const int64_t n0 = t0 + TILE;
            const int nl = (int)(n - n0 < TILE ? (n - n0 > 0 ? n - n0 : 0) : TILE);
            for (int k = threadIdx.x - WAVE; k < nl; k += loaders) nxt[k] = f(n0 + k);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) acc_s = acc;
    __syncthreads();
    return acc_s;
}

constexpr int HARD_TILE = 4096;

__global__ void __launch_bounds__(1024) k_hard_prep(pcx_mat m, HardArgs h) {
    __shared__ double tile[2 * HARD_TILE];
    __shared__ unsigned long long wkey_s, first_s;
    __shared__ int pos_s, dom_s, neg_s;
    const int j = blockIdx.x;
    const int c = h.cols[j];
    const int mode = h.modes[j];
    const int64_t N = m.n_total;
    double* X = h.X + (int64_t)j * N;
    double* W = h.W + (int64_t)j * N;
    double* hs = h.hs + (int64_t)j * 4;
    // concatenate the ranks' rows (rank order = row order)
    int64_t n = 0;
    for (int w = 0; w < m.world; w++) {
        const int64_t cw = h.recv_cnt[(int64_t)w * h.n_hard + j];
        const double* src = h.recv + ((int64_t)w * h.n_hard + j) * h.cap * 2;
        for (int64_t k = threadIdx.x; k < cw; k += blockDim.x) {
            X[n + k] = src[2 * k];
            W[n + k] = src[2 * k + 1];
        }
        n += cw;
    }
    __syncthreads();
    if (m.sel_phase == 1) {  // weights rep_j / sequential total of the present rep (:294-302)
        const double tot = block_serial_sum(n, [&](int64_t k) { return W[k]; }, tile, HARD_TILE);
        for (int64_t k = threadIdx.x; k < n; k += blockDim.x) W[k] = W[k] / tot;
        __syncthreads();
    }
    const int s = m.scaled_index ? m.scaled_index[c] : -1;
    if (mode == HARD_MEAN) {  // guess = sum_seq(w * x) then catch (:304-309)
        const double g = block_serial_sum(n, [&](int64_t k) { return W[k] * X[k]; }, tile, HARD_TILE);
        if (threadIdx.x == 0) {
            double v = n > 0 ? catch_value(g, m.catch_tolerance) : catch_value(0.0, m.catch_tolerance);
            if (m.int_dtype) v = trunc(v);
            m.ev[EV_GUESS * m.n_events + c] = v;
            hs[2] = 0.0;
        }
        return;
    }
    uint64_t* st = m.sel_state + (int64_t)s * SELS;
    const double mid = 0.5 * block_serial_sum(n, [&](int64_t k) { return W[k]; }, tile, HARD_TILE);
    // dominance: any(w > mid) -> data[first index of max(w)]; no positive weight -> None.
    // Weights may be negative (a negative reputation): max over order-preserving keys.
    if (threadIdx.x == 0) {
        wkey_s = 0;
        first_s = ~0ull;
        pos_s = 0;
        dom_s = 0;
        neg_s = 0;
    }
    __syncthreads();
    double wl = -__builtin_inf();
    int posl = 0, doml = 0, negl = 0;
    for (int64_t k = threadIdx.x; k < n; k += blockDim.x) {
        wl = fmax(wl, W[k]);
        posl |= W[k] > 0.0;
        doml |= W[k] > mid;
        negl |= W[k] < 0.0;
    }
    if (negl) neg_s = 1;
    wl = wave_max_d(wl);
    if ((threadIdx.x & 63) == 0) atomicMax(&wkey_s, (unsigned long long)dkey(wl));
    if (posl) pos_s = 1;
    if (doml) dom_s = 1;
    __syncthreads();
    if (dom_s) {
        const double wmax = dkey_inv(wkey_s);  // some W[k] > mid: the max is a finite element
        for (int64_t k = threadIdx.x; k < n; k += blockDim.x)
            if (W[k] == wmax) {
                atomicMin(&first_s, (unsigned long long)k);
                break;
            }
        __syncthreads();
        if (threadIdx.x == 0) {
            sel_done(st, X[first_s]);
            hs[2] = 0.0;
        }
        return;
    }
    if (!pos_s) {
        if (threadIdx.x == 0) {
            sel_done(st, __builtin_nan(""));
            hs[2] = 0.0;
        }
        return;
    }
    uint64_t* keys = h.keys + (int64_t)j * h.P * 2;
    for (int64_t k = threadIdx.x; k < h.P; k += blockDim.x) {
        keys[2 * k + 0] = k < n ? dkey(X[k]) : ~0ull;
        keys[2 * k + 1] = k < n ? dkey(W[k]) : ~0ull;
    }
    if (threadIdx.x == 0) {
        hs[0] = mid;
        hs[1] = (double)n;
        hs[2] = 1.0;  // sort + walk pending
        hs[3] = neg_s ? 1.0 : 0.0;  // some weight < 0: the walk's partial sums are not monotone
    }
}

// bitonic sort of every segment keys[j][0 .. P) by (value key, weight key)
__device__ __forceinline__ bool key_gt(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl) {
    return ah > bh || (ah == bh && al > bl);
}

constexpr int BS_TILE = 4096;  // elements sorted in LDS per block (64 KB)

// stages size <= min(P, BS_TILE) of the network (init) or strides < BS_TILE of one size (merge)
__global__ void __launch_bounds__(1024) k_bsort_lds(uint64_t* keys, int64_t P, int64_t size_only) {
    __shared__ uint64_t kh[BS_TILE], kl[BS_TILE];
    const int64_t tile = P < BS_TILE ? P : BS_TILE;
    const int64_t base = (int64_t)blockIdx.x * tile;  // global element index (segments are contiguous)
    for (int k = threadIdx.x; k < tile; k += 1024) {
        kh[k] = keys[2 * (base + k)];
        kl[k] = keys[2 * (base + k) + 1];
    }
    __syncthreads();
    const int64_t s0 = size_only ? size_only : 2;
    const int64_t s1 = size_only ? size_only : tile;
    for (int64_t size = s0; size <= s1; size <<= 1) {
        for (int64_t stride = (size_only ? tile : size) >> 1; stride > 0; stride >>= 1) {
            if (stride >= size) continue;
            for (int t = threadIdx.x; t < tile / 2; t += 1024) {
                const int lo = (int)(2 * stride * (t / stride) + (t % stride));
                const int hi = lo + (int)stride;
                const int64_t g = (base + lo) % P;  // index within the segment: direction
                const bool up = (g & size) == 0;
                const bool gt = key_gt(kh[lo], kl[lo], kh[hi], kl[hi]);
                if (gt == up) {
                    const uint64_t a = kh[lo], b = kl[lo];
                    kh[lo] = kh[hi];
                    kl[lo] = kl[hi];
                    kh[hi] = a;
                    kl[hi] = b;
                }
            }
            __syncthreads();
        }
    }
    for (int k = threadIdx.x; k < tile; k += 1024) {
        keys[2 * (base + k)] = kh[k];
        keys[2 * (base + k) + 1] = kl[k];
    }
}

__global__ void __launch_bounds__(BT) k_bsort_global(uint64_t* keys, int64_t P, int64_t total, int64_t size,
                                                     int64_t stride) {
    for (int64_t t = blockIdx.x * (int64_t)BT + threadIdx.x; t < total / 2; t += (int64_t)gridDim.x * BT) {
        const int64_t lo = 2 * stride * (t / stride) + (t % stride);
        const int64_t hi = lo + stride;
        const bool up = ((lo % P) & size) == 0;
        const uint64_t ah = keys[2 * lo], al = keys[2 * lo + 1], bh = keys[2 * hi], bl = keys[2 * hi + 1];
        if (key_gt(ah, al, bh, bl) == up) {
            keys[2 * lo] = bh;
            keys[2 * lo + 1] = bl;
            keys[2 * hi] = ah;
            keys[2 * hi + 1] = al;
        }
    }
}

// the walk (:weighted_median while loop) over the sorted pairs of each pending event
__global__ void __launch_bounds__(1024) k_hard_walk(pcx_mat m, HardArgs h) {
    constexpr int TWS = HARD_TILE + 2 * CHAIN;  // a tile and the padding the chain's prefetch reads
    __shared__ double tw[2 * TWS];
    __shared__ int done_s;
    __shared__ int64_t k_s;
    __shared__ double cum_s;
    const int j = blockIdx.x;
    double* hs = h.hs + (int64_t)j * 4;
    if (h.modes[j] != HARD_MEDIAN || hs[2] != 1.0) return;
    const int c = h.cols[j];
    uint64_t* st = m.sel_state + (int64_t)m.scaled_index[c] * SELS;
    const uint64_t* keys = h.keys + (int64_t)j * h.P * 2;
    const double mid = hs[0];
    const int64_t n = (int64_t)hs[1];
    const bool monotone = hs[3] == 0.0;  // every weight >= 0: a chunk's last partial is its largest
    if (threadIdx.x == 0) {
        done_s = 0;
        k_s = 0;
        cum_s = 0.0;
    }
    // (a partial tile is followed by zeros: a chunk that runs past the last weight adds + 0.0)
    for (int k = threadIdx.x; k < TWS; k += blockDim.x) tw[k] = k < n && k < HARD_TILE ? dkey_inv(keys[2 * k + 1]) : 0.0;
    __syncthreads();
    // cum += w while cum <= mid (weightedstats' walk; mid > 0 here, so the first add always runs):
    // lane 0 adds a chunk's weights unconditionally -- partial sums up to the first one above mid
    // are exactly the walk's -- then finds that first one; waves 1.. stage the next tile meanwhile
    const int loaders = (int)blockDim.x - WAVE;
    int it = 0;
    for (int64_t t0 = 0; t0 < n; t0 += HARD_TILE, it++) {
        const int len = (int)(n - t0 < HARD_TILE ? n - t0 : HARD_TILE);
        const double* cur = tw + (it & 1) * TWS;
        double* nxt = tw + ((it + 1) & 1) * TWS;
        if (threadIdx.x == 0) {
            // static register indices only (a dynamic p[hit] sends the array to scratch); the tiles
            // are padded by 2 CHAIN so the next chunk's loads need no bounds test
            double cum = cum_s, hit_cum = 0.0;
            int hit_at = -1;
            double nv[CHAIN];
#pragma unroll
            for (int q = 0; q < CHAIN; q++) nv[q] = cur[q];
            for (int k = 0; k < len; k += CHAIN) {
                double v[CHAIN], p[CHAIN];
#pragma unroll
                for (int q = 0; q < CHAIN; q++) v[q] = nv[q];  // (past len: the tile's zero padding)
#pragma unroll
                for (int q = 0; q < CHAIN; q++) nv[q] = cur[k + CHAIN + q];  // the next chunk, in flight
                double acc = cum;
#pragma unroll
                for (int q = 0; q < CHAIN; q++) {
                    acc = acc + v[q];
                    p[q] = acc;
                }
                if (monotone && !(acc > mid)) {  // no partial of this chunk exceeds mid
                    cum = acc;
                    continue;
                }
                int h = -1;
                double hc = 0.0;
#pragma unroll
                for (int q = CHAIN - 1; q >= 0; q--)
                    if (p[q] > mid) {  // (padded partials repeat the last real one)
                        h = q;
                        hc = p[q];
                    }
                if (h >= 0) {
                    hit_at = k + h;
                    hit_cum = hc;
                    break;
                }
                cum = acc;
            }
            if (hit_at >= 0) {
                cum_s = hit_cum;
                k_s = t0 + hit_at + 1;
                done_s = 1;
            } else {
                cum_s = cum;
                k_s = t0 + len;
            }
        } else if ((int)threadIdx.x >= WAVE) {
            const int64_t n0 = t0 + HARD_TILE;
            const int nl = (int)(n - n0 < HARD_TILE ? (n - n0 > 0 ? n - n0 : 0) : HARD_TILE);
            for (int k = threadIdx.x - WAVE; k < TWS; k += loaders) nxt[k] = k < nl ? dkey_inv(keys[2 * (n0 + k) + 1]) : 0.0;
        }
        __syncthreads();
        if (done_s) break;
    }
    if (threadIdx.x == 0) {
        double res;
        const int64_t k = k_s;
        if (!done_s) {
            res = __builtin_nan("");  // the walk ran off the end (the reference raises IndexError)
        } else {
            const double wk = dkey_inv(keys[2 * (k - 1) + 1]);
            const double before = cum_s - wk;
            const double xk = dkey_inv(keys[2 * (k - 1)]);
            if (fabs(before - mid) < 2.220446049250313080847e-16) {
                if (k >= 2)
                    res = (dkey_inv(keys[2 * (k - 2)]) + xk) / 2.0;
                else
                    res = n == 1 ? xk / 1.0 : __builtin_nan("");
            } else {
                res = xk;
            }
        }
        sel_done(st, res);
        hs[2] = 0.0;
    }
}

// events marked hard (m.hard[c] != 0) in event order -> cols / modes, count -> info[IN_HARD]
__global__ void __launch_bounds__(1024) k_hard_list(pcx_mat m, int32_t* cols, int32_t* modes) {
    const int64_t cnt = block_compact(
        m.n_events, [&](int64_t c) { return m.hard[c] != HARD_NONE; },
        [&](int64_t c, int64_t pos) {
            cols[pos] = (int32_t)c;
            modes[pos] = m.hard[c];
        });
    if (threadIdx.x == 0) m.info[IN_HARD] = cnt;
}

}  // namespace

hipError_t hard_stage(pcx_mat& m, const HardArgs& h, int stage, hipStream_t st, std::string& err) {
    if (h.n_hard <= 0) return hipSuccess;
    switch (stage) {
        case M_HARD_GATHER:
            hipLaunchKernelGGL(k_hard_gather, dim3(h.n_hard), dim3(1024), 0, st, m, h);
            break;
        case M_HARD_PREP:
            hipLaunchKernelGGL(k_hard_prep, dim3(h.n_hard), dim3(1024), 0, st, m, h);
            break;
        case M_HARD_SORT: {
            // bitonic network over n_hard contiguous segments of P (a power of two)
            const int64_t P = h.P, total = P * h.n_hard;
            const int64_t tile = P < BS_TILE ? P : BS_TILE;
            const unsigned nblk = (unsigned)(total / tile);
            hipLaunchKernelGGL(k_bsort_lds, dim3(nblk), dim3(1024), 0, st, h.keys, P, (int64_t)0);
            for (int64_t size = tile * 2; size <= P; size <<= 1) {
                for (int64_t stride = size >> 1; stride >= tile; stride >>= 1)
                    hipLaunchKernelGGL(k_bsort_global, dim3(grid_rows(total / 2, BT)), dim3(BT), 0, st, h.keys, P,
                                       total, size, stride);
                hipLaunchKernelGGL(k_bsort_lds, dim3(nblk), dim3(1024), 0, st, h.keys, P, size);
            }
            break;
        }
        case M_HARD_WALK:
            hipLaunchKernelGGL(k_hard_walk, dim3(h.n_hard), dim3(1024), 0, st, m, h);
            break;
        default:
            err = "hard_stage: unknown stage";
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// hard-list compaction (events with m.hard[c] != 0) into cols / modes, count -> info[IN_HARD]
hipError_t hard_list(pcx_mat& m, int32_t* cols, int32_t* modes, hipStream_t st) {
    hipLaunchKernelGGL(k_hard_list, dim3(1), dim3(1024), 0, st, m, cols, modes);
    return hipGetLastError();
}

}  // namespace pcx
