// pcx_medium_device.inc -- the device helpers of the workgroup-per-round kernel (reductions, the
// weighted median, the Jacobi component scores, the clusterings, the LDS carve sizes), included inside
// namespace pcx { namespace { by pcx_medium.hip (medium_round_kernel) and by pcx_medium_ragged.hip
// (ragged_medium_kernel): two translation units, so the equal-shape kernels keep the code object
// they had before the ragged form existed.  pcx_tall.hip includes it under PCX_MEDIUM_TALL 1 for rounds
// of up to 1024 reporters: where a comment below says n <= 256, the text under that macro lifts it
// (mpw, the NaN rank path of wv_wmedian, bvecmat_chunked, tall_plan); without the macro nothing changes.
#ifndef PCX_MEDIUM_TALL
#define PCX_MEDIUM_TALL 0  // 1: pcx_tall.hip (tall_round_kernel, rounds of up to 1024 reporters; DESIGN.md 5.3.1)
#endif
#if PCX_MEDIUM_TALL
#ifndef PCX_TALL_THREADS  // 256, 512 and 1024 were measured (DESIGN.md 5.3.1): 512 is fastest, and at 1024
#define PCX_TALL_THREADS 512  // the static LDS (sh[MT]) no longer leaves a 1024 x 64 round its one median wave
#endif
constexpr int MT = PCX_TALL_THREADS;  // threads per round (a build constant of the tall unit)
constexpr int MN = 1024;              // max reporters
static_assert(MT >= 256 && MT <= 1024 && MT % 64 == 0, "the round text owns tiles and columns by tid < 256");
#else
constexpr int MT = 256;  // threads per round
constexpr int MN = 256;  // max reporters
#endif
constexpr int MEV = 64;  // max events
constexpr double M_PI_TOL = 1e-14;
constexpr int M_PI_MAXIT = 256, M_PI_PRESQUARE = 3, M_PI_SQUARE_EVERY = 32, M_PI_MAX_SQUARINGS = 8,
              M_PI_POLISH = 2;
constexpr double M_DBL_EPS = 2.220446049250313080847e-16;
constexpr double M_DBL_MIN = 2.2250738585072014e-308;

// numpy pairwise sum (SPEC pw_sum) of g(0..n-1), n <= 256: leaves of <= 128, halves rounded
// down to multiples of 8 (the right half of n > 242 splits once more)
template <class G>
__device__ double mpw_leaf(G g, int off, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; i++) r += g(off + i);
        return r;
    }
    double r[8];
    for (int k = 0; k < 8; k++) r[k] = g(off + k);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int k = 0; k < 8; k++) r[k] += g(off + i + k);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += g(off + i);
    return res;
}
template <class G>
__device__ double mpw_sub(G g, int off, int n) {  // n <= 256: the right half may split once more
    if (n <= 128) return mpw_leaf(g, off, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return mpw_leaf(g, off, n2) + mpw_leaf(g, off + n2, n - n2);
}
#if PCX_MEDIUM_TALL
// n <= 1024: the same recursion (pw_sum(left) + pw_sum(right)) to any depth, without recursion: the
// leaves in index order, each with its depth; two finished values of one depth are siblings and add
// into their parent.  At most five segments and five values are pending (n = 1023 splits four times:
// 519, 263, 135 on the right), packed off | n << 11 | depth << 22.
template <class G>
__device__ double mpw(G g, int n) {
    if (n <= 128) return mpw_leaf(g, 0, n);
    uint32_t seg[6];
    double val[6];
    uint32_t vdep = 0;  // the pending values' depths, four bits each
    int sp = 1, vp = 0;
    seg[0] = (uint32_t)n << 11;
    while (sp) {
        const uint32_t s = seg[--sp];
        const int off = s & 2047, m = (s >> 11) & 2047;
        int d = (int)(s >> 22);
        if (m > 128) {
            int h = m / 2;
            h -= h % 8;
            seg[sp++] = (uint32_t)(off + h) | (uint32_t)(m - h) << 11 | (uint32_t)(d + 1) << 22;
            seg[sp++] = (uint32_t)off | (uint32_t)h << 11 | (uint32_t)(d + 1) << 22;
            continue;
        }
        double v = mpw_leaf(g, off, m);
        while (vp && (int)((vdep >> (4 * (vp - 1))) & 15u) == d) {
            vp--;
            v = val[vp] + v;
            d--;
        }
        val[vp] = v;
        vdep = (vdep & ~(15u << (4 * vp))) | (uint32_t)d << (4 * vp);
        vp++;
    }
    return val[0];
}
#else
template <class G>
__device__ double mpw(G g, int n) {
    if (n <= 128) return mpw_leaf(g, 0, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return mpw_leaf(g, 0, n2) + mpw_sub(g, n2, n - n2);
}
#endif

// the same tree64 on wave 0 (lane = slot): the xor butterfly by shuffles; valid on lane 0
template <class G>
__device__ double wtree64(G g, int n) {
    const int l = threadIdx.x & 63;
    double v = l < n ? g(l) : 0.0;
    for (int s = 1; s <= 8; s <<= 1) v = v + __shfl_xor(v, s, 64);
    const double t16 = __shfl(v, 16, 64), t32 = __shfl(v, 32, 64), t48 = __shfl(v, 48, 64);
    return (v + t16) + (t32 + t48);
}

// the same tree64 on a register value per lane (0 beyond n); valid on lane 0
__device__ double wtree64v(double v) {
    for (int s = 1; s <= 8; s <<= 1) v = v + __shfl_xor(v, s, 64);
    const double t16 = __shfl(v, 16, 64), t32 = __shfl(v, 32, 64), t48 = __shfl(v, 48, 64);
    return (v + t16) + (t32 + t48);
}

// SPEC dot2 (compensated dot, index order)
template <class A, class B>
__device__ double mdot2(A a, B b, int n) {
    double s = 0.0, c = 0.0;
    auto step = [&](double x, double y) {
        const double p = x * y;
        const double pe = fma(x, y, -p);
        const double t = s + p;
        const double z = t - s;
        const double se = (s - (t - z)) + (p - z);
        s = t;
        c = c + (pe + se);
    };
    int i = 0;
    for (; i + 8 <= n; i += 8) {  // in index order, loads eight ahead
        double xa[8], ya[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            xa[q] = a(i + q);
            ya[q] = b(i + q);
        }
#pragma unroll
        for (int q = 0; q < 8; q++) step(xa[q], ya[q]);
    }
    for (; i < n; i++) step(a(i), b(i));
    return s + c;
}

// np.dot(v, F)[j] in OpenBLAS's order (SPEC ob_vecmat)
template <class V, class X>
__device__ double mob_vecmat(V v, X F, int N, int E, int j) {
    if (E == 1) {  // numpy's ddot
        double acc8[4][8], acc4[4][4];
        for (int r = 0; r < 4; r++)
            for (int l = 0; l < 8; l++) acc8[r][l] = 0.0;
        const int n32 = N & -32, n16 = N & -16;
        for (int i = 0; i < n32; i += 32)
            for (int k = 0; k < 32; k++) acc8[k / 8][k % 8] = fma(v(i + k), F(i + k), acc8[k / 8][k % 8]);
        for (int r = 0; r < 4; r++)
            for (int l = 0; l < 4; l++) acc4[r][l] = acc8[r][l] + acc8[r][l + 4];
        for (int i = n32; i < n16; i += 16)
            for (int k = 0; k < 16; k++) acc4[k / 4][k % 4] = fma(v(i + k), F(i + k), acc4[k / 4][k % 4]);
        double A[4];
        for (int l = 0; l < 4; l++) A[l] = ((acc4[0][l] + acc4[1][l]) + acc4[2][l]) + acc4[3][l];
        double d = (A[0] + A[2]) + (A[1] + A[3]);
        for (int i = n16; i < N; i++) d = fma(v(i), F(i), d);
        return d;
    }
    if (j < (E & ~3)) {
        double y = 0.0;
        int n = 0;
        for (; n + 8 <= N; n += 8) {  // two blocks of four rows, loads ahead of the adds
            double f[8], w[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                f[q] = F(n + q);
                w[q] = v(n + q);
            }
            double t0 = f[1] * w[1];
            t0 = fma(f[0], w[0], t0);
            t0 = fma(f[2], w[2], t0);
            t0 = fma(f[3], w[3], t0);
            double t1 = f[5] * w[5];
            t1 = fma(f[4], w[4], t1);
            t1 = fma(f[6], w[6], t1);
            t1 = fma(f[7], w[7], t1);
            y = y + t0;
            y = y + t1;
        }
        for (; n + 4 <= N; n += 4) {
            double t = F(n + 1) * v(n + 1);
            t = fma(F(n), v(n), t);
            t = fma(F(n + 2), v(n + 2), t);
            t = fma(F(n + 3), v(n + 3), t);
            y = y + t;
        }
        if (n + 2 <= N) {
            double t = F(n + 1) * v(n + 1);
            t = fma(F(n), v(n), t);
            y = y + t;
            n += 2;
        }
        if (n < N) y = y + F(n) * v(n);
        return y;
    }
    double t = 0.0;
    int i = 0;
    if (E == 2 || E == 3)
        for (; i + 4 <= N; i += 4) {
            t = t + fma(F(i), v(i), F(i + 1) * v(i + 1));
            t = t + fma(F(i + 2), v(i + 2), F(i + 3) * v(i + 3));
        }
    for (; i < N; i++) t = fma(F(i), v(i), t);
    return t;
}

// out[j] = np.dot(v, F)[j] for every column (block call, all threads): OpenBLAS's four-row
// block partials of the columns j < E & ~3 in parallel into tb ((N / 4) x (E & ~3) doubles),
// then each column's sequential sum of its partials and the row tail; the other columns (and
// E == 1) by mob_vecmat on their thread over a copy staged in LDS after the partials
// ((E - E & ~3) x N doubles).  The caller syncs before reading out.
template <class V>
__device__ void bvecmat(V v, const double* F, int N, int E, double* out, double* tb);

__device__ __forceinline__ double mcatch(double x, double tol) {
    if (x < 1.5 - tol) return 1.0;
    if (x > 1.5 + tol) return 2.0;
    return 1.5;
}

#if PCX_MEDIUM_TALL
// tall rounds: the block partials in chunks of `nbc` four-row blocks (the plan's: tb holds nbc x E4
// partials, then the staged tail columns).  Column j's chain y = y + t stays on thread j across the
// chunks, in block order -- the order of additions is bvecmat's.
template <class V>
__device__ void bvecmat_chunked(V v, const double* F, int N, int E, double* out, double* tb, int nbc) {
    const int E4 = E == 1 ? 0 : (E & ~3), nb = N >> 2, tid = threadIdx.x;
    double* tl = tb + nbc * E4;  // the columns past E & ~3 staged from F (their chains read LDS)
    const int nt = (E - E4) * N;
    for (int idx = tid; idx < nt; idx += MT) tl[idx] = F[(idx % N) * E + E4 + idx / N];
    double y = 0.0;
    for (int b0 = 0; b0 < nb && E4; b0 += nbc) {
        const int cb = nb - b0 < nbc ? nb - b0 : nbc, ni = cb * E4;
        for (int idx = tid; idx < ni; idx += MT) {
            const int j = idx % E4, n = 4 * (b0 + idx / E4);
            double f[4], w[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                f[r] = F[(n + r) * E + j];
                w[r] = v(n + r);
            }
            double t = f[1] * w[1];
            t = fma(f[0], w[0], t);
            t = fma(f[2], w[2], t);
            t = fma(f[3], w[3], t);
            tb[idx] = t;
        }
        __syncthreads();
        if (tid < E4) {  // y = y + t, block order, loads eight ahead
            int b = 0;
            for (; b + 8 <= cb; b += 8) {
                double t8[8];
#pragma unroll
                for (int q = 0; q < 8; q++) t8[q] = tb[(b + q) * E4 + tid];
#pragma unroll
                for (int q = 0; q < 8; q++) y += t8[q];
            }
            for (; b < cb; b++) y += tb[b * E4 + tid];
        }
        __syncthreads();  // (the next chunk overwrites tb; with E4 == 0 the barrier below orders tl)
    }
    if (!E4 || !nb) __syncthreads();
    if (tid < E) {  // (E <= 64 <= MT: one column per thread)
        const int j = tid;
        if (j >= E4) {
            const double* col = tl + (j - E4) * N;
            out[j] = mob_vecmat(v, [&](int i) { return col[i]; }, N, E, j);
        } else {
            int n = 4 * nb;
            if (n + 2 <= N) {
                double t = F[(n + 1) * E + j] * v(n + 1);
                t = fma(F[n * E + j], v(n), t);
                y = y + t;
                n += 2;
            }
            if (n < N) y = y + F[n * E + j] * v(n);
            out[j] = y;
        }
    }
}
#endif

template <class V>
__device__ void bvecmat(V v, const double* F, int N, int E, double* out, double* tb) {
    const int E4 = E == 1 ? 0 : (E & ~3), nb = N >> 2, ni = nb * E4;
    for (int i0 = threadIdx.x; i0 < ni; i0 += 4 * MT) {  // four blocks' loads per round trip
        double f[4][4], w[4][4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = i0 + u * MT;
            const int j = idx % E4, n = 4 * (idx / E4);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                f[u][r] = idx < ni ? F[(n + r) * E + j] : 0.0;
                w[u][r] = idx < ni ? v(n + r) : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int idx = i0 + u * MT;
            double t = f[u][1] * w[u][1];
            t = fma(f[u][0], w[u][0], t);
            t = fma(f[u][2], w[u][2], t);
            t = fma(f[u][3], w[u][3], t);
            if (idx < ni) tb[idx] = t;
        }
    }
    double* tl = tb + ni;  // the columns past E & ~3 staged from F (their chains read LDS)
    const int nt = (E - E4) * N;
    for (int idx = threadIdx.x; idx < nt; idx += MT) tl[idx] = F[(idx % N) * E + E4 + idx / N];
    __syncthreads();
    for (int j = threadIdx.x; j < E; j += MT) {
        if (j >= E4) {
            const double* col = tl + (j - E4) * N;
            out[j] = mob_vecmat(v, [&](int i) { return col[i]; }, N, E, j);
            continue;
        }
        double y = mseq([&](int b) { return tb[b * E4 + j]; }, nb);  // y = y + t, block order
        int n = 4 * nb;
        if (n + 2 <= N) {
            double t = F[(n + 1) * E + j] * v(n + 1);
            t = fma(F[n * E + j], v(n), t);
            y = y + t;
            n += 2;
        }
        if (n < N) y = y + F[n * E + j] * v(n);
        out[j] = y;
    }
}

// block reductions (max of doubles / first index)
// (max-norms of non-negative values: exact in any order)
__device__ double bmax(double v, double* sh) {
    for (int s = 1; s < 64; s <<= 1) v = fmax(v, __shfl_xor(v, s, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < MT / 64; w++) r = fmax(r, sh[w]);
    __syncthreads();
    return r;
}

// one wave's LDS writes visible to its other lanes (LDS operations of a wave execute in issue
// order: a compiler-ordering wave barrier, no lgkmcnt drain)
__device__ __forceinline__ void mwsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// broadcast from a wave-uniform lane (v_readlane into SGPRs)
__device__ __forceinline__ double mbcast(double v, int src) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// sequential sum g(0) + g(1) + ... in index order (Python's builtin sum), the loads issued
// eight at a time ahead of the dependent adds
template <class G>
__device__ double mseq(G g, int n) {
    double s = 0.0;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = g(i + q);
#pragma unroll
        for (int q = 0; q < 8; q++) s += v[q];
    }
    for (; i < n; i++) s += g(i);
    return s;
}

// weightedstats.weighted_median (SPEC wmedian) of n <= 256 (x, w) pairs in LDS on ONE wave:
// lane 0's sequential total and walk (loads batched by eight), the stable (x, w) order by a
// bitonic network over the lanes in LDS (the SPEC's rank placement when a NaN is present); sb is
// this wave's sort scratch of PN doubles x, PN doubles w and PN ints (PN = pow2 >= n); the result
// on every lane of the wave
__device__ double wv_wmedian(const double* x, const double* w, int n, double* sb, int PN,
                             long long* prof = nullptr) {
    const int lane = threadIdx.x & 63;
    double* xs = sb;
    double* ws = sb + PN;
    long long t0 = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
    const double W = mseq([&](int i) { return w[i]; }, n);  // every lane alike (broadcast loads)
    const double mid = 0.5 * W;
    bool dom = false, pos = false, nan_ = false;
    for (int i = lane; i < n; i += 64) {
        dom |= w[i] > mid;
        pos |= w[i] > 0;
        nan_ |= __builtin_isnan(x[i]) || __builtin_isnan(w[i]);
    }
    const bool anydom = __ballot(dom) != 0, anypos = __ballot(pos) != 0;
    double r = __builtin_nan("");
    if (anydom) {
        if (lane == 0) {
            double m = w[0];
            for (int i = 1; i < n; i++)
                if (w[i] > m) m = w[i];
            for (int i = 0; i < n; i++)
                if (w[i] == m) {
                    r = x[i];
                    break;
                }
        }
        return mbcast(r, 0);
    }
    if (!anypos) return r;
    if (prof) {
        const long long t = (long long)__builtin_amdgcn_s_memtime();
        prof[0] += t - t0;
        t0 = t;
    }
    if (__ballot(nan_) == 0) {
        // the stable (x, w) order is the ascending order of (x, w, index) (x, w compared with
        // < and ==): a bitonic network over P = pow2 >= n slots in LDS, padding slots last
        int* id = (int*)(sb + 2 * PN);
        int P = 2;
        while (P < n) P <<= 1;
        for (int i = lane; i < P; i += 64) {
            const bool v = i < n;
            xs[i] = v ? x[i] : 0.0;
            ws[i] = v ? w[i] : 0.0;
            id[i] = v ? i : -1;
        }
        mwsync();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                    const int ia = id[i], il = id[l];
                    const double xa = xs[i], wa = ws[i], xl = xs[l], wl = ws[l];
                    bool gt;  // (x, w, id) at i after the one at l; padding after everything
                    if (ia < 0 || il < 0)
                        gt = ia < 0 && il >= 0;
                    else
                        gt = (xl < xa) || (xl == xa && (wl < wa || (wl == wa && il < ia)));
                    if (gt == ((i & k) == 0)) {
                        xs[i] = xl;
                        xs[l] = xa;
                        ws[i] = wl;
                        ws[l] = wa;
                        id[i] = il;
                        id[l] = ia;
                    }
                }
                mwsync();
            }
    } else {
        // stable rank by (x, w) as the SPEC places it: this lane's elements i = lane + 64 q in
        // registers, the compared elements m read eight at a time (LDS broadcasts)
#if PCX_MEDIUM_TALL
        // (n <= 1024: the lane's sixteen elements four at a time, each four against every m)
        for (int q0 = 0; q0 < ((n + 63) >> 6); q0 += 4) {
        const int nq = ((n + 63) >> 6) - q0, l0 = lane + 64 * q0;
#else
        const int nq = (n + 63) >> 6, l0 = lane;
#endif
        double xi[4], wi[4];
        int rk[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = l0 + 64 * q;
            xi[q] = i < n ? x[i] : 0.0;
            wi[q] = i < n ? w[i] : 0.0;
            rk[q] = 0;
        }
        // (numpy's sort order, the SPEC's: a NaN after every number, NaNs equal among themselves;
        // a total order, so the ranks are a permutation and every slot below n is written)
        auto cmp = [&](double xm, double wm, int m) {
            const bool xmn = __builtin_isnan(xm), wmn = __builtin_isnan(wm);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (q >= nq) break;  // wave-uniform
                const bool xin = __builtin_isnan(xi[q]), win = __builtin_isnan(wi[q]);
                const bool xlt = (xm < xi[q]) || (xin && !xmn), xeq = (xm == xi[q]) || (xin && xmn);
                const bool wlt = (wm < wi[q]) || (win && !wmn), weq = (wm == wi[q]) || (win && wmn);
                rk[q] += (xlt || (xeq && (wlt || (weq && m < l0 + 64 * q)))) ? 1 : 0;
            }
        };
        int m0 = 0;
        for (; m0 + 8 <= n; m0 += 8) {
            double xm[8], wm[8];
#pragma unroll
            for (int t = 0; t < 8; t++) {
                xm[t] = x[m0 + t];
                wm[t] = w[m0 + t];
            }
#pragma unroll
            for (int t = 0; t < 8; t++) cmp(xm[t], wm[t], m0 + t);
        }
        for (; m0 < n; m0++) cmp(x[m0], w[m0], m0);
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (l0 + 64 * q < n) {
                xs[rk[q]] = xi[q];
                ws[rk[q]] = wi[q];
            }
#if PCX_MEDIUM_TALL
        }
#endif
    }
    mwsync();
    if (prof) {
        const long long t = (long long)__builtin_amdgcn_s_memtime();
        prof[1] += t - t0;
        t0 = t;
    }
    {
        // the walk `while cum <= mid: cum += ws[k]; k += 1` on every lane alike (no divergence):
        // branch-free steps, eight loads ahead, leaving at the first batch past the crossing
        double cum = 0.0;
        int k = 0;
        bool stop = !(cum <= mid);
        for (int i = 0; i < n && !stop; i += 8) {
            const int lim = n - i < 8 ? n - i : 8;
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = q < lim ? ws[i + q] : 0.0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const bool go = !stop && q < lim;
                const double c2 = cum + v[q];
                cum = go ? c2 : cum;
                k += go ? 1 : 0;
                stop = stop || (go && !(cum <= mid));
            }
        }
        const bool fail = !stop;  // ran past the end with cum <= mid
        if (!fail) {
            const double before = cum - ws[k - 1];
            if (fabs(before - mid) < M_DBL_EPS) {
                if (k >= 2) r = (xs[k - 2] + xs[k - 1]) / 2.0;
                else if (n == 1) r = xs[0] / 1.0;
            } else {
                r = xs[k - 1];
            }
        }
    }
    r = mbcast(r, 0);
    mwsync();  // xs / ws free for the wave's next use
    if (prof) prof[2] += (long long)__builtin_amdgcn_s_memtime() - t0;
    return r;
}

// "big-five" / "fixed-variance" (:373-390, :429-451), SPEC component_scores: eigenpairs of C by
// cyclic two-sided Jacobi with the round-robin pair schedule (every step's pairs disjoint: one
// thread per pair for the angles, per (pair, index) for the rotations, rows then columns), Sigma
// descending (ties by index), net_i = sum_c Sigma_c (wcd_i . loading_c) over the components.
// A = M, V = Tm (LDS, stride ES); returns the fixed-variance count, else -1.
constexpr int M_JAC_MAXSWEEP = 30;
constexpr double M_JAC_TOL = 1e-15;

__device__ __forceinline__ void mjac_pair(int i, int r, int n, int& p, int& q) {
    const int a = i == 0 ? 0 : 1 + (i - 1 + r) % (n - 1);
    const int b = 1 + (n - 2 - i + r) % (n - 1);
    p = a < b ? a : b;
    q = a < b ? b : a;
}

__device__ int component_scores(const BatchArgs& a, const double* C, double* A, double* V, int ES, const double* F,
                                const double* mu, double* net, double* sh, double* scal) {
    const int E = a.E, N = a.N, tid = threadIdx.x;
    __shared__ double cc[MEV / 2 + 1], ss[MEV / 2 + 1];
    __shared__ int pp[MEV / 2 + 1], qq[MEV / 2 + 1];
    __shared__ int order[MEV];
    __shared__ double sig[MEV];
    for (int e = tid; e < E * E; e += MT) {
        const int j = e / E, k = e % E;
        A[j * ES + k] = C[e];
        V[j * ES + k] = j == k ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid == 0) scal[0] = mpw([&](int j) { return C[j * E + j]; }, E);  // np.trace: add.reduce
    if (E >= 2) {
        const int n = E + (E & 1), npair = n / 2;
        for (int sweep = 0; sweep < M_JAC_MAXSWEEP; sweep++) {
            double off = 0.0, dg = 0.0;  // max-norms: exact in any order
            for (int e = tid; e < E * E; e += MT) {
                const int j = e / E, k = e % E;
                const double v = fabs(A[j * ES + k]);
                if (j == k) dg = fmax(dg, v);
                else off = fmax(off, v);
            }
            off = bmax(off, sh);
            dg = bmax(dg, sh);
            if (!(off > M_JAC_TOL * dg)) break;  // block-uniform
            for (int r = 0; r < n - 1; r++) {
                for (int i = tid; i < npair; i += MT) {
                    int p, q;
                    mjac_pair(i, r, n, p, q);
                    pp[i] = p;
                    qq[i] = q;
                    double c = 1.0, sn = 0.0;
                    if (q < E) {
                        const double app = A[p * ES + p], aqq = A[q * ES + q], apq = A[p * ES + q];
                        if (apq != 0.0) {
                            const double tau = (aqq - app) / (2.0 * apq);
                            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                            c = 1.0 / sqrt(1.0 + t * t);
                            sn = t * c;
                        }
                    }
                    cc[i] = c;
                    ss[i] = sn;
                }
                __syncthreads();
                for (int e = tid; e < npair * E; e += MT) {  // rows
                    const int i = e / E, k = e % E;
                    if (ss[i] == 0.0) continue;
                    const int p = pp[i], q = qq[i];
                    const double c = cc[i], sn = ss[i];
                    const double apk = A[p * ES + k], aqk = A[q * ES + k];
                    A[p * ES + k] = c * apk - sn * aqk;
                    A[q * ES + k] = sn * apk + c * aqk;
                }
                __syncthreads();
                for (int e = tid; e < npair * E; e += MT) {  // columns of A and V
                    const int i = e / E, j = e % E;
                    if (ss[i] == 0.0) continue;
                    const int p = pp[i], q = qq[i];
                    const double c = cc[i], sn = ss[i];
                    const double ajp = A[j * ES + p], ajq = A[j * ES + q];
                    A[j * ES + p] = c * ajp - sn * ajq;
                    A[j * ES + q] = sn * ajp + c * ajq;
                    const double vjp = V[j * ES + p], vjq = V[j * ES + q];
                    V[j * ES + p] = c * vjp - sn * vjq;
                    V[j * ES + q] = sn * vjp + c * vjq;
                }
                __syncthreads();
            }
        }
    }
    for (int j = tid; j < E; j += MT) sig[j] = fabs(A[j * ES + j]);
    __syncthreads();
    for (int j = tid; j < E; j += MT) {  // descending Sigma, ties by index
        int rk = 0;
        for (int k = 0; k < E; k++) rk += (sig[k] > sig[j]) || (sig[k] == sig[j] && k < j);
        order[rk] = j;
    }
    __syncthreads();
    const int kmax = a.algorithm == PCX_ALG_BIG_FIVE ? a.max_components : E;
    if (tid == 0) {  // fixed-variance: cumsum(Sigma / trace) >= threshold stops after that component
        int used = kmax;
        if (a.algorithm == PCX_ALG_FIXED_VARIANCE) {
            double ve = 0.0;
            for (int c = 0; c < kmax; c++) {
                ve = ve + sig[order[c]] / scal[0];
                if (ve >= a.variance_threshold) {
                    used = c + 1;
                    break;
                }
            }
        }
        scal[1] = (double)used;
    }
    __syncthreads();
    const int used = (int)scal[1];
    for (int i = tid; i < N; i += MT) {
        double acc = 0.0;
        for (int c = 0; c < used; c++) {
            const int idx = order[c];
            const double sg = sig[idx];
            const double fl = V[idx] < 0.0 ? -1.0 : 1.0;  // loading *= -1 if loading[0] < 0
            double d = 0.0;
            for (int j = 0; j < E; j++) d = fma(F[i * E + j] - mu[j], fl * V[j * ES + idx], d);
            acc = acc + sg * d;
        }
        net[i] = acc;
    }
    __syncthreads();
    return a.algorithm == PCX_ALG_FIXED_VARIANCE ? used : -1;
}

// ---- clustering algorithms (SPEC hier_nc / feck_nc / kmeans_nc), the CLUS instantiation only ----
// Each turns the filled reports into the nonconformity vector nc (LDS, one row per thread:
// N <= MT).  L is the LDS work region (medium_region doubles); X is this round's N x E global
// scratch, laid out event-major ([k][i]) so that a thread per row or per cluster reads it
// coalesced.
constexpr int M_KMAX = 16;          // k-means code books: ceil(sqrt(256))
constexpr int M_KMEANS_MAXIT = 4096;  // Lloyd steps per restart (the SPEC's guard)
#if !PCX_MEDIUM_TALL  // (the tall unit takes no clustering: they are one thread per row by design)
static_assert(MT >= MN, "one thread per reporter row");

// first thread of the smallest key among the candidate threads (block call; -1: none), the key
// through *kmin.  shd / shi: MT / 64 slots each, free again after the caller's next barrier.
__device__ int bfirstmin(bool cand, double key, double* shd, int* shi, double* kmin) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double v = cand ? key : __builtin_inf();
    double m = v;
    for (int s = 1; s < 64; s <<= 1) m = fmin(m, __shfl_xor(m, s, 64));
    const unsigned long long at = __ballot(cand && v == m);
    if (lane == 0) {
        shd[wv] = m;
        shi[wv] = at ? wv * 64 + __builtin_ctzll(at) : -1;
    }
    __syncthreads();
    int bi = -1;
    double bm = __builtin_inf();
    for (int w = 0; w < MT / 64; w++)
        if (shi[w] >= 0 && (bi < 0 || shd[w] < bm)) {
            bm = shd[w];
            bi = shi[w];
        }
    *kmin = bm;
    return bi;
}

// SPEC nc_from_sizes: (size - min size) / sum, the integer sum exact, equal sizes 0/0 = NaN
__device__ void mnc_from_sizes(int size, int N, double* nc, int* red) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        red[0] = 0x7fffffff;
        red[1] = 0;
    }
    __syncthreads();
    if (tid < N) atomicMin(&red[0], size);
    __syncthreads();
    const int mn = red[0];
    if (tid < N) atomicAdd(&red[1], size - mn);
    __syncthreads();
    if (tid < N) nc[tid] = (double)(size - mn) / (double)red[1];
    __syncthreads();
}

// hierarchical: the connected components of {sqrt(d2_ij) <= t}, d2_ij the sequential sum of the
// squared wcd differences; thread i owns row i's adjacency mask, labels settle by min-label
// propagation with one pointer jump per sweep
__device__ __noinline__ void mhier_nc(const double* F, const double* mu, int N, int E, double t, double* X, double* L,
                                      double* nc) {
    const int tid = threadIdx.x;
    for (int e = tid; e < N * E; e += MT) X[(e % E) * N + e / E] = F[e] - mu[e % E];
    unsigned long long* adj = (unsigned long long*)L;  // [N][4]
    int* lab = (int*)(L + 4 * N);                      // [N]
    int* cnt = lab + N;                                // [N]
    int* red = cnt + N;                                // [2]
    __syncthreads();
    const bool row = tid < N;
    if (row) {
#pragma unroll
        for (int w = 0; w < MN / 64; w++) {
            unsigned long long mw = 0;
            const int jend = N < 64 * w + 64 ? N : 64 * w + 64;
            for (int j0 = 64 * w; j0 < jend; j0 += 4) {
                double d2[4] = {0.0, 0.0, 0.0, 0.0};
                int jj[4];
#pragma unroll
                for (int q = 0; q < 4; q++) jj[q] = j0 + q < N ? j0 + q : N - 1;
                for (int k = 0; k < E; k++) {
                    const double di = X[k * N + tid];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const double df = di - X[k * N + jj[q]];
                        d2[q] = d2[q] + df * df;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (j0 + q < N && j0 + q != tid && sqrt(d2[q]) <= t) mw |= 1ull << (j0 + q - 64 * w);
            }
            adj[tid * 4 + w] = mw;
        }
        lab[tid] = tid;
        cnt[tid] = 0;
    }
    __syncthreads();
    for (;;) {
        int nl = 0;
        bool changed = false;
        if (row) {
            const int old = lab[tid];
            nl = old;
            for (int w = 0; w < MN / 64; w++) {
                unsigned long long m = adj[tid * 4 + w];
                while (m) {
                    const int j = 64 * w + __builtin_ctzll(m);
                    m &= m - 1;
                    const int lj = lab[j];
                    nl = lj < nl ? lj : nl;
                }
            }
            const int lj = lab[nl];
            nl = lj < nl ? lj : nl;
            changed = nl != old;
        }
        __syncthreads();
        if (row) lab[tid] = nl;
        if (!__syncthreads_or(changed)) break;
    }
    if (row) atomicAdd(&cnt[lab[tid]], 1);
    __syncthreads();
    mnc_from_sizes(row ? cnt[lab[tid]] : 0, N, nc, red);
}

// clusterfeck's running clusters: thread x = cluster x
struct MFeck {
    double* sumT;   // [E][N] (global) sum(vec * repVec, axis=0), running in member order
    double* meanT;  // [E][N] (global) SPEC feck_mean: the founding row of a singleton, else sumT / crep --
                    // kept current as a cluster changes (one per row), so the distances divide nothing
    double* crep;   // [N] running member weight
    double* dx;     // [N] per-cluster distance to the mode
    int* of;        // [N] cluster of each row, -1 = none
    const int* rnan;  // [N] the row holds a NaN
    const double* w;  // [N] member weights
    const double* F;
    int N, E;
};

// one cluster() pass (SPEC feck_pass + feck_rowdist): rows in order, the existing clusters'
// distances in parallel (numpy pairwise sums), first minimum; dm = the rows' distances for this
// pass's mode; returns the mode's distance to outc (every thread alike)
__device__ __noinline__ double mfeck_pass(const MFeck& f, double thr, const double* outc, double* mm, double* dm,
                                          double* shd, int* shi) {
    const int tid = threadIdx.x, N = f.N, E = f.E;
    // (no cluster at all: every row holds a NaN; the mode's mean stays defined)
    if (tid < E) f.meanT[tid * N] = f.F[tid];
    if (tid == 0) f.crep[0] = 0.0;
    __syncthreads();
    int ncl = 0;
    for (int i = 0; i < N; i++) {
        const double* Fi = f.F + i * E;
        const bool valid = tid < ncl;
        double d = 0.0;
        if (valid) d = sqrt(mpw([&](int k) { const double t = Fi[k] - f.meanT[k * N + tid]; return t * t; }, E));
        double dmin;
        const int bx = bfirstmin(valid && d < 0x1p255, d, shd, shi, &dmin);
        const double wi = f.w[i];
        if (bx >= 0 && dmin < thr) {
            if (tid < 64) {  // wave 0 (E <= 64): every lane reads the weight before lane 0 updates it
                const double nr = f.crep[bx] + wi;
                mwsync();
                if (tid < E) {
                    const double sm = f.sumT[tid * N + bx] + Fi[tid] * wi;
                    f.sumT[tid * N + bx] = sm;
                    f.meanT[tid * N + bx] = sm / nr;
                }
                if (tid == 0) {
                    f.crep[bx] = nr;
                    f.of[i] = bx;
                }
            }
        } else if (!f.rnan[i]) {
            const int x = ncl++;
            if (tid < E) {
                f.sumT[tid * N + x] = Fi[tid] * wi;
                f.meanT[tid * N + x] = Fi[tid];
            }
            if (tid == 0) {
                f.crep[x] = wi;
                f.of[i] = x;
            }
        } else if (tid == 0) {
            f.of[i] = -1;
        }
        __syncthreads();
    }
    const bool valid = tid < ncl;
    const double r = valid ? f.crep[tid] : 0.0;
    double top;
    int mode = bfirstmin(valid && r > 0.0, -r, shd, shi, &top);  // first cluster of largest weight
    if (mode < 0) mode = 0;
    if (tid < E) mm[tid] = f.meanT[tid * N + mode];
    __syncthreads();
    if (valid) f.dx[tid] = sqrt(mpw([&](int k) { const double t = mm[k] - f.meanT[k * N + tid]; return t * t; }, E));
    const double dmode = sqrt(mpw([&](int k) { const double t = mm[k] - outc[k]; return t * t; }, E));
    __syncthreads();
    if (tid < N) {
        const int o = f.of[tid];
        dm[tid] = o >= 0 ? f.dx[o] : 0.0;
    }
    __syncthreads();
    return dmode;
}

__device__ __noinline__ void mfeck_nc(const BatchArgs& a, const double* F, const double* tok, int N, int E, double* X,
                                      double* L, double* nc, double* scal) {
    const int tid = threadIdx.x;
    MFeck f;
    f.sumT = X;
    f.meanT = X + N * E;
    f.crep = L;
    f.dx = L + N;
    double* w = L + 2 * N;
    double* dm1 = L + 3 * N;
    double* dm2 = L + 4 * N;
    double* outc = L + 5 * N;
    double* mm = outc + E;
    double* shd = mm + E;  // [4]
    f.of = (int*)(shd + 4);
    int* rnan = f.of + N;
    int* shi = rnan + N;  // [4]
    f.rnan = rnan;
    f.w = w;
    f.F = F;
    f.N = N;
    f.E = E;
    if (tid < N) {
        w[tid] = tok[tid] == 0.0 ? 0.00001 : tok[tid];
        int nn = 0;
        for (int k = 0; k < E; k++) nn |= __builtin_isnan(F[tid * E + k]) ? 1 : 0;
        rnan[tid] = nn;
    }
    double thr = a.cluster_threshold;
    if (!(thr > 0.0)) {
        thr = log10((double)E) / 1.77;
        if (thr == 0.0) thr = 0.3;
    }
    __syncthreads();
    if (tid == 0) scal[0] = mpw([&](int i) { return w[i]; }, N);
    __syncthreads();
    if (tid < E) {  // outcomes = np.ma.average(features, axis=0, weights=rep)
        double num;
        if (E == 1) {
            num = mpw([&](int i) { return F[i * E + tid] * w[i]; }, N);
        } else {
            num = F[tid] * w[0];
            for (int i = 1; i < N; i++) num = num + F[i * E + tid] * w[i];
        }
        outc[tid] = num / scal[0];
    }
    __syncthreads();
    const double d1 = mfeck_pass(f, thr, outc, mm, dm1, shd, shi);
    const double* dm = dm1;
    if (d1 > 1.07) {  // a far mode re-clusters once with 3 x thr; the closer mode wins
        const double d2 = mfeck_pass(f, thr * 3, outc, mm, dm2, shd, shi);
        if (d2 < d1) dm = dm2;
    }
    if (tid == 0) {  // np.amax: NaN propagates
        double mx = dm[0];
        for (int i = 1; i < N; i++)
            if (__builtin_isnan(dm[i]) || dm[i] > mx) mx = __builtin_isnan(mx) ? mx : dm[i];
        scal[1] = mx;
    }
    __syncthreads();
    if (tid < N) w[tid] = fabs(1.0 - dm[tid] / (scal[1] + 0.00000001));  // (the weights are done)
    __syncthreads();
    if (tid == 0) {  // normalize
        const double S = mpw([&](int i) { return w[i]; }, N);
        scal[2] = S;
        scal[3] = S == 0 ? mpw([&](int i) { return w[i] + 1.0; }, N) : S;
    }
    __syncthreads();
    if (tid < N) nc[tid] = scal[2] == 0 ? (w[tid] + 1.0) / scal[3] : w[tid] / scal[3];
    __syncthreads();
}

// scipy _vq.vq distance^2 (SPEC vq_d2) of one observation x(k) against four codes at a time (c: the
// first one's row, stride E; rows past `nc` codes are clamped and their result unused): E < 5 the
// naive loop; else -2 x.c (one fma chain for E < 32, eight interleaved chains summed as a tree
// from 32) + |x|^2 + |c|^2.  The observation is read eight events ahead, once for the four codes.
template <class XG>
__device__ __forceinline__ void mvq_d2x4(XG x, const double* c, int nc, int E, double xs, const double* cs, double* d) {
    const double* cq[4];
#pragma unroll
    for (int q = 0; q < 4; q++) cq[q] = c + (q < nc ? q : nc - 1) * E;
    if (E < 32) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < E; k += 8) {
            double xv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) xv[u] = k + u < E ? x(k + u) : 0.0;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (k + u >= E) break;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (E < 5) {
                        const double t = xv[u] - cq[q][k + u];
                        acc[q] = acc[q] + t * t;
                    } else {
                        acc[q] = fma(xv[u], cq[q][k + u], acc[q]);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) d[q] = E < 5 ? acc[q] : (-2.0 * acc[q] + xs) + cs[q < nc ? q : nc - 1];
        return;
    }
    double a[4][8];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int u = 0; u < 8; u++) a[q][u] = 0.0;
    for (int k = 0; k < E; k += 8) {
        double xv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) xv[u] = k + u < E ? x(k + u) : 0.0;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (k + u >= E) break;
#pragma unroll
            for (int q = 0; q < 4; q++) a[q][u] = fma(xv[u], cq[q][k + u], a[q][u]);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const double dot = ((a[q][0] + a[q][1]) + (a[q][2] + a[q][3])) + ((a[q][4] + a[q][5]) + (a[q][6] + a[q][7]));
        d[q] = (-2.0 * dot + xs) + cs[q < nc ? q : nc - 1];
    }
}

// k-means (SPEC kmeans_nc): whiten(wcd) into X, scipy kmeans over the caller's restarts (best mean
// distortion, strict <), vq labels, cluster sizes.  Thread i = observation i in vq; threads take
// (code, event) pairs in the mean update, the member sums in row order.
__device__ __noinline__ void mkmeans_nc(const BatchArgs& a, int64_t b, const double* F, const double* mu, int N, int E,
                                        double* X, double* L, double* nc, double* scal) {
    const int tid = threadIdx.x;
    const bool row = tid < N;
    double* book = L;                  // [M_KMAX][E]
    double* best = book + M_KMAX * E;  // [M_KMAX][E]
    double* sd = best + M_KMAX * E;    // [E]
    double* csq = sd + E;              // [M_KMAX]
    double* dist = csq + M_KMAX;       // [N]
    int* lab = (int*)(dist + N);       // [N]
    int* cntc = lab + N;               // [M_KMAX]
    int* red = cntc + M_KMAX;          // [2]
    // np.std(wcd, axis=0): sequential column sums (pairwise when E == 1); 0 -> 1
    if (tid < E) {
        const int j = tid;
        double s, v;
        if (E == 1) {
            s = mpw([&](int i) { return F[i * E + j] - mu[j]; }, N);
        } else {
            s = 0.0;
            for (int i = 0; i < N; i++) s = s + (F[i * E + j] - mu[j]);
        }
        const double m = s / (double)N;
        if (E == 1) {
            v = mpw([&](int i) { const double d = (F[i * E + j] - mu[j]) - m; return d * d; }, N);
        } else {
            v = 0.0;
            for (int i = 0; i < N; i++) {
                const double d = (F[i * E + j] - mu[j]) - m;
                v = v + d * d;
            }
        }
        double sj = sqrt(v / (double)N);
        if (sj == 0.0) sj = 1.0;
        sd[j] = sj;
    }
    __syncthreads();
    for (int e = tid; e < N * E; e += MT) X[(e % E) * N + e / E] = (F[e] - mu[e % E]) / sd[e % E];
    __syncthreads();
    auto obs = [&](int k) { return X[k * N + tid]; };
    double xs = 0.0;
    if (row)
        for (int k = 0; k < E; k++) xs = xs + obs(k) * obs(k);
    // labels and distortions against `codes` (ncodes of them); the mean distortion in scal[0]
    auto vq = [&](const double* codes, int ncodes) {
        if (tid < ncodes) {
            double s = 0.0;
            for (int k = 0; k < E; k++) s = s + codes[tid * E + k] * codes[tid * E + k];
            csq[tid] = s;
        }
        __syncthreads();
        if (row) {
            int li = 0;
            double low = __builtin_inf();
            for (int c0 = 0; c0 < ncodes; c0 += 4) {  // in code order, first minimum
                double d[4];
                mvq_d2x4(obs, codes + c0 * E, ncodes - c0, E, xs, csq + c0, d);
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (c0 + q < ncodes && d[q] < low) {
                        low = d[q];
                        li = c0 + q;
                    }
            }
            lab[tid] = li;
            dist[tid] = low > 0 ? sqrt(low) : 0.0;
        }
        __syncthreads();
    };
    const int K = a.kmeans_k, RS = a.kmeans_restarts;
    const int32_t* init = a.kmeans_init + b * (int64_t)RS * K;
    double best_d = __builtin_inf();
    int best_n = 0;
    for (int r = 0; r < RS; r++) {
        for (int o = tid; o < K * E; o += MT) {
            const int c = o / E, k = o - c * E;
            const int r0 = init[r * K + c];
            book[o] = X[k * N + (r0 < 0 ? 0 : r0 >= N ? N - 1 : r0)];
        }
        int ncodes = K;
        double prev0 = __builtin_inf(), prev1 = __builtin_inf();
        for (int it = 0;; it++) {
            __syncthreads();
            vq(book, ncodes);
            if (tid == 0) scal[0] = mpw([&](int i) { return dist[i]; }, N) / (double)N;
            if (tid < ncodes) {
                int n = 0;
                for (int i = 0; i < N; i++) n += lab[i] == tid;
                cntc[tid] = n;
            }
            __syncthreads();
            prev0 = prev1;
            prev1 = scal[0];
            // update_cluster_means: member sums in row order, / count; empty codes dropped
            unsigned nonempty = 0;
            for (int c = 0; c < ncodes; c++) nonempty |= cntc[c] > 0 ? 1u << c : 0u;
            double nv[M_KMAX * MEV / MT];
            int nk[M_KMAX * MEV / MT];
#pragma unroll
            for (int q = 0; q < M_KMAX * MEV / MT; q++) {
                const int p = tid + MT * q;
                nk[q] = -1;
                nv[q] = 0.0;
                if (p < ncodes * E) {
                    const int c = p / E, k = p - c * E;
                    const int n = cntc[c];
                    if (n > 0) {
                        double sm = 0.0;
                        for (int i = 0; i < N; i += 8) {  // in row order, loads eight ahead
                            double xv[8];
                            int lb[8];
#pragma unroll
                            for (int u = 0; u < 8; u++) {
                                const int iu = i + u < N ? i + u : N - 1;
                                xv[u] = X[k * N + iu];
                                lb[u] = i + u < N ? lab[iu] : -1;
                            }
#pragma unroll
                            for (int u = 0; u < 8; u++)
                                if (lb[u] == c) sm = sm + xv[u];
                        }
                        nv[q] = sm / (double)n;
                        nk[q] = __popc(nonempty & ((1u << c) - 1u)) * E + k;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < M_KMAX * MEV / MT; q++)
                if (nk[q] >= 0) book[nk[q]] = nv[q];
            ncodes = __popc(nonempty);
            if (!(fabs(prev0 - prev1) > 1e-5) || it + 1 >= M_KMEANS_MAXIT) break;
        }
        __syncthreads();
        if (prev1 < best_d) {  // block-uniform
            best_d = prev1;
            best_n = ncodes;
            for (int o = tid; o < ncodes * E; o += MT) best[o] = book[o];
        }
    }
    __syncthreads();
    if (best_n == 0) {  // no restart with a finite distortion: the reference raises
        if (row) nc[tid] = __builtin_nan("");
        __syncthreads();
        return;
    }
    vq(best, best_n);
    if (tid < best_n) {
        int n = 0;
        for (int i = 0; i < N; i++) n += lab[i] == tid;
        cntc[tid] = n;
    }
    __syncthreads();
    mnc_from_sizes(row ? cntc[lab[tid]] : 0, N, nc, red);
}
#endif  // !PCX_MEDIUM_TALL

// doubles of a round's clustering scratch: wcd / the whitened observations; clusterfeck's sums and means
__host__ __device__ __forceinline__ int medium_xscratch(int N, int E, int alg) {
    return alg == PCX_ALG_CLUSTERFECK ? 2 * N * E : alg >= PCX_ALG_KMEANS ? N * E : 0;
}
// doubles of the clusterings' LDS region (the carvings of mhier_nc / mfeck_nc / mkmeans_nc)
__host__ __device__ __forceinline__ int medium_clus(int N, int E, int alg) {
    if (alg == PCX_ALG_HIERARCHICAL) return 5 * N + 2;
    if (alg == PCX_ALG_CLUSTERFECK) return 6 * N + 2 * E + 8;
    if (alg == PCX_ALG_KMEANS) return 2 * M_KMAX * E + E + 2 * M_KMAX + 2 * N + 12;
    return 0;
}

// N-vectors (each N doubles)
enum { VN_REP = 0, VN_TOK, VN_S, VN_SET1, VN_SET2, VN_NW1, VN_NW2, VN_U, VN_THIS, VN_SMOOTH, VN_XS, VN_COUNT };
// E-vectors (each E doubles)
enum { VE_MU = 0, VE_OLD, VE_LD, VE_X, VE_Y, VE_SQ, VE_D1, VE_D2, VE_NEW1, VE_NEW2, VE_R0, VE_R1, VE_R2, VE_E1, VE_E2,
       VE_RAW, VE_ADJ, VE_FIN, VE_CERT, VE_REWARD, VE_PC, VE_RELC, VE_COUNT };
// doubles of the work region: M (E x (E+1); and Tm for the Jacobi algorithms), or per wave two N-vectors (median
// operands) and the sort scratch (PN doubles x, PN doubles w, PN ints; PN = pow2 >= N), or the
// vector-matrix block partials, or the covariance's staged rows
__host__ __device__ __forceinline__ int medium_pow2(int N) {
    int p = 2;
    while (p < N) p <<= 1;
    return p;
}
__host__ __device__ __forceinline__ int medium_wave_stride(int N) {
    const int pn = medium_pow2(N);
    return 2 * N + 2 * pn + pn / 2;
}
__host__ __device__ __forceinline__ int medium_work(int N, int E, int alg) {
    const bool jac = alg == PCX_ALG_BIG_FIVE || alg == PCX_ALG_FIXED_VARIANCE;  // Tm: the eigenvectors
    const int E4 = E == 1 ? 0 : (E & ~3);
    const int mt = (jac ? 2 : 1) * E * (E + 1), wq = (MT / 64) * medium_wave_stride(N),
              vb = (N >> 2) * E4 + (E - E4) * N;
    const int m = mt > wq ? mt : wq;
    return m > vb ? m : vb;  // and bvecmat's block partials
}
// the work region with the clusterings' carvings (the other algorithms: medium_work)
__host__ __device__ __forceinline__ int medium_region(int N, int E, int alg) {
    const int w = medium_work(N, E, alg), c = medium_clus(N, E, alg);
    return w > c ? w : c;
}

#if PCX_MEDIUM_TALL
// The LDS plan of one tall round (256 < N <= 1024 reporters; DESIGN.md 5.3.1): a function of the
// shape and the algorithm, used alike by the kernel, the launcher and pcx_tall_plan.  The vectors
// and the flag words are fixed; what is left of the 160 KB a workgroup may use, after the kernel's
// static LDS, is the work region.  It must hold M (and the Jacobi algorithms' second matrix), one
// wave's median operands and sort scratch, and the staged np.dot tail columns beside one row of
// block partials: else the shape does not fit (waves = 0) and stays on the round scheduler.  Within
// that the plan takes as many median / certainty waves as fit (4, 2 or 1) and the np.dot block
// partials in chunks of as many four-row blocks as fit; the region is the largest of the three.
struct TallPlan {
    int waves;   // concurrent median / certainty waves (0: the shape does not fit)
    int nbc;     // four-row blocks per np.dot chunk
    int chunks;  // np.dot chunks (the last one may be shorter)
    int region;  // doubles of the work region
};
constexpr int TALL_LDS_LIMIT = 160 * 1024;
// tall_round_kernel's static LDS (sh[MT], the scalars, the scaled-event list, component_scores'
// tables), rounded up; pcx_tall.hip checks it against the code object's figure at the first launch
constexpr int TALL_STATIC_LDS = 8 * MT + 2560;
__host__ __device__ __forceinline__ int tall_fixed_bytes(int N, int E) {
    return (VN_COUNT * N + VE_COUNT * E) * (int)sizeof(double) + ((N * E + 15) >> 4) * 4 + 16;
}
__host__ __device__ inline TallPlan tall_plan(int N, int E, int alg) {
    TallPlan p = {0, 0, 0, 0};
    if (N < 1 || N > MN || E < 1 || E > MEV || alg < PCX_ALG_PCA || alg > PCX_ALG_COKURTOSIS) return p;
    const bool jac = alg == PCX_ALG_BIG_FIVE || alg == PCX_ALG_FIXED_VARIANCE;
    const int E4 = E == 1 ? 0 : (E & ~3), nb = N >> 2, tail = (E - E4) * N;
    const int mt = (jac ? 2 : 1) * E * (E + 1), stride = medium_wave_stride(N);
    const int room = TALL_LDS_LIMIT - TALL_STATIC_LDS - tall_fixed_bytes(N, E);
    const int avail = room > 0 ? room / (int)sizeof(double) : 0;
    if (avail < mt || avail < stride || avail < tail + E4) return p;
    const int maxw = MT / 64 < 4 ? MT / 64 : 4;
    p.waves = maxw * stride <= avail ? maxw : 2 * stride <= avail ? 2 : 1;
    const int fitb = E4 ? (avail - tail) / E4 : nb;
    p.nbc = nb < 1 ? 1 : (fitb < nb ? fitb : nb);
    p.chunks = E4 && nb ? (nb + p.nbc - 1) / p.nbc : 1;
    const int wq = p.waves * stride, vb = p.nbc * E4 + tail;
    const int m = mt > wq ? mt : wq;
    p.region = m > vb ? m : vb;
    return p;
}
#endif

// diagnostic phase stamps (PCX_STAMPS=1): shader-clock reads at phase boundaries
#define MSTAMP(k)                                                                 \
    do {                                                                          \
        if (a.stamps) {                                                           \
            const long long t_ = (long long)__builtin_amdgcn_s_memtime();         \
            if (threadIdx.x == 0) a.stamps[b * 32 + (k)] = t_;                    \
        }                                                                         \
    } while (0)

#ifndef PCX_MEDIUM_WAVES  // waves per SIMD the VGPR budget is sized for (a build parameter for A/B runs)
#define PCX_MEDIUM_WAVES 3
#endif
