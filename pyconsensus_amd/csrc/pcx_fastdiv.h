// pcx_fastdiv.h -- a correctly rounded fp64 division by a denominator whose reciprocal is formed once:
// shared by the single-matrix units (pcx_mat_device.h: the rescale by a column's range) and the batched
// round kernel (pcx_batched_round.inc: the covariance's divisions by the wave-uniform token sum).  The
// helpers sit in each unit's anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>

namespace pcx {
namespace {

// d / b correctly rounded from y = RN(1 / b) (Markstein: q0 = RN(d y) is faithful, the residual
// d - b q0 is exact in one fma, and RN(q0 + r y) = RN(d / b)), in 4 fp64 ops where the IEEE
// division sequence (div_scale x2, rcp, 5 fma, div_fmas, div_fixup) takes 11 with a quarter-rate
// rcp.  The theorem assumes no underflow or overflow: with |b| in [2^-100, 2^100] (else y is
// NaN) and |q0| in [2^-860, 2^1000], |d| >= 2^-960 keeps the residual exact and q finite.  Other
// cells -- zeros among them, whose sign the fast path can get wrong (-0 / b) -- divide (a branch,
// skipped when no lane needs it).  NaN d passes: the fast path returns NaN as the division does.
// tests/test_fastdiv.py checks the sequence and its guard against the division bit for bit.
__device__ __forceinline__ double div_rn(double d, double b, double y) {
    const double q0 = d * y;
    const double r = __builtin_fma(-q0, b, d);
    double q = __builtin_fma(r, y, q0);
    const bool slow = __builtin_isnan(y) | (fabs(q0) < 0x1p-860) | (fabs(q0) > 0x1p1000);
    if (__builtin_expect(slow, 0)) q = d / b;
    return q;
}

__device__ __forceinline__ double range_rcp(double range) {
    const double a = fabs(range);
    return (a >= 0x1p-100 && a <= 0x1p100) ? 1.0 / range : __builtin_nan("");
}

}  // namespace
}  // namespace pcx
