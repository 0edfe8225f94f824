"""The batched kernel's covariance divisions (csrc/pcx_batched_round.inc, `put`): an accumulator over the
token sum minus one through div_rn (csrc/pcx_fastdiv.h) with y = range_rcp(denom) formed once per round.
The stand-alone C restatement of tests/test_fastdiv.py (the same operations in the same order) over the
operands this site sees: numerators that are the SPEC's chains fma((F_ij - mu_j) tok_i, F_ik - mu_k, acc)
over 50 reporters with integer tokens and binary, scaled or agreed columns (an agreed pair's accumulator is
an exact zero, which takes the guard's division), denominators that are integers in [1, 6.4e7].  Every
quotient must equal the IEEE division bit for bit."""
import subprocess
import textwrap

import pytest

SRC = textwrap.dedent(r"""
    #include <math.h>
    #include <stdint.h>
    #include <stdio.h>
    #include <stdlib.h>
    #include <string.h>
    static uint64_t s = 88172645463325252ull;
    static uint64_t xr(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    static double unit(void) { return (xr() >> 11) * 0x1p-53; }
    static uint64_t ubits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
    static double range_rcp(double b) {
        double a = fabs(b);
        return (a >= 0x1p-100 && a <= 0x1p100) ? 1.0 / b : NAN;
    }
    static double div_rn(double d, double b, double y) {  /* pcx_fastdiv.h div_rn */
        volatile double q0 = d * y;
        volatile double r = fma(-q0, b, d);
        double q = fma(r, y, q0);
        if (isnan(y) || fabs(q0) < 0x1p-860 || fabs(q0) > 0x1p1000) q = d / b;
        return q;
    }
    enum { N = 50 };
    static void column(double* f, int kind) {  /* 0 binary, 1 scaled in [0, 1], 2 every reporter agrees */
        double agreed = 1.0 + (double)(xr() & 1);
        for (int i = 0; i < N; i++) f[i] = kind == 0 ? 1.0 + (double)(xr() & 1) : kind == 1 ? unit() : agreed;
    }
    static double mean(const double* f, const double* rep) {  /* the weighted mean's chain over the sum of rep */
        double acc = f[0] * rep[0], den = 0.0;
        for (int i = 1; i < N; i++) acc = acc + f[i] * rep[i];
        for (int i = 0; i < N; i++) den += rep[i];
        return acc / den;
    }
    int main(int argc, char** argv) {
        long n = atol(argv[1]), bad = 0, fast = 0, zeros = 0;
        s ^= (uint64_t)atol(argv[2]);
        for (long k = 0; k < n; k++) {
            double rep[N], tok[N], fj[N], fk[N], tot = 0.0, toksum = 0.0;
            for (int i = 0; i < N; i++) { rep[i] = 1.0 + (double)(xr() % 99); tot += rep[i]; }
            for (int i = 0; i < N; i++) { rep[i] /= tot; tok[i] = trunc(rep[i] * 1e6); toksum += tok[i]; }
            /* the round's own denominator, or any integer in [1, 6.4e7] (64 reporters' tokens at most) */
            double denom = k % 2 ? toksum - 1.0 : 1.0 + (double)(xr() % 64000000ull);
            column(fj, (int)(xr() % 3));
            if (xr() % 4 == 0) memcpy(fk, fj, sizeof fk); else column(fk, (int)(xr() % 3));  /* a diagonal entry */
            double mj = mean(fj, rep), mk = mean(fk, rep), acc = 0.0;
            for (int i = 0; i < N; i++) acc = fma((fj[i] - mj) * tok[i], fk[i] - mk, acc);
            double y = range_rcp(denom);
            double e = acc / denom, f = div_rn(acc, denom, y);
            if (acc == 0.0) zeros++;
            if (!isnan(y) && !(fabs(acc * y) < 0x1p-860 || fabs(acc * y) > 0x1p1000)) fast++;
            if (isnan(e) ? !isnan(f) : ubits(e) != ubits(f)) {
                if (bad < 5) printf("b=%a d=%a expect=%a got=%a\n", denom, acc, e, f);
                bad++;
            }
        }
        printf("n=%ld fast=%ld zeros=%ld bad=%ld\n", n, fast, zeros, bad);
        return bad != 0;
    }
""")


@pytest.fixture(scope="module")
def fastdiv_cov_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastdiv_cov")
    src, exe = d / "fastdiv_cov.c", d / "fastdiv_cov"
    src.write_text(SRC)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", str(src), "-o", str(exe), "-lm"],
                   check=True)
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_covariance_quotients_equal_division(fastdiv_cov_bin, seed):
    r = subprocess.run([str(fastdiv_cov_bin), "400000", str(seed)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad=0" in r.stdout
    fast = int(r.stdout.split("fast=")[1].split()[0])
    zeros = int(r.stdout.split("zeros=")[1].split()[0])
    # an operand is an agreed column one time in three, so about 5 / 9 of the accumulators are exact zeros
    # (the guard's division) and the rest take the fast path: both must occur in quantity
    assert fast > 100_000 and zeros > 100_000
