"""The Monte Carlo simulator's round generator on the CPU (no GPU needed).

``pcx_sim_generate_host`` runs the inline code the device kernel runs (csrc/pcx_sim.h).  It is
checked here against a numpy restatement written from the specification (DESIGN.md
"Simulator"), not by calling libpcx: Philox4x32-10 on uint64 arrays, counters (event j,
reporter i, round b, stream << 24 | timestep), decisions ``w < floor(p * 2^32)``, 53-bit
uniforms and fp64 +, -, * one rounding each.
"""
import ctypes as C
import math

import numpy as np
import pytest

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SHAPES = [(1, 1, 1, 0), (3, 7, 5, 2), (5, 64, 32, 1), (2, 65, 33, 0), (4, 50, 20, 3)]
SEEDS = [20261019, (0xC0FFEE << 32) | 0x1234567]  # the second exercises the key's high word
DEFAULTS = dict(liar_frac=0.3, collude_frac=0.5, distort=0.1, na_frac=0.1, scaled_frac=0.25)

# ------------------------------------------------------------------ numpy restatement
_M0, _M1, _MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
EVENT_A, EVENT_B, EVENT_C, REPORTER, CELL = range(5)


def np_philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over broadcast uint64 arrays that hold 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _MASK,
                          (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _MASK)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def np_u53(a, b):
    hi = (a >> np.uint64(5)).astype(np.float64) * 67108864.0
    return (hi + (b >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)


def np_frac(u):
    return 0.001 + 0.999 * u


def _thr(p):
    return np.uint64(int(math.floor(p * 4294967296.0)))


def np_generate(B, N, E, t, seed, liar_frac, collude_frac, distort, na_frac, scaled_frac):
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    b2, j2 = np.arange(B, dtype=np.uint64)[:, None], np.arange(E, dtype=np.uint64)[None, :]
    a = np_philox(j2, 0, b2, EVENT_A << 24 | t, k0, k1)
    q = np_philox(j2, 0, b2, EVENT_B << 24 | t, k0, k1)
    c = np_philox(j2, 0, b2, EVENT_C << 24 | t, k0, k1)
    scaled = a[0] < _thr(scaled_frac)
    lo_s = -100.0 + 100.0 * np_u53(a[2], a[3])
    hi_s = lo_s + (1.0 + 199.0 * np_u53(q[0], q[1]))
    truth_s = lo_s + (hi_s - lo_s) * np_frac(np_u53(q[2], q[3]))
    lie_s = lo_s + (hi_s - lo_s) * np_frac(np_u53(c[0], c[1]))
    truth_b = 1.0 + (a[1] >> np.uint64(31)).astype(np.float64)
    lo, hi = np.where(scaled, lo_s, 1.0), np.where(scaled, hi_s, 2.0)
    truth, lie = np.where(scaled, truth_s, truth_b), np.where(scaled, lie_s, 3.0 - truth_b)
    i2 = np.arange(N, dtype=np.uint64)[None, :]
    r = np_philox(0, i2, b2, REPORTER << 24, k0, k1)
    liar = r[0] < _thr(liar_frac)
    colludes = liar & (r[1] < _thr(collude_frac))
    b3, i3, j3 = b2[:, :, None], i2[:, :, None], j2[:, None, :]
    x = np_philox(j3, i3, b3, CELL << 24 | t, k0, k1)
    u = np_u53(x[2], x[3])
    lo3, hi3 = lo[:, None, :], hi[:, None, :]
    rv = np.where(scaled[:, None, :], lo3 + (hi3 - lo3) * np_frac(u), np.where(u < 0.5, 1.0, 2.0))
    honest = np.where(x[1] < _thr(distort), rv, truth[:, None, :])
    lying = np.where(colludes[:, :, None], lie[:, None, :], rv)
    reports = np.where(liar[:, :, None], lying, honest)
    reports[x[0] < _thr(na_frac)] = np.nan
    return {"reports": reports, "scaled": scaled.astype(np.uint8), "lo": lo, "hi": hi, "truth": truth,
            "liar": liar.astype(np.uint8) | (colludes.astype(np.uint8) << 1), "lie": lie}


def same_bits(a, b):
    """Equal bit for bit, NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    return bool((np.isnan(a) == np.isnan(b)).all() and
                (a.view(np.uint64)[~np.isnan(a)] == b.view(np.uint64)[~np.isnan(b)]).all())


# ------------------------------------------------------------------ tests
def test_philox_known_answers():
    from pyconsensus_amd import _lib

    h = _lib.lib()
    for ctr, key, want in KAT:
        out = (C.c_uint32 * 4)()
        h.pcx_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert tuple(out) == want
        got = np_philox(*ctr, *key)
        assert tuple(int(w) for w in got) == want


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_generate_host_is_the_specification(shape, seed):
    from pyconsensus_amd.simulate import generate_host

    B, N, E, t = shape
    got = generate_host(B, N, E, t=t, seed=seed, **DEFAULTS)
    want = np_generate(B, N, E, t, seed, **DEFAULTS)
    for name in ("reports", "scaled", "lo", "hi", "truth", "liar"):
        assert same_bits(got[name], want[name]), name
    assert got["reports"].shape == (B, N, E) and got["liar"].dtype == np.uint8


def test_probability_extremes():
    from pyconsensus_amd.simulate import generate_host

    B, N, E, seed = 6, 9, 7, 5
    base = dict(DEFAULTS)

    def gen(**kw):
        return generate_host(B, N, E, t=1, seed=seed, **dict(base, **kw))

    assert np.isnan(gen(na_frac=1.0)["reports"]).all()
    assert not np.isnan(gen(na_frac=0.0)["reports"]).any()
    assert (gen(liar_frac=0.0)["liar"] == 0).all()
    assert (gen(liar_frac=1.0)["liar"] & 1 == 1).all()
    assert (gen(scaled_frac=0.0)["scaled"] == 0).all()
    g = gen(scaled_frac=0.0)
    assert (g["lo"] == 1.0).all() and (g["hi"] == 2.0).all() and np.isin(g["truth"], (1.0, 2.0)).all()
    assert (gen(scaled_frac=1.0)["scaled"] == 1).all()
    # every liar colludes: each of its cells is the event's lie (3 - truth on a binary event;
    # the restatement supplies the scaled events' lie, which the generator does not return)
    g = gen(collude_frac=1.0, na_frac=0.0)
    lie = np_generate(B, N, E, 1, seed, **dict(base, collude_frac=1.0, na_frac=0.0))["lie"]
    liars = g["liar"] & 1 == 1
    assert liars.any() and (g["liar"][liars] == 3).all()
    assert (g["reports"] == np.broadcast_to(lie[:, None, :], (B, N, E)))[liars].all()
    binary = g["scaled"] == 0
    assert (lie[binary] == 3.0 - g["truth"][binary]).all()
    # nobody lies, nothing is distorted, nothing is missing: every report is the truth
    g = gen(liar_frac=0.0, distort=0.0, na_frac=0.0)
    assert (g["reports"] == g["truth"][:, None, :]).all()
    # every honest report distorted: a random value inside the event's range, never lo
    g = gen(liar_frac=0.0, distort=1.0, na_frac=0.0, scaled_frac=1.0)
    assert (g["reports"] > g["lo"][:, None, :]).all() and (g["reports"] <= g["hi"][:, None, :]).all()
    assert (g["reports"] != g["truth"][:, None, :]).all()
    # liars that never collude report random values as well
    g = gen(liar_frac=1.0, collude_frac=0.0, na_frac=0.0, scaled_frac=1.0)
    assert (g["liar"] == 1).all() and (g["reports"] != g["truth"][:, None, :]).all()


def test_liars_are_the_same_people_in_every_timestep():
    from pyconsensus_amd.simulate import generate_host

    a = generate_host(8, 50, 20, t=0, seed=3, **DEFAULTS)
    b = generate_host(8, 50, 20, t=5, seed=3, **DEFAULTS)
    assert (a["liar"] == b["liar"]).all() and (a["liar"] & 1).any()
    assert not same_bits(a["reports"], b["reports"]) and not same_bits(a["truth"], b["truth"])


def test_no_scaled_report_equals_lo():
    from pyconsensus_amd.simulate import generate_host

    g = generate_host(64, 50, 20, t=0, seed=11, **dict(DEFAULTS, scaled_frac=1.0, distort=0.5))
    finite = ~np.isnan(g["reports"])
    assert finite.any()
    assert (g["reports"] != np.broadcast_to(g["lo"][:, None, :], g["reports"].shape))[finite].all()
    assert (g["truth"] != g["lo"]).all() and (g["hi"] > g["lo"]).all()


def test_empirical_rates():
    """Each rate within 4 standard errors (binomial, from the parameter) of its parameter."""
    from pyconsensus_amd.simulate import generate_host

    B, N, E = 4096, 50, 20
    p = DEFAULTS
    g = generate_host(B, N, E, t=0, seed=20261019, **p)

    def within(count, n, prob, what):
        se = math.sqrt(prob * (1.0 - prob) / n)
        assert abs(count / n - prob) <= 4.0 * se, (what, count / n, prob, se)

    missing = np.isnan(g["reports"])
    within(int(missing.sum()), B * N * E, p["na_frac"], "missing")
    liars = g["liar"] & 1 == 1
    within(int(liars.sum()), B * N, p["liar_frac"], "liar")
    within(int((g["liar"][liars] & 2 == 2).sum()), int(liars.sum()), p["collude_frac"], "collude")
    within(int(g["scaled"].sum()), B * E, p["scaled_frac"], "scaled")
    # distortion shows on scaled events (a random value there is never the truth): honest
    # reporters' reports that are present and differ from the truth
    sel = (~liars)[:, :, None] & (g["scaled"] == 1)[:, None, :] & ~missing
    differs = g["reports"] != np.broadcast_to(g["truth"][:, None, :], g["reports"].shape)
    within(int((differs & sel).sum()), int(sel.sum()), p["distort"], "distort")


def _host_rc(t=0, **kw):
    """pcx_sim_generate_host's status and message for a 2 x 3 x 4 simulation with ``kw`` changed
    (every output pointer NULL: an accepted call writes nothing)."""
    from pyconsensus_amd import _abi, _lib
    from pyconsensus_amd.simulate import _sim

    args = dict(B=2, N=3, E=4, T=1, seed=1, scaled_tol=0.1, algorithm="PCA", **DEFAULTS)
    args.update(kw)
    rc = _lib.lib().pcx_sim_generate_host(C.byref(_sim(**args)), t, C.byref(_abi.SimRounds()))
    return rc, _lib.lib().pcx_last_error().decode()


@pytest.mark.parametrize("bad", [
    dict(liar_frac=-0.01), dict(liar_frac=1.5), dict(liar_frac=float("nan")), dict(liar_frac=float("inf")),
    dict(collude_frac=-1.0), dict(collude_frac=1.0000001), dict(collude_frac=float("nan")),
    dict(distort=-0.5), dict(distort=2.0), dict(distort=float("nan")),
    dict(na_frac=-1e-9), dict(na_frac=1.1), dict(na_frac=float("-inf")),
    dict(scaled_frac=-0.25), dict(scaled_frac=7.0), dict(scaled_frac=float("nan")),
    dict(scaled_tol=-0.1), dict(scaled_tol=float("nan")), dict(scaled_tol=float("inf")),
    dict(T=0), dict(T=1 << 24), dict(T=-3),
    dict(algorithm="k-means"), dict(algorithm="cokurtosis"),
    dict(B=-1), dict(B=1 << 31), dict(N=0), dict(N=1 << 31), dict(E=0), dict(E=65537),
    dict(algorithm="big-five", max_components=0),
    dict(algorithm="fixed-variance", variance_threshold=float("nan")),
    dict(algorithm="hierarchical", hierarchy_threshold=float("nan")),
    dict(catch_tolerance=float("inf")), dict(alpha=float("nan")),
], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_rejected_arguments(bad):
    from pyconsensus_amd import _abi

    rc, msg = _host_rc(**bad)
    assert rc == _abi.EINVAL and msg, (rc, msg)


def test_rejected_timestep_algorithm_and_null():
    from pyconsensus_amd import _abi, _lib
    from pyconsensus_amd.simulate import _sim

    assert _host_rc(t=-1)[0] == _abi.EINVAL
    assert _host_rc(t=1 << 24)[0] == _abi.EINVAL
    assert _host_rc(t=(1 << 24) - 1)[0] == _abi.OK  # (every output NULL: nothing is written)
    assert _host_rc()[0] == _abi.OK
    for alg in (-1, 8, 99):
        s = _sim(B=2, N=3, E=4, T=1, seed=1, **DEFAULTS)
        s.algorithm = alg
        assert _lib.lib().pcx_sim_generate_host(C.byref(s), 0, C.byref(_abi.SimRounds())) == _abi.EINVAL
    s = _sim(B=2, N=3, E=4, T=1, seed=1, algorithm="big-five", **DEFAULTS)
    s.max_components = 5  # > n_events
    assert _lib.lib().pcx_sim_generate_host(C.byref(s), 0, C.byref(_abi.SimRounds())) == _abi.EINVAL
    assert _lib.lib().pcx_sim_generate_host(None, 0, C.byref(_abi.SimRounds())) == _abi.EINVAL
    assert _lib.lib().pcx_sim_generate_host(C.byref(s), 0, None) == _abi.EINVAL


def test_abi_mirrors_of_the_simulator_structs():
    """Byte layout of pcx_sim / pcx_sim_rounds / pcx_sim_result as the C compiler lays them out."""
    import os
    import subprocess
    import tempfile

    from pyconsensus_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"pcx_sim": _abi.Sim, "pcx_sim_rounds": _abi.SimRounds, "pcx_sim_result": _abi.SimResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pcx.h"', "int main(void) {",
             'printf("abi %d\\n", PCX_ABI_VERSION); printf("nmetrics %d\\n", PCX_SIM_NMETRICS);']
    for cname, py in structs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), src, "-o", exe])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["abi"]) == _abi.ABI_VERSION == 9 and int(out["nmetrics"]) == _abi.SIM_NMETRICS
    for cname, py in structs.items():
        assert int(out["%s size" % cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)
