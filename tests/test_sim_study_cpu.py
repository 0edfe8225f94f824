"""Simulator studies without a GPU: the host entries of the detail metrics and of the
per-cell statistics against numpy restatements of the specification, pcx_sim_study_check's refusals,
the struct layouts and ``pair_with="first"``.

Everything is compared bit for bit, all NaNs alike: the host entries are the inline code of the kernels.
"""
import ctypes as C
import sys

import numpy as np
import pytest

import sim_study_cases as S


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401  (the module: the package exports the function of that name)

    return sys.modules["pyconsensus_amd.simulate"]


def test_exports_and_names():
    import pyconsensus_amd
    from pyconsensus_amd import _abi, _lib

    h = _lib.lib()
    for name in ("pcx_sim_detail_f64", "pcx_sim_detail_host", "pcx_sim_sweep_detail_f64", "pcx_sim_sweep_detail_host",
                 "pcx_sim_study_check", "pcx_sim_sweep_stats_f64", "pcx_sim_sweep_stats_host", "pcx_simulate_study_f64"):
        assert hasattr(h, name), name
    M = _sim()
    assert pyconsensus_amd.study is M.study
    assert len(M.DETAIL) == _abi.SIM_NDETAIL == 12 and M.VALUES == M.METRICS + M.DETAIL and len(M.VALUES) == 18
    assert M.STATS == ("n", "mean", "var", "min", "max")
    assert M.DETAIL[6:10] == ("tp", "fn", "fp", "tn") and M.DETAIL[10] == "mcc"


def test_abi_mirror_of_the_study_struct():
    """pcx_sim_study_result (and the sweep structs it travels with) as the C compiler lays them out."""
    import os
    import subprocess
    import tempfile

    from pyconsensus_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"pcx_sim_study_result": _abi.SimStudyResult, "pcx_sim_sweep": _abi.SimSweep,
               "pcx_sim_result": _abi.SimResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pcx.h"', "int main(void) {",
             'printf("abi %d\\n", PCX_ABI_VERSION); printf("nmetrics %d\\n", PCX_SIM_NMETRICS);',
             'printf("ndetail %d\\n", PCX_SIM_NDETAIL); printf("nvalues %d\\n", PCX_SIM_NVALUES);',
             'printf("nstats %d\\n", PCX_SIM_NSTATS); printf("npaired %d\\n", PCX_SIM_NPAIRED);']
    for cname, py in structs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), src,
                               "-o", exe])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["abi"]) == _abi.ABI_VERSION == 9 and int(out["nmetrics"]) == _abi.SIM_NMETRICS == 6
    assert (int(out["ndetail"]), int(out["nvalues"])) == (_abi.SIM_NDETAIL, _abi.SIM_NVALUES) == (12, 18)
    assert (int(out["nstats"]), int(out["npaired"])) == (_abi.SIM_NSTATS, _abi.SIM_NPAIRED) == (5, 3)
    for cname, py in structs.items():
        assert int(out["%s size" % cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)
    assert C.sizeof(_abi.SimStudyResult) == 24


# ------------------------------------------------------------------ detail metrics
@pytest.fixture(scope="module")
def hand():
    flat, per_cell = S.hand_rounds()
    want = [S.np_detail_cell(d, S.TOL) for d in per_cell]
    return flat, per_cell, want


def test_hand_made_rounds_reach_every_case(hand):
    """What the detail test relies on: each cell's rounds reach every branch of the definitions."""
    _, per_cell, want = hand
    for c, (d, w) in enumerate(zip(per_cell, want)):
        sc, lies, out = d["scaled"] != 0, (d["liar"] & 1) == 1, d["outcomes"]
        assert sc.all(axis=1).any() and (~sc).all(axis=1).any(), c          # no binary event / no scaled event
        assert (~lies).all(axis=1).any() and lies.all(axis=1).any(), c      # no liar / only liars
        assert ((d["liar"] & 3) != 3).all(axis=1).any(), c                  # a colluder-free round
        tp, fn, fp, tn = (w[:, k] for k in (6, 7, 8, 9))
        for factor in (tp + fp, tp + fn, tn + fp, tn + fn):                 # every mcc factor zero in turn
            assert (factor == 0).any(), c
            assert np.isnan(w[factor == 0, 10]).all(), c
        assert np.isnan(d["smooth"]).any(), c
        assert (np.isnan(out) & ~sc).any() and (np.isnan(out) & sc).any(), c
        assert ((out == 1.5) & ~sc).any() and ((out == 3.0 - d["truth"]) & ~sc).any(), c
        assert (sc & (np.abs(out - d["truth"]) == S.TOL * (d["hi"] - d["lo"])) & (out != d["truth"])).any(), c
        assert np.isnan(w[:, 0]).any() and np.isnan(w[:, 1]).any() and np.isnan(w[:, 5]).any(), c
        assert (w[:, 6:10].sum(axis=1) == d["liar"].shape[1]).all(), c
    # the outcome on the tolerance bound counts as correct: round 11 of the 1 x 1 cell is that event alone
    assert want[0][11, 1] == 1.0 and want[0][11, 5] == 0.25
    # mcc is a number where no factor is zero
    assert np.isfinite(want[3][:, 10]).any() and (np.abs(want[3][np.isfinite(want[3][:, 10]), 10]) <= 1.0).all()


def test_sweep_detail_host_is_the_specification(hand):
    flat, per_cell, want = hand
    got = _sim().sweep_detail_host(S.HAND_CELLS, S.rounds_of(flat), flat["old"], flat["smooth"], flat["outcomes"],
                                   scaled_tol=S.TOL)
    assert got.shape == (sum(c["rounds"] for c in S.HAND_CELLS), 12)
    b = 0
    for c, w in enumerate(want):
        for r in range(len(w)):
            assert S.same_bits(got[b + r], w[r]), (c, r, got[b + r], w[r])
        b += len(w)


def test_detail_host_of_one_cell_is_its_slice(hand):
    flat, per_cell, want = hand
    for c in (0, 2, 3):
        d = per_cell[c]
        got = _sim().detail_host({k: d[k] for k in ("scaled", "lo", "hi", "truth", "liar")}, d["old"], d["smooth"],
                                 d["outcomes"], scaled_tol=S.TOL)
        assert S.same_bits(got, want[c]), c


def test_detail_refuses_wrong_lengths(hand):
    flat, _, _ = hand
    M = _sim()
    with pytest.raises(ValueError):
        M.sweep_detail_host(S.HAND_CELLS, S.rounds_of(flat), flat["old"][:-1], flat["smooth"], flat["outcomes"])
    with pytest.raises(Exception) as e:
        M.sweep_detail_host([S.cell(2, 5, 3, 1), S.cell(2, 300, 3, 1)], S.rounds_of(flat), flat["old"], flat["smooth"],
                            flat["outcomes"])
    assert "cell 1:" in str(e.value)


# ------------------------------------------------------------------ statistics and paired differences
@pytest.fixture(scope="module")
def stats_case():
    metrics, detail = S.stats_values()
    return metrics, detail, S.np_stats(S.STATS_CELLS, metrics, detail, S.STATS_BASE)


def test_sweep_stats_host_is_the_specification(stats_case):
    metrics, detail, (want_stats, want_paired) = stats_case
    got = _sim().sweep_stats_host(S.STATS_CELLS, metrics, detail, pair_with=list(S.STATS_BASE))
    Cn = len(S.STATS_CELLS)
    assert got["stats"].shape == (S.STATS_T, Cn, 18, 5) and got["paired"].shape == (S.STATS_T, Cn, 18, 3)
    assert got["pair_base"].tolist() == S.STATS_BASE.tolist()
    for t in range(S.STATS_T):
        for c in range(Cn):
            assert S.same_bits(got["stats"][t, c], want_stats[t, c]), (t, c)
            assert S.same_bits(got["paired"][t, c], want_paired[t, c]), (t, c)
    st, pr = got["stats"], got["paired"]
    R = np.array([c["rounds"] for c in S.STATS_CELLS], dtype=np.float64)
    assert (st[:, :, :6, 0] == R[None, :, None]).all()                      # no NaN among the metrics
    assert (st[:, 2, 7, 0] == 0).all() and np.isnan(st[:, 2, 7, 1:]).all()  # a whole column NaN: n = 0
    assert np.isnan(st[:, 0, :6, 2]).all() and (st[:, 0, :6, 3] == st[:, 0, :6, 4]).all()  # R = 1: no variance
    assert (pr[:, :6, :, 0] == 0).all() and np.isnan(pr[:, :6, :, 1:]).all()  # base -1
    assert (pr[:, 6, 9, 0] == 255).all() and (pr[:, 7, 9, 0] == 256).all()    # NaN on either side of a pair
    assert (pr[:, 6, 2, 0] == 257).all() and (st[:, 6, 9, 0] == 256).all() and (st[:, 4, 9, 0] == 256).all()
    assert np.isnan(pr[:, 10, :6, 2]).all() and (pr[:, 10, :6, 0] == 1).all()  # one pair: a mean, no variance
    # the order is observable: a plain numpy mean has other bits somewhere
    assert not S.same_bits(st[0, 5, :6, 1], metrics[0, S_start(5):S_start(6)].mean(axis=0))


def S_start(c):
    return int(sum(k["rounds"] for k in S.STATS_CELLS[:c]))


def test_stats_means_are_the_sweep_summary_bytes(stats_case):
    """With no NaN, `mean` of the six base metrics is the sweep's summary, replayed in numpy."""
    metrics, detail, _ = stats_case
    got = _sim().sweep_stats_host(S.STATS_CELLS, metrics, detail)
    assert "paired" not in got
    for t in range(S.STATS_T):
        for c in range(len(S.STATS_CELLS)):
            want = S.W.np_summary(metrics[t, S_start(c):S_start(c + 1)])
            assert S.same_bits(got["stats"][t, c, :6, 1], want), (t, c)


def test_stderr():
    M = _sim()
    x = np.array([[4.0, 1.0, 16.0, 0.0, 2.0], [1.0, 1.0, np.nan, 1.0, 1.0], [0.0, np.nan, np.nan, np.nan, np.nan]])
    se = M.stderr(x)
    assert se[0] == 2.0 and np.isnan(se[1]) and np.isnan(se[2])
    assert M.stderr(x[:, :3])[0] == 2.0  # a paired array has n and var in the same places


# ------------------------------------------------------------------ pcx_sim_study_check
def _check(cells, base):
    from pyconsensus_amd import _lib

    s, arr, _, _ = _sim()._sweep(cells, 1)
    bad = C.c_int64(-7)
    b = None if base is None else np.asarray(base, dtype=np.int32)
    rc = _lib.lib().pcx_sim_study_check(C.byref(s), None if b is None else b.ctypes.data, C.byref(bad))
    return rc, bad.value, _lib.lib().pcx_last_error().decode()


CHECK_CELLS = [S.cell(4, 5, 3, 1), S.cell(4, 6, 2, 1), S.cell(5, 5, 3, 1)]
CHECK_REFUSALS = [("base = C", [-1, 3, -1], 1), ("base = -2", [-1, -1, -2], 2), ("self", [0, 0, -1], 0),
                  ("another R", [-1, 0, 1], 2)]


@pytest.mark.parametrize("what,base,bad_cell", CHECK_REFUSALS, ids=[r[0] for r in CHECK_REFUSALS])
def test_study_check_refusals_name_the_cell(what, base, bad_cell):
    rc, bad, msg = _check(CHECK_CELLS, base)
    assert rc == -1 and bad == bad_cell, (what, rc, bad, msg)
    assert msg.startswith("pcx_sim_study_check: ") and "cell %d:" % bad_cell in msg, msg
    M = _sim()
    with pytest.raises(Exception) as e:
        M.study_check(CHECK_CELLS, base)
    assert "cell %d:" % bad_cell in str(e.value)
    # the host statistics refuse the same pairing before they read or write anything (the arrays are too small)
    from pyconsensus_amd import _abi, _lib

    s, arr, _, _ = M._sweep(CHECK_CELLS, 1)
    b = np.asarray(base, dtype=np.int32)
    one = np.zeros(1)
    rc = _lib.lib().pcx_sim_sweep_stats_host(C.byref(s), one.ctypes.data, one.ctypes.data, b.ctypes.data,
                                             one.ctypes.data, one.ctypes.data)
    assert rc == -1 and "cell %d:" % bad_cell in _lib.lib().pcx_last_error().decode() and one[0] == 0.0


def test_study_check_accepts():
    assert _check(CHECK_CELLS, None)[:2] == (0, -1)                 # a NULL pair_base
    assert _check(CHECK_CELLS, [-1, 0, -1])[:2] == (0, -1)          # another shape, the same R: a legal base
    assert _check(CHECK_CELLS, [1, 0, -1])[:2] == (0, -1)           # two cells may be each other's base
    assert _check([], None)[:2] == (0, -1)
    rc, bad, msg = _check([S.cell(4, 5, 3, 1), S.cell(4, 300, 3, 1)], [-1, 0])  # what the plan refuses
    assert rc == -1 and bad == 1 and "cell 1:" in msg
    assert _sim().study_check(CHECK_CELLS, None) is None
    assert _sim().study_check(CHECK_CELLS, [-1, 0, -1]).tolist() == [-1, 0, -1]
    with pytest.raises(ValueError):
        _sim().study_check(CHECK_CELLS, [-1, 0])
    with pytest.raises(ValueError):
        _sim().study_check(CHECK_CELLS, "last")


# ------------------------------------------------------------------ pair_with="first"
def test_pair_with_first():
    M = _sim()
    g = M.grid(16, seed=5, reporters=[20, 50], liar_frac=[0.1, 0.2, 0.3])
    assert M.pair_base(g, "first").tolist() == [-1, 0, 0, -1, 3, 3]     # two shapes: two first cells
    assert M.study_check(g, "first").tolist() == [-1, 0, 0, -1, 3, 3]
    ind = M.grid(16, seed=5, independent=True, reporters=[20, 50], liar_frac=[0.1, 0.2, 0.3])
    assert M.pair_base(ind, "first").tolist() == [-1] * 6               # other seeds: nobody has a base
    mixed = [S.cell(4, 5, 3, 1), S.cell(5, 5, 3, 1), S.cell(4, 5, 3, 1), S.cell(4, 5, 4, 1), S.cell(5, 5, 3, 1)]
    assert M.pair_base(mixed, "first").tolist() == [-1, -1, 0, -1, 1]   # rounds and events count too
    assert M.pair_base(g, None) is None
