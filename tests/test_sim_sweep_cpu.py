"""Simulator sweeps without a GPU: the struct layouts, the host generator against the equal-shape host
generator cell by cell, common random numbers, and pcx_sim_sweep_plan with its refusals.

Everything is compared bit for bit (a cell's slice is that cell's own simulation).
"""
import ctypes as C

import numpy as np
import pytest

import sim_sweep_cases as W


def _sim():
    import pyconsensus_amd.simulate  # noqa: F401  (the module: the package exports the function of that name)
    import sys

    return sys.modules["pyconsensus_amd.simulate"]


def test_exports():
    from pyconsensus_amd import _lib

    h = _lib.lib()
    for name in ("pcx_sim_sweep_plan", "pcx_sim_sweep_generate_host", "pcx_sim_sweep_generate_f64",
                 "pcx_sim_sweep_metrics_f64", "pcx_simulate_sweep_f64"):
        assert hasattr(h, name), name


def test_abi_mirrors_of_the_sweep_structs():
    """Byte layout of pcx_sim_cell / pcx_sim_sweep as the C compiler lays them out (the header stays C99)."""
    import os
    import subprocess
    import tempfile

    from pyconsensus_amd import _abi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"pcx_sim_cell": _abi.SimCell, "pcx_sim_sweep": _abi.SimSweep}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pcx.h"', "int main(void) {",
             'printf("abi %d\\n", PCX_ABI_VERSION);']
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
    assert int(out["abi"]) == _abi.ABI_VERSION == 9
    for cname, py in structs.items():
        assert int(out["%s size" % cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)


# ------------------------------------------------------------------ the host generator
@pytest.mark.parametrize("t", [0, 2])
def test_host_generator_is_the_equal_shape_generator_cell_by_cell(t):
    S = _sim()
    got = S.sweep_generate_host(W.HOST_SWEEP, t)
    off = got["offsets"]
    assert off["rounds"].tolist() == [0, 3, 5, 9, 11, 12]
    for c, k in enumerate(W.HOST_SWEEP):
        want = S.generate_host(k["rounds"], k["reporters"], k["events"], t=t, seed=k["seed"], **W.rates(k))
        for name in W.ROUNDS:
            mine = W.cell_slice(got[name], off, W.OFFSET_OF[name], c)
            assert W.same_bits(mine, want[name].reshape(-1)), (c, name)


def test_tuple_cells_and_defaults():
    S = _sim()
    a = S.sweep_generate_host([(2, 7, 5, 9), {"rounds": 3}], 1)
    b = S.sweep_generate_host([W.cell(2, 7, 5, 9), W.cell(3, 50, 20, 0)], 1)
    for name in W.ROUNDS:
        assert W.same_bits(a[name], b[name]), name
    with pytest.raises(ValueError):
        S.sweep_generate_host([{"reporters": 3}])
    with pytest.raises(ValueError):
        S.sweep_generate_host([{"rounds": 3, "liars": 0.2}])


def test_common_random_numbers():
    S = _sim()
    same = S.sweep_generate_host([W.cell(4, 30, 12, 7), W.cell(4, 30, 12, 7), W.cell(4, 30, 12, 8)], 1)
    off = same["offsets"]
    for name in W.ROUNDS:
        k = W.OFFSET_OF[name]
        a, b, c = (W.cell_slice(same[name], off, k, i) for i in range(3))
        assert W.same_bits(a, b), name                    # the same seed, shape and rates: equal
    for name in ("reports", "truth", "liar"):
        k = W.OFFSET_OF[name]
        assert not W.same_bits(W.cell_slice(same[name], off, k, 0), W.cell_slice(same[name], off, k, 2)), name
    # the same word against two thresholds: the liars at 0.2 are liars at 0.4
    r = S.sweep_generate_host([W.cell(8, 200, 4, 7, liar_frac=0.2), W.cell(8, 200, 4, 7, liar_frac=0.4)], 0)
    few, many = (W.cell_slice(r["liar"], r["offsets"], "reporters", i) & 1 for i in range(2))
    assert 0 < few.sum() < many.sum() and not (few & ~many).any()
    # and whatever does not depend on the liars is the same in both: the events
    for name in ("scaled", "lo", "hi", "truth"):
        assert W.same_bits(W.cell_slice(r[name], r["offsets"], "events", 0),
                           W.cell_slice(r[name], r["offsets"], "events", 1)), name


def test_grid_shares_a_seed_unless_independent():
    S = _sim()
    g = S.grid(16, seed=5, liar_frac=[0.1, 0.3], reporters=[20, 50], events=10)
    assert [(c["liar_frac"], c["reporters"]) for c in g] == [(0.1, 20), (0.1, 50), (0.3, 20), (0.3, 50)]
    assert all(c["rounds"] == 16 and c["seed"] == 5 and c["events"] == 10 for c in g)
    assert [c["seed"] for c in S.grid(16, seed=5, independent=True, na_frac=[0.0, 0.1, 0.2])] == [5, 6, 7]
    assert S.grid(3) == [{"rounds": 3, "seed": 0}]
    with pytest.raises(ValueError):
        S.grid(3, liars=[0.1])


def test_probability_extremes_per_cell():
    S = _sim()
    r = S.sweep_generate_host([W.cell(3, 9, 4, 1, na_frac=1.0), W.cell(3, 9, 4, 1, na_frac=0.0),
                               W.cell(3, 9, 4, 1, liar_frac=0.0), W.cell(3, 9, 4, 1, liar_frac=1.0),
                               W.cell(3, 9, 4, 1, scaled_frac=0.0), W.cell(3, 9, 4, 1, scaled_frac=1.0)], 0)
    off = r["offsets"]
    assert np.isnan(W.cell_slice(r["reports"], off, "cells", 0)).all()
    assert not np.isnan(W.cell_slice(r["reports"], off, "cells", 1)).any()
    assert (W.cell_slice(r["liar"], off, "reporters", 2) == 0).all()
    assert (W.cell_slice(r["liar"], off, "reporters", 3) & 1 == 1).all()
    assert (W.cell_slice(r["scaled"], off, "events", 4) == 0).all()
    assert (W.cell_slice(r["scaled"], off, "events", 5) == 1).all()
    assert (W.cell_slice(r["lo"], off, "events", 4) == 1.0).all() and (W.cell_slice(r["hi"], off, "events", 4) == 2.0).all()


# ------------------------------------------------------------------ pcx_sim_sweep_plan
def _plan(cells, T=1, algorithm="PCA", **kw):
    """(rc, totals, counts, lds, bad_cell, message) of pcx_sim_sweep_plan."""
    from pyconsensus_amd import _lib

    S = _sim()
    s, arr, _, _ = S._sweep(cells, T, algorithm=algorithm, **kw)
    out = [(C.c_int64 * 4)() for _ in range(3)]
    bad = C.c_int64(-7)
    rc = _lib.lib().pcx_sim_sweep_plan(C.byref(s), out[0], out[1], out[2], C.byref(bad))
    return rc, [list(x) for x in out], bad.value, _lib.lib().pcx_last_error().decode()


@pytest.mark.parametrize("algorithm,kw", [("PCA", {}), ("big-five", {"max_components": 5}), ("hierarchical", {})])
def test_plan_totals_counts_and_lds(algorithm, kw):
    """One cell in each launch slot (50 x 20 on the wave kernel; 100 x 50 and 256 x 64 in workgroup launch
    classes, which depend on the algorithm's LDS) against pcx_ragged_plan_wide on the expanded rounds."""
    from pyconsensus_amd.batched import ragged_plan

    cells = [W.cell(3, 50, 20, 1), W.cell(5, 100, 50, 2), W.cell(2, 256, 64, 3), W.cell(4, 65, 33, 4)]
    rc, (totals, counts, lds), bad, _ = _plan(cells, algorithm=algorithm, **kw)
    assert rc == 0 and bad == -1
    R, N, E = (np.array([c[k] for c in cells], dtype=np.int64) for k in ("rounds", "reporters", "events"))
    assert totals == [R.sum(), (R * N).sum(), (R * E).sum(), (R * N * E).sum()]
    shapes = [(c["reporters"], c["events"]) for c in cells for _ in range(c["rounds"])]
    t3, counts_w, lds_w = ragged_plan(shapes, algorithm, wide=True)
    assert totals[1:] == [int(x) for x in t3]
    assert counts == [int(x) for x in counts_w] and lds == [int(x) for x in lds_w]
    assert counts[0] == 3 and sum(counts) == R.sum()


def test_plan_reaches_every_launch_slot():
    """50 x 20 runs on the wave kernel; under PCA 100 x 50 is launch class 3 and 256 x 64 class 2 or lower;
    256 x 64 under big-five is class 1: the four slots, as pcx_ragged_plan_wide assigns them."""
    from pyconsensus_amd.batched import ragged_plan

    seen = set()
    for algorithm, kw in (("PCA", {}), ("big-five", {"max_components": 5})):
        cells = [W.cell(1, 50, 20, 1), W.cell(1, 100, 50, 2), W.cell(1, 256, 64, 3)]
        rc, (_, counts, lds), _, _ = _plan(cells, algorithm=algorithm, **kw)
        assert rc == 0
        _, cw, lw = ragged_plan([(c["reporters"], c["events"]) for c in cells], algorithm, wide=True)
        assert counts == [int(x) for x in cw] and lds == [int(x) for x in lw]
        seen |= {k for k in range(4) if counts[k]}
    assert seen == {0, 1, 2, 3}


REFUSALS = [
    ("N = 0", [W.cell(2, 5, 3, 1), W.cell(2, 0, 3, 1)], {}, 1),
    ("N = 257", [W.cell(2, 257, 3, 1)], {}, 0),
    ("E = 65", [W.cell(2, 5, 3, 1), W.cell(2, 5, 3, 1), W.cell(2, 5, 65, 1)], {}, 2),
    ("R = 0", [W.cell(2, 5, 3, 1), W.cell(0, 5, 3, 1)], {}, 1),
    ("NaN probability", [W.cell(2, 5, 3, 1, distort=float("nan"))], {}, 0),
    ("probability 1.5", [W.cell(2, 5, 3, 1), W.cell(2, 5, 3, 1, na_frac=1.5)], {}, 1),
    ("T = 0", [W.cell(2, 5, 3, 1)], {"T": 0}, -1),
    ("T = 2^24", [W.cell(2, 5, 3, 1)], {"T": 1 << 24}, -1),
    ("k-means", [W.cell(2, 5, 3, 1)], {"algorithm": "k-means"}, -1),
    ("cokurtosis", [W.cell(2, 5, 3, 1)], {"algorithm": "cokurtosis"}, -1),
    ("sum R >= 2^31", [W.cell(1 << 30, 5, 3, 1), W.cell(1 << 30, 5, 3, 1)], {}, 1),  # pure: nothing is allocated
    ("NaN scaled_tol", [W.cell(2, 5, 3, 1)], {"scaled_tol": float("nan")}, -1),
    ("big-five without components", [W.cell(2, 5, 3, 1)], {"algorithm": "big-five", "max_components": 0}, -1),
]


@pytest.mark.parametrize("what,cells,kw,bad_cell", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_refusals_name_the_cell(what, cells, kw, bad_cell):
    rc, _, bad, msg = _plan(cells, **kw)
    assert rc == -1 and bad == bad_cell, (what, rc, bad, msg)
    assert msg.startswith("pcx_sim_sweep_plan: ")
    if bad_cell >= 0:
        assert "cell %d:" % bad_cell in msg, msg
    else:
        assert "cell " not in msg, msg
    # the host generator refuses the same sweep before it writes anything (its pointers are NULL here)
    if "T" not in kw:
        from pyconsensus_amd import _abi, _lib

        sweep, cell_array, _, _ = _sim()._sweep(cells, **kw)
        rc = _lib.lib().pcx_sim_sweep_generate_host(C.byref(sweep), 0, C.byref(_abi.SimRounds()))
        msg = _lib.lib().pcx_last_error().decode()
        assert rc == -1 and msg.startswith("pcx_sim_sweep_generate_host: "), msg
        assert ("cell %d:" % bad_cell in msg) == (bad_cell >= 0), msg


def test_the_largest_legal_totals_do_not_overflow():
    rc, (totals, counts, _), bad, _ = _plan([W.cell((1 << 31) - 1, 256, 64, 1)])
    assert rc == 0 and bad == -1
    R = (1 << 31) - 1
    assert totals == [R, R * 256, R * 64, R * 256 * 64] and sum(counts) == R


def test_empty_sweep():
    from pyconsensus_amd import _abi, _lib

    rc, (totals, counts, lds), bad, _ = _plan([])
    assert rc == 0 and bad == -1 and totals == [0, 0, 0, 0] and counts == [0, 0, 0, 0] and lds == [0, 0, 0, 0]
    S = _sim()
    r = S.sweep_generate_host([], 0)
    assert all(len(r[name]) == 0 for name in W.ROUNDS)
    s = _abi.SimSweep(0, None, 1, 0.1, 0.1, 0.1, 0, 5, 0.9, 0.5, 0.0, None)  # cells NULL with C = 0
    assert _lib.lib().pcx_sim_sweep_plan(C.byref(s), None, None, None, None) == 0
