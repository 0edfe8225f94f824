"""The single-matrix path's weighted medians (csrc/pcx_mat_select.hip, pcx_mat_hard.hip, select() and
hard_replay() of pcx_runner.cpp) on the crafted columns of matrix_median_cases.py, against the numpy
restatement (oracle.pcx_oracle.OracleCPU), on four routes:

  exact     one rank, N = 2,203 <= SEL_EXACT_MAX: k_sel_exact, the one-block replay;
  tiers     one rank, N = 8,200 (the smallest ragged-16 size above SEL_EXACT_MAX): the histogram tiers;
  shards2 / shards3   N = 2,203 over 2 and 3 virtual ranks (ThreadComm, test_matrix_gpu._sharded): unequal
            shards of more than one 1,024-row sample span plus a remainder; the exchanged passes;
  comm1     N = 2,203 on a one-rank context WITH a communicator (Oracle(devices=[0]): pcx_create_devices
            makes a one-rank RCCL communicator, as test_c_program_multi_device_context's "0"): the
            exchanged passes at world 1.

Every output is compared with parity.compare (north-star tolerances, EXACT keys exact, NaN patterns equal,
no exemption); the crafted columns of `filled`, `outcomes_raw` and `outcomes_final` bit for bit (their
medians are selections or exact averages, and test_matrix_median_cpu.py shows them stable).

What `meta` can and cannot show.  n_hard and sel_passes are totals of a call: they show that the dyadic
and thirds matrices reach the hard replay, that the deep column takes the passes its key range forces, and
that the exact route runs no histogram pass.  They do not say which event took which branch: that the
dominant columns run k_sel_argmax / k_sel_value, that `duplicates` is refused a window, that a count-mode
average takes its predecessor from an earlier bucket, is read from the code (DESIGN.md's table) and shown
only by the result being right where a slip in that branch makes it wrong."""
import numpy as np
import pytest

import golden_cases as G
import matrix_median_cases as M
import parity as P

pytestmark = pytest.mark.gpu

ROUTES = ("exact", "tiers", "shards2", "shards3", "comm1")  # (all but the first: the histogram tiers)
route_n = lambda route: M.N_TIERS if route.startswith("tiers") else M.N_SMALL


def _oracle(c, route):
    from pyconsensus_amd import Oracle

    return Oracle(devices=[0] if route == "comm1" else None, **c.oracle_kw())


def _consensus(c, route):
    """(outputs under their ABI names, info) of one case on one route."""
    if route in ("shards2", "shards3"):
        from test_matrix_gpu import _sharded

        return _sharded(np.asarray(c.R, dtype=np.float64), c.rep, c.sc, c.lo, c.hi, int(route[-1]), alpha=c.alpha,
                        int_dtype=c.int_dtype)
    o = _oracle(c, route)
    res = o.consensus()
    return {P.ABI_NAME[k]: v for k, v in G.flat_result(res).items() if k in P.ABI_NAME}, o.last_info


def _interpolate(c, route):
    from pyconsensus_amd import Oracle

    devices = {"shards2": [0, 0], "shards3": [0, 0, 0], "comm1": [0], "tiers-shards2": [0, 0]}.get(route)
    o = Oracle(devices=devices, **c.oracle_kw())
    return np.asarray(o.interpolate(o.reports), dtype=np.float64)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", list(M.KINDS))
def test_crafted_medians(gpu_lib, kind, route):
    """Kind "nan" also pins what stands BESIDE a NaN fill at N != E (found by this battery): the reference's
    this_rep / smooth_rep are fully masked numpy.ma arrays whose data is alpha, and np.dot(smooth_rep, X)
    hands the mask on only when N == E (the 4 x 4 golden case q_all_missing_scaled_col).  Otherwise it is
    the plain product: outcomes_raw = alpha * sum(F[:, c]) (394.0 at 2,203 x 32), participation_columns =
    1 - alpha * missing (-20.4), participation a plain number (-40.24), reporter_bonus relative_part *
    percent_na (pcx_matrix.hip rep_masked_plain_dot)."""
    N = route_n(route)
    c, ref = M.case(kind, N), M.reference(kind, N)
    M.preconditions(c, ref)
    ours, info = _consensus(c, route)
    print(kind, route, {k: info[k] for k in ("n_hard", "sel_passes")})
    bad, _ = P.compare(ref, ours)
    assert not bad, bad
    # selections and exact averages: no tolerance
    j = c.crafted
    assert np.all(M.bits_equal(ours["filled"][:, j], ref["filled"][:, j])), "filled"
    for k in ("outcomes_raw", "outcomes_final"):
        assert np.all(M.bits_equal(ours[k][j], ref["events." + k][j])), (k, ours[k][j], ref["events." + k][j])
    # each tier was entered
    if route == "exact":
        assert info["sel_passes"] == 0 and info["n_hard"] == 0, info
        return
    assert info["sel_passes"] > 0, info
    if kind in ("dyadic", "thirds"):  # tie-weights / tie-above: a prefix on the half -> the hard replay
        assert info["n_hard"] >= 1, info
    if kind == "negative":  # weights outside [0, 2^8): every selection of both phases replays
        assert info["n_hard"] >= 2 * len(c.crafted), info
    if kind in ("given", "none", "constant"):
        # the deep column: ceil(bits / 8) passes in each phase (matrix_median_cases.deep_min_passes: its
        # first range has 62 bits, a pass keeps one of 256 buckets, and the column's keys M +- 2^e keep
        # every kept bucket at least half full in key span, so a pass narrows by exactly 8 bits); the
        # runner stops a phase at MAX_SEL_PASSES
        need = M.deep_min_passes(c, c.cols["deep"])
        assert 2 * need <= info["sel_passes"] <= 2 * M.MAX_SEL_PASSES, (need, info)


@pytest.mark.parametrize("kind", list(M.KINDS))
def test_interpolate_alone(gpu_lib, kind):
    """Phase 1 by itself (Oracle.interpolate: no NaN fill of one column reaches another) is the
    reference's on every route, hence the same on every route at one N (the header of
    pcx_mat_select.hip: the result does not depend on the sharding)."""
    got = {}
    for route in ROUTES + ("tiers-shards2",):
        N = route_n(route)
        got[route] = _interpolate(M.case(kind, N), route)
        assert np.all(M.bits_equal(got[route], M.reference_filled(kind, N))), route
    for route in ("shards2", "shards3", "comm1"):
        assert np.all(M.bits_equal(got[route], got["exact"])), route
    assert np.all(M.bits_equal(got["tiers-shards2"], got["tiers"]))
