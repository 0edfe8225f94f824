"""GPU parity of the single-matrix pipeline (csrc/pcx_matrix.hip and pcx_mat_*.hip via pipeline.py).

* golden vectors (KATs, mixed shapes, synthetic 50x20, C2 1000x100) forced through
  the matrix path, north_star tolerances, near-tie rounds counted separately;
* larger matrices against the numpy CPU oracle run on the box;
* virtual row shards (2 and 3 ranks in one process) against the 1-rank result.

The golden cases are all far below SEL_EXACT_MAX rows on one rank: of the weighted medians' code they reach
only k_sel_exact; the histogram tiers, the exchanged passes and the hard replay are covered branch by branch
by test_matrix_median_gpu.py (crafted columns, matrix_median_cases.py).
"""
import numpy as np
import pytest

import golden_cases as G
import parity as P

pytestmark = pytest.mark.gpu


def run_matrix(case, **kw):
    from pyconsensus_amd.pipeline import consensus_matrix

    R = case["in_reports"]
    bk = {}
    if bool(case["in_has_bounds"]):
        bk = dict(scaled=case["in_scaled"], lo=case["in_lo"], hi=case["in_hi"])
    rep = case["in_reputation"] if bool(case["in_has_rep"]) else None
    ev, ag, meta = consensus_matrix(R, rep, catch_tolerance=float(case["in_catch_tolerance"]),
                                    alpha=float(case["in_alpha"]), int_dtype=bool(case["in_int_dtype"]),
                                    matrices=True, **bk, **kw)
    out = {k: v.cpu().numpy() for k, v in list(ev.items()) + list(ag.items())}
    out["participation"] = np.array(meta["participation"])
    out["avg_certainty"] = np.array(meta["avg_certainty"])
    out["branch"] = np.array(meta["branch"])
    return out


def _suite(cases):
    observed, ran = {}, []
    for name, case in cases:
        if name in P.EXCLUDED:
            continue
        ran.append(name)
        kind, _ = P.mismatch_kind(case, run_matrix(case))
        if kind:
            observed[name] = kind
    return observed, ran


def test_matrix_golden_kat(gpu_lib):
    P.assert_known("matrix", *_suite(G.kat().items()))


def test_matrix_golden_mixed(gpu_lib):
    P.assert_known("matrix", *_suite(G.mixed().items()))


def test_matrix_golden_synth(gpu_lib):
    st = G.synth()
    P.assert_known("matrix", *_suite(("s%03d" % b, G.unstack(st, b)) for b in range(0, st["branch"].shape[0], 5)))


def test_matrix_golden_c2(gpu_lib):
    """Config C2 (1000 x 100, 10% NA, mixed bounds) through the drop-in Oracle."""
    from pyconsensus_amd import Oracle

    case = G.c2()
    res = Oracle(**G.oracle_args(case)).consensus()
    ours = {P.ABI_NAME[k]: v for k, v in G.flat_result(res).items() if k in P.ABI_NAME}
    bad, sign = P.compare(case, ours)
    assert not bad, bad


_REF = {}


def _big_case(name):
    """Inputs and the numpy oracle's result of a large case (computed once per session).

    C4: BASELINE config C4 exactly as SURVEY.md 8(d) specifies it -- 100k x 1k, integer
    reputations U[1, 99], seed 2 -- so exact-half weighted-median prefixes occur and must be
    resolved the reference's way.  C5r: the C5 recipe (GPU generator, seed 3, eight shards,
    reputation=None: every interpolation weight of a column is the same double) at 250k x 1024.
    C5r_1M: the same recipe at C5's own row count, 1M x 1024 -- there every token is
    int(1e-6 * 1e6) = 1 (__init__.py:146) and every median is a 1M-row equal-weight walk
    (:303, :520-523); the restatement needs ~60 GB of host memory and a few minutes.
    C5w: the recipe at C5's own event width, 250k x 4096 -- the 6-digit int8 mixed block over
    ~3,072 grid events x ~1,024 general ones (:326), the E = 4096 power iteration (:330-337) and
    the rank rule's `old` ties among 3,072 binary events under equal weights (:489-498)."""
    if name in _REF:
        return _REF[name]
    from oracle.pcx_oracle import OracleCPU
    from pyconsensus_amd import synthetic

    if name == "C4":
        R, sc, lo, hi, rep = synthetic.matrix(100_000, 1000, seed=2)
    elif name in ("C5r", "C5r_1M", "C5w"):
        import torch

        N = 1_000_000 if name == "C5r_1M" else 250_000
        E = 4096 if name == "C5w" else 1024
        Rd, scd, lod, hid, _ = synthetic.matrix_device(N, E, seed=3, n_shards=8, device="cuda:0")
        R, sc, lo, hi, rep = Rd.cpu().numpy(), scd.cpu().numpy().astype(bool), lod.cpu().numpy(), hid.cpu().numpy(), None
        del Rd
        torch.cuda.empty_cache()
    else:  # (N, E) or (N, E, None): reputation=None -- tokens int(1e6 / N) <= 63 from N = 15,874, so the
        # binary events take the int8 covariance and the compact passes (k_gemv2_c / k_outcomes_c)
        N, E = name[:2]
        R, sc, lo, hi, rep = synthetic.matrix(N, E, seed=N + E)
        if len(name) == 3 and name[2] is None:
            rep = None
        elif len(name) == 3 and name[2] == "nomiss":
            # a few scaled events with no missing report: phase 1 selects nothing for them, so phase
            # 2's first pass over them counts every element itself while the others take phase 1's
            # bucket counts (k_sel_hist, vsave) -- both kinds in one launch
            idx = np.flatnonzero(sc)[:3]
            for j in idx:
                col = R[:, j]
                col[np.isnan(col) | (col == 0.0)] = 0.5 * (lo[j] + hi[j])
        elif len(name) == 3:
            rep = _signed_reputation(rep, name[2], seed=N)
    b = synthetic.bounds_list(sc, lo, hi)
    ref = G.flat_result(OracleCPU(reports=R, event_bounds=b, reputation=rep).consensus())
    _REF[name] = (R, sc, lo, hi, rep, ref)
    return _REF[name]


def _signed_reputation(rep, kind, seed):
    """Reputations with negative entries (the reference takes any numbers: rep / sum(rep) keeps
    the signs, __init__.py:142-145, and smooth_rep inherits them, :472), so the weighted medians'
    weights leave [0, 1]: "neg" flips 10% of them -- beyond the exact weight limbs' [0, 2^8) range,
    so the selection must replay those events in the reference's order (k_sel_start's weight-range
    test).  (A weight of 2^8 or more needs a total far below the entries, i.e. signed tokens whose
    covariance is indefinite with nearly equal |eigenvalues| -- svd's first vector is then not
    determined to 1e-9 and the case tests LAPACK, not the selection.)"""
    rng = np.random.default_rng(seed)
    r = np.asarray(rep, dtype=np.float64).copy()
    flip = rng.random(r.size) < 0.1
    r[flip] = -r[flip]
    return r


def _record(name, world, info):
    """Keep the large cases' selection statistics (n_hard, sel_passes) beside the run's logs."""
    import json
    import os

    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "large_cases.jsonl"), "a") as f:
            f.write(json.dumps({"case": name, "world": world, "n_hard": info.get("n_hard"),
                                "sel_passes": info.get("sel_passes"), "branch": info.get("branch"),
                                "pi_iters": info.get("pi_iters"), "grid_events": info.get("grid_events"),
                                "mixed_int8": info.get("mixed_int8")}) + "\n")
    except OSError:
        pass


def _flat_gpu(ev, ag, meta):
    out = {k: v.cpu().numpy() for k, v in list(ev.items()) + list(ag.items())}
    out["participation"] = np.array(meta["participation"])
    out["avg_certainty"] = np.array(meta["avg_certainty"])
    return out


def _sharded(R, rep, sc, lo, hi, world, **kw):
    """consensus_matrix over `world` virtual ranks (ThreadComm, one GPU); rows concatenated.
    (kw: further arguments of consensus_matrix -- test_matrix_median_gpu.py passes alpha, int_dtype.)"""
    import threading

    import torch
    from pyconsensus_amd.pipeline import ThreadComm, ThreadGroup, consensus_matrix, shard_rows

    N = R.shape[0]
    grp = ThreadGroup(world)
    res, errs = [None] * world, []

    def worker(r):
        try:
            torch.cuda.set_device(0)
            off, cnt = shard_rows(N, world, r)
            comm = ThreadComm(grp, r)
            ev, ag, meta = consensus_matrix(R[off:off + cnt], rep, sc, lo, hi, comm=comm, n_total=N, row_offset=off,
                                            matrices=True, **kw)
            res[r] = (_flat_gpu(ev, ag, meta), meta)
            comm.close()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs
    out = dict(res[0][0])
    for k in list(out):
        if out[k].ndim >= 1 and out[k].shape[0] == res[0][0]["smooth_rep"].shape[0] and k not in _abi_events():
            out[k] = np.concatenate([res[r][0][k] for r in range(world)])
    for r in range(1, world):  # event outputs identical on every rank
        for k in _abi_events():
            np.testing.assert_array_equal(res[r][0][k], res[0][0][k], err_msg=k)
    return out, res[0][1]


def _abi_events():
    from pyconsensus_amd import _abi

    return _abi.MAT_OUTPUT_EVENTS


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", [(3000, 150), (20000, 400), (20008, 400), (16648, 2048, None), (20000, 80, "neg"),
                                  (12000, 60, "nomiss"), "C4", "C5r", "C5r_1M", "C5w"],
                         ids=["3000x150", "20000x400", "20008x400_ragged16",
                              "16648x2048_repNone_ragged16_empty_chunks", "20000x80_negative_rep",
                              "12000x60_scaled_without_missing",
                              "C4_100k_x_1k_intrep",
                              "C5recipe_250k_x_1024_repNone",
                              "C5r_1M_x_1024_repNone", "C5width_250k_x_4096_repNone"])
@pytest.mark.parametrize("world", [1, 2])
def test_matrix_vs_numpy_oracle(gpu_lib, case, world):
    """Against the numpy restatement run on the box, no exemption: binary outcomes and the
    filled matrix exact, everything continuous within 1e-9.  world=2: two virtual row shards."""
    from pyconsensus_amd import Oracle, synthetic

    R, sc, lo, hi, rep, ref = _big_case(case)
    if world == 1:
        b = synthetic.bounds_list(sc, lo, hi)
        o = Oracle(reports=R.copy(), event_bounds=b, reputation=rep)
        res = o.consensus()
        ours = {P.ABI_NAME[k]: v for k, v in G.flat_result(res).items() if k in P.ABI_NAME}
        info = o.last_info
    else:
        ours, info = _sharded(R, rep, sc, lo, hi, world)
    print(case, world, {k: info[k] for k in ("n_hard", "sel_passes") if k in info})
    bad, sign = P.compare(ref, ours)
    if case in ("C4", "C5r", "C5r_1M", "C5w"):
        _record(case, world, info)
    assert not bad, bad
    if case == "C5r_1M" and world == 1:  # the drop-in's tokens: int(1e-6 * 1e6) = 1 for every reporter (:146)
        assert set(o.reptokens) == {1}
    if case in ("C4", "C5w"):
        # C4: integer reputations, tokens int(r / sum(r) 1e6) in [0, 19] -- non-uniform tokens through
        # the int8 blocks (the mixed block's digits of tok * w); C5w: the 3,072-event grid
        assert info.get("mixed_int8", 0) & 1 and info.get("grid_events", 0) > 0, info


def test_virtual_shards_match_single(gpu_lib):
    """2 and 3 row shards (ThreadComm, one GPU) reproduce the 1-rank result."""
    import threading

    import torch
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.pipeline import ThreadComm, ThreadGroup, consensus_matrix, shard_rows

    N, E = 5000, 120
    R, sc, lo, hi, rep = synthetic.matrix(N, E, seed=17)
    ev1, ag1, m1 = consensus_matrix(R, rep, sc, lo, hi)
    ref_ev = {k: v.cpu().numpy() for k, v in ev1.items()}
    ref_ag = {k: v.cpu().numpy() for k, v in ag1.items()}
    for world in (2, 3):
        grp = ThreadGroup(world)
        res = [None] * world
        errs = []

        def worker(r):
            try:
                torch.cuda.set_device(0)
                off, cnt = shard_rows(N, world, r)
                ev, ag, meta = consensus_matrix(R[off:off + cnt], rep, sc, lo, hi, comm=ThreadComm(grp, r),
                                                n_total=N, row_offset=off)
                res[r] = ({k: v.cpu().numpy() for k, v in ev.items()},
                          {k: v.cpu().numpy() for k, v in ag.items()}, meta["branch"])
            except Exception as e:  # pragma: no cover
                errs.append(e)
                grp.barrier.abort()

        th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
        [x.start() for x in th]
        [x.join() for x in th]
        assert not errs, errs
        for r in range(world):
            ev, ag, br = res[r]
            assert br == m1["branch"]
            for k in ref_ev:
                np.testing.assert_allclose(ev[k], ref_ev[k], rtol=1e-12, atol=1e-14, err_msg=k)
            for k in ("outcomes_adjusted", "outcomes_final"):
                np.testing.assert_array_equal(ev[k], ref_ev[k], err_msg=k)
        for k in ref_ag:
            got = np.concatenate([res[r][1][k] for r in range(world)])
            np.testing.assert_allclose(got, ref_ag[k], rtol=1e-12, atol=1e-14, err_msg=k)
