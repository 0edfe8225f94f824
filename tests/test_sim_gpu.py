"""The Monte Carlo simulator on the GPU: generator, metrics, summary order, whole trajectories.

Everything is compared bit for bit: the device generator against ``pcx_sim_generate_host`` (the
same inline code on the CPU, itself checked against the specification in test_sim_cpu.py), the
metrics and the summary against the numpy restatement below (written from DESIGN.md
"Simulator"), and whole trajectories against a host replay -- ``generate_host``, the C oracle's
batched consensus with the carried reputation, the numpy metrics.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULTS = dict(liar_frac=0.3, collude_frac=0.5, distort=0.1, na_frac=0.1, scaled_frac=0.25)
ROUNDS = ("reports", "scaled", "lo", "hi", "truth", "liar")


# ------------------------------------------------------------------ numpy restatement
def np_metrics(scaled, lo, hi, truth, liar, old_rep, smooth_rep, outcomes_final, scaled_tol):
    """[B][6]: correct, liar_rep_before, liar_rep_after, liars_bonus, beats, n_liars."""
    B, E = truth.shape
    with np.errstate(invalid="ignore"):
        ok = np.where(scaled != 0, np.abs(outcomes_final - truth) <= scaled_tol * (hi - lo),
                      outcomes_final == truth)  # a NaN outcome compares false
    lies = (liar & 1) == 1
    before, after = np.zeros(B), np.zeros(B)
    for i in range(liar.shape[1]):  # sequentially, in increasing i
        before = np.where(lies[:, i], before + old_rep[:, i], before)
        after = np.where(lies[:, i], after + smooth_rep[:, i], after)
    with np.errstate(invalid="ignore"):
        beats = (after > before).astype(np.float64)
    return np.stack([ok.sum(axis=1).astype(np.float64) / float(E), before, after, after - before, beats,
                     lies.sum(axis=1).astype(np.float64)], axis=1)


def np_summary(m):
    """Mean over the rounds in the library's order: thread tau of 256 adds rounds tau, tau + 256,
    ... from 0.0; a tree with strides 128 .. 1 (s[tau] += s[tau + stride]); then / B."""
    B = m.shape[0]
    s = np.zeros((256, m.shape[1]))
    for b0 in range(0, B, 256):
        chunk = m[b0:b0 + 256]
        s[:len(chunk)] = s[:len(chunk)] + chunk
    stride = 128
    while stride >= 1:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        stride //= 2
    return s[0] / float(B)


def same_bits(a, b):
    """Equal bit for bit, NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a.view(np.uint64)[~nan] == b.view(np.uint64)[~nan]).all())


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items() if not k.startswith("_")}


# ------------------------------------------------------------------ generation
@pytest.mark.parametrize("shape", [(1, 1, 1, 0), (3, 7, 5, 2), (5, 64, 32, 1), (2, 65, 33, 0), (4, 50, 20, 3),
                                   (1025, 3, 3, 1), (257, 50, 20, 0)])
def test_generate_matches_host(gpu_lib, shape):
    from pyconsensus_amd.simulate import generate, generate_host

    B, N, E, t = shape
    for seed in (20261019, (0xC0FFEE << 32) | 0x1234567):
        dev = _np(generate(B, N, E, t=t, seed=seed, **DEFAULTS))
        host = generate_host(B, N, E, t=t, seed=seed, **DEFAULTS)
        for name in ROUNDS:
            assert same_bits(dev[name], host[name]), (name, seed)


def test_generate_tiles_events_and_reporter_chunks(gpu_lib):
    """More events than one LDS tile (256) and more reporters than one work item (1024), both
    with a ragged tail: the paths a Monte Carlo shape never takes."""
    from pyconsensus_amd.simulate import generate, generate_host

    for B, N, E in ((2, 3, 515), (2, 1030, 3)):
        dev = _np(generate(B, N, E, t=1, seed=77, **DEFAULTS))
        host = generate_host(B, N, E, t=1, seed=77, **DEFAULTS)
        for name in ROUNDS:
            assert same_bits(dev[name], host[name]), (name, N, E)


# ------------------------------------------------------------------ metrics and summary
def test_metrics_on_hand_built_rounds(gpu_lib):
    from pyconsensus_amd.simulate import metrics

    tol = 0.1
    scaled = np.array([[0, 0, 1, 1], [0, 1, 0, 1], [1, 1, 0, 0]], dtype=np.uint8)
    lo = np.array([[1, 1, 0, -50], [1, -100, 1, 3], [0, 10, 1, 1]], dtype=np.float64)
    hi = np.array([[2, 2, 40, 150], [2, 60, 2, 4], [40, 20, 2, 2]], dtype=np.float64)
    truth = np.array([[1, 2, 10, 25.5], [2, -20.25, 1, 3.5], [10, 15, 2, 1]], dtype=np.float64)
    edge = 10.0 + tol * (40.0 - 0.0)  # |outcome - truth| == scaled_tol * (hi - lo) exactly
    assert abs(edge - 10.0) == tol * 40.0
    outcomes = np.array([[1, 1.5, edge, 25.5 + 21.0],          # right, ambiguous, on the boundary, outside
                         [np.nan, -20.25, 1, np.nan],          # NaN binary, exact, right, NaN scaled
                         [np.nextafter(edge, 99.0), 15.9, 2, 1]], dtype=np.float64)  # just past the boundary
    liar = np.array([[1, 0, 3, 0, 1], [0, 0, 0, 0, 0], [3, 1, 1, 3, 1]], dtype=np.uint8)
    rng = np.random.default_rng(5)
    old = rng.random((3, 5)) / 3.0
    smooth = rng.random((3, 5)) / 3.0
    got = _np(metrics(dict(scaled=scaled, lo=lo, hi=hi, truth=truth, liar=liar), old, smooth, outcomes, tol))
    want = np_metrics(scaled, lo, hi, truth, liar, old, smooth, outcomes, tol)
    assert want[:, 0].tolist() == [0.5, 0.5, 0.75] and want[:, 5].tolist() == [3.0, 0.0, 5.0]
    assert want[1, 1:5].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert same_bits(got["metrics"], want)
    assert same_bits(got["summary"], np_summary(want))


@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000])
def test_summary_order(gpu_lib, B):
    from pyconsensus_amd.simulate import metrics

    rng = np.random.default_rng(B)
    N, E = 6, 3
    rounds = dict(scaled=np.zeros((B, E), np.uint8), lo=np.ones((B, E)), hi=np.full((B, E), 2.0),
                  truth=rng.integers(1, 3, (B, E)).astype(np.float64), liar=rng.integers(0, 4, (B, N)).astype(np.uint8))
    old = rng.random((B, N)) * np.exp(rng.normal(0, 6, (B, N)))  # magnitudes apart: the order shows
    smooth = rng.random((B, N)) * np.exp(rng.normal(0, 6, (B, N)))
    outcomes = rng.integers(1, 3, (B, E)).astype(np.float64)
    got = _np(metrics(rounds, old, smooth, outcomes))
    want = np_metrics(rounds["scaled"], rounds["lo"], rounds["hi"], rounds["truth"], rounds["liar"], old, smooth,
                      outcomes, 0.1)
    assert same_bits(got["metrics"], want)
    assert same_bits(got["summary"], np_summary(want))
    if B >= 255:  # (the order is observable: another one gives other bits)
        assert not same_bits(np_summary(want), want.sum(axis=0) / float(B))


# ------------------------------------------------------------------ whole trajectories
def _replay(B, N, E, T, seed, scaled_tol=0.1, **p):
    """The trajectory on the host: generate_host, the C oracle with the carried reputation, numpy metrics."""
    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd.simulate import generate_host

    rep, ms, ss = None, [], []
    for t in range(T):
        g = generate_host(B, N, E, t=t, seed=seed, **p)
        c = OC.batched(g["reports"], g["scaled"], g["lo"], g["hi"], rep, threads=8,
                       want=("old_rep", "smooth_rep", "outcomes_final"))
        m = np_metrics(g["scaled"], g["lo"], g["hi"], g["truth"], g["liar"], c["old_rep"], c["smooth_rep"],
                       c["outcomes_final"], scaled_tol)
        ms.append(m)
        ss.append(np_summary(m))
        rep = c["smooth_rep"]
    return {"metrics": np.stack(ms), "summary": np.stack(ss), "reputation": rep, "rounds": g, "outputs": c}


@pytest.mark.parametrize("shape,extra", [((257, 50, 20, 3), {}),       # one wavefront per round
                                         ((9, 65, 33, 2), {}),         # one workgroup per round
                                         ((3, 1, 1, 2), {"na_frac": 0.0})])
def test_trajectory_matches_host_replay(gpu_lib, shape, extra):
    import torch

    from pyconsensus_amd.simulate import simulate

    B, N, E, T = shape
    p = dict(DEFAULTS, **extra)
    r = simulate(B, N, E, T, seed=42, keep_rounds=True, keep_outputs=True, **p)
    torch.cuda.synchronize()
    want = _replay(B, N, E, T, 42, **p)
    assert r["metrics"].shape == (T, B, 6) and r["summary"].shape == (T, 6)
    for name in ("metrics", "summary", "reputation"):
        assert same_bits(r[name].cpu().numpy(), want[name]), name
    for name in ROUNDS:
        assert same_bits(r["rounds"][name].cpu().numpy(), want["rounds"][name]), name
    for name in ("smooth_rep", "outcomes_final", "old_rep"):
        assert same_bits(r["outputs"][name].cpu().numpy(), want["outputs"][name]), name
    assert same_bits(r["outputs"]["smooth_rep"].cpu().numpy(), r["reputation"].cpu().numpy())
    if B == 257:  # the default population: the consensus mostly finds the truth
        assert 0.5 < float(r["summary"][0, 0]) <= 1.0 and abs(float(r["summary"][0, 5]) - 0.3 * N) < 1.0


def test_trajectory_takes_a_starting_reputation(gpu_lib):
    import torch

    from oracle import pcx_oracle_c as OC
    from pyconsensus_amd.simulate import generate_host, simulate

    B, N, E = 5, 50, 20
    rep0 = np.random.default_rng(1).integers(1, 100, (B, N)).astype(np.float64)
    r = simulate(B, N, E, 1, seed=8, reputation=rep0, keep_outputs=True, **DEFAULTS)
    torch.cuda.synchronize()
    g = generate_host(B, N, E, t=0, seed=8, **DEFAULTS)
    c = OC.batched(g["reports"], g["scaled"], g["lo"], g["hi"], rep0, want=("old_rep", "smooth_rep"))
    assert same_bits(r["outputs"]["old_rep"].cpu().numpy(), c["old_rep"])
    assert same_bits(r["reputation"].cpu().numpy(), c["smooth_rep"])


def test_determinism_and_seed(gpu_lib):
    import torch

    from pyconsensus_amd.simulate import simulate

    def run(seed):
        r = simulate(300, 50, 20, 2, seed=seed, keep_rounds=True, **DEFAULTS)
        torch.cuda.synchronize()
        return ({k: r[k].cpu().numpy() for k in ("metrics", "summary", "reputation")},
                r["rounds"]["reports"].cpu().numpy())

    a, ra = run(7)
    b, rb = run(7)
    c, rc = run(8)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert ra.tobytes() == rb.tobytes()
    assert not same_bits(ra, rc) and not same_bits(a["metrics"], c["metrics"])


def test_work_buffers_grow_and_are_released(gpu_lib):
    """The context's work buffers serve a larger shape after a smaller one, and a call after
    pcx_release_workspace allocates them again: the same bytes every time."""
    import torch

    from pyconsensus_amd import _lib
    from pyconsensus_amd.simulate import simulate

    def run(B):
        r = simulate(B, 50, 20, 2, seed=5, **DEFAULTS)
        torch.cuda.synchronize()
        return r["metrics"].cpu().numpy().tobytes() + r["reputation"].cpu().numpy().tobytes()

    small, large = run(3), run(300)
    _lib.check(gpu_lib.pcx_release_workspace(_lib.context(torch.cuda.current_device())))
    assert run(300) == large and run(3) == small


def test_rejections(gpu_lib):
    from pyconsensus_amd._lib import PcxError
    from pyconsensus_amd.simulate import simulate

    for kw in (dict(algorithm="k-means"), dict(algorithm="cokurtosis"), dict(T=0), dict(liar_frac=1.5),
               dict(scaled_tol=-1.0)):
        with pytest.raises(PcxError):
            simulate(4, 5, 3, **kw)
    with pytest.raises(NotImplementedError):
        simulate(4, 5, 3, algorithm="no-such")


def test_consensus_batched_unchanged_on_generated_rounds(gpu_lib):
    import torch

    from pyconsensus_amd import consensus_batched
    from pyconsensus_amd.simulate import generate, simulate

    B, N, E = 257, 50, 20
    g = generate(B, N, E, t=0, seed=3, **DEFAULTS)
    direct = consensus_batched(g["reports"], None, g["scaled"], g["lo"], g["hi"])
    sim = simulate(B, N, E, 1, seed=3, keep_outputs=True, **DEFAULTS)
    torch.cuda.synchronize()
    for name, x in sim["outputs"].items():
        assert same_bits(x.cpu().numpy(), direct[name].cpu().numpy()), name
    assert set(sim["outputs"]) == {k for k in direct if not k.startswith("_")}


def test_other_algorithms_run(gpu_lib):
    """The non-PCA algorithms the simulator admits reach the consensus with their parameters."""
    import torch

    from pyconsensus_amd import consensus_batched
    from pyconsensus_amd.simulate import generate, simulate

    B, N, E = 33, 20, 8
    g = generate(B, N, E, t=0, seed=9, **DEFAULTS)
    for alg, kw in (("big-five", dict(max_components=3)), ("fixed-variance", dict(variance_threshold=0.8)),
                    ("hierarchical", dict(hierarchy_threshold=0.4)), ("clusterfeck", {}), ("absolute", {})):
        direct = consensus_batched(g["reports"], None, g["scaled"], g["lo"], g["hi"], algorithm=alg, **kw)
        sim = simulate(B, N, E, 1, seed=9, algorithm=alg, keep_outputs=True, **dict(DEFAULTS, **kw))
        torch.cuda.synchronize()
        for name in ("smooth_rep", "outcomes_final", "components"):
            assert same_bits(sim["outputs"][name].cpu().numpy(), direct[name].cpu().numpy()), (alg, name)
