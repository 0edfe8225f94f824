"""On-device Monte Carlo simulator: draw random rounds, run consensus on them, score them.

The Simulator.jl-style driver of the batched regime (README.rst:52-56) without the host in
the loop.  Per timestep libpcx generates B rounds of N x E reports on the device (a
counter-based Philox4x32-10 generator, csrc/pcx_sim.h; DESIGN.md "Simulator" is its
specification), runs :func:`pyconsensus_amd.consensus_batched`'s kernel on them, reduces each
round to :data:`METRICS` against the truth it drew, and carries ``smooth_rep`` into the next
timestep's reputation.

    python -m pyconsensus_amd.simulate --rounds 65536 --timesteps 8 --seed 1

prints the per-timestep means of the metrics as JSON.

A study is a curve or a grid, not a point: :func:`sweep` runs cells of different shapes, rates and
seeds in one call (``pcx_simulate_sweep_f64``), each cell byte for byte its own
:func:`simulate`, and :func:`grid` builds the cell list of a cartesian product.  On the command
line a comma list for a shape or a rate (``--liars 0.1,0.2,0.3 --reporters 20,50``) runs the grid.

A study's result has error bars: :func:`study` is :func:`sweep` plus the twelve :data:`DETAIL` metrics
of every round and timestep (did the consensus punish the liars? what kind of wrong was a wrong
outcome?), every value's per-cell ``{n, mean, var, min, max}`` and, against a base cell, the paired
differences in which common random numbers pay off (``pcx_simulate_study_f64``).
``--stats`` and ``--paired`` print them.

"k-means" is simulated where ``kmeans_restarts`` is given (``--algorithm k-means`` on the command line):
its restarts' initial code books are drawn on the device from a further stream of the generator
(:func:`kmeans_books`, with the CPU twin :func:`kmeans_books_host`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _device, _lib
from .batched import clusterfeck_threshold

METRICS = ("correct", "liar_rep_before", "liar_rep_after", "liars_bonus", "beats", "n_liars")
DETAIL = ("correct_binary", "correct_scaled", "indeterminate", "flipped", "nan_outcomes", "scaled_err",
          "tp", "fn", "fp", "tn", "mcc", "colluder_rep_after")
VALUES = METRICS + DETAIL
STATS = ("n", "mean", "var", "min", "max")
PAIRED = ("n", "mean", "var")
ROUND_FIELDS = tuple(name for name, _, _ in _abi.SIM_ROUNDS)

_NP = {"f8": np.float64, "u1": np.uint8, "i4": np.int32}


def _sim(B, N, E, T, seed, liar_frac, collude_frac, distort, na_frac, scaled_frac, scaled_tol=0.1,
         algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
         hierarchy_threshold=0.5, cluster_threshold=None, reputation0=None):
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    B, N, E, T = int(B), int(N), int(E), int(T)
    cthr = clusterfeck_threshold(E) if cluster_threshold is None and E >= 1 else float(cluster_threshold or 0.0)
    mc = int(max_components) if E >= int(max_components) else E  # __init__.py:134-137
    return _abi.Sim(B, N, E, T, int(seed) & 0xFFFFFFFFFFFFFFFF, float(liar_frac), float(collude_frac),
                    float(distort), float(na_frac), float(scaled_frac), float(scaled_tol),
                    float(catch_tolerance), float(alpha), alg, mc, float(variance_threshold),
                    float(hierarchy_threshold), cthr, reputation0)


def _torch_dtype(t, dt):
    return {"f8": t.float64, "u1": t.uint8, "i4": t.int32}[dt]


def _device_rounds(t, dev, B, N, E):
    """Empty device tensors of one timestep's rounds and the pcx_sim_rounds that points at them."""
    rounds, c = {}, _abi.SimRounds()
    for name, kind, dt in _abi.SIM_ROUNDS:
        x = t.empty(_abi.out_shape(kind, B, N, E), dtype=_torch_dtype(t, dt), device=dev)
        rounds[name] = x
        setattr(c, name, x.data_ptr())
    return rounds, c


def generate_host(B, N, E, t=0, seed=0, liar_frac=0.3, collude_frac=0.5, distort=0.1, na_frac=0.1,
                  scaled_frac=0.25):
    """The rounds of timestep ``t`` drawn on the CPU (``pcx_sim_generate_host``; no GPU needed).

    Returns numpy arrays ``reports (B,N,E)``, ``scaled (B,E) u8``, ``lo``, ``hi``, ``truth (B,E)``
    and ``liar (B,N) u8`` (bit 0: liar, bit 1: a liar that colludes) -- bit for bit what
    :func:`generate` writes on the device."""
    s = _sim(B, N, E, max(1, int(t) + 1), seed, liar_frac, collude_frac, distort, na_frac, scaled_frac)
    rounds, c = {}, _abi.SimRounds()
    for name, kind, dt in _abi.SIM_ROUNDS:
        a = np.empty(_abi.out_shape(kind, max(int(B), 0), max(int(N), 0), max(int(E), 0)), dtype=_NP[dt])
        rounds[name] = a
        setattr(c, name, a.ctypes.data)
    _lib.check(_lib.lib().pcx_sim_generate_host(C.byref(s), int(t), C.byref(c)))
    return rounds


def generate(B, N, E, t=0, seed=0, liar_frac=0.3, collude_frac=0.5, distort=0.1, na_frac=0.1,
             scaled_frac=0.25, device=None):
    """The rounds of timestep ``t`` drawn on the device: a dict of torch tensors named like
    :func:`generate_host`'s arrays.  Asynchronous on torch's current stream."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    s = _sim(B, N, E, max(1, int(t) + 1), seed, liar_frac, collude_frac, distort, na_frac, scaled_frac)
    rounds, c = _device_rounds(tc, dev, int(B), int(N), int(E))
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_generate_f64(h, C.byref(s), int(t), C.byref(c)))
    return rounds


def metrics(rounds, old_rep, smooth_rep, outcomes_final, scaled_tol=0.1, device=None):
    """Score rounds that ran: ``metrics (B,6)`` (:data:`METRICS`) and their means ``summary (6,)``
    as device tensors (``pcx_sim_metrics_f64``).  ``rounds`` holds ``scaled``, ``lo``, ``hi``,
    ``truth`` and ``liar`` as :func:`generate` returns them."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    c, keep = _abi.SimRounds(), []
    for name, _, dt in _abi.SIM_ROUNDS:
        if name != "reports":
            x = _device.as_device(rounds[name], _torch_dtype(tc, dt), dev)
            keep.append(x)
            setattr(c, name, x.data_ptr())
    B, N = keep[-1].shape
    E = keep[0].shape[1]
    old, smooth, outc = (_device.as_device(x, tc.float64, dev) for x in (old_rep, smooth_rep, outcomes_final))
    if tuple(old.shape) != (B, N) or tuple(smooth.shape) != (B, N) or tuple(outc.shape) != (B, E):
        raise ValueError("old_rep / smooth_rep must be (B, N) and outcomes_final (B, E)")
    s = _sim(B, N, E, 1, 0, 0.0, 0.0, 0.0, 0.0, 0.0, scaled_tol=scaled_tol)
    m = tc.empty((B, _abi.SIM_NMETRICS), dtype=tc.float64, device=dev)
    sm = tc.empty((_abi.SIM_NMETRICS,), dtype=tc.float64, device=dev)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_metrics_f64(h, C.byref(s), C.byref(c), old.data_ptr(), smooth.data_ptr(),
                                              outc.data_ptr(), m.data_ptr(), sm.data_ptr()))
    return {"metrics": m, "summary": sm, "_inputs": (keep, old, smooth, outc)}


def simulate(B, N=50, E=20, T=1, seed=0, liar_frac=0.3, collude_frac=0.5, distort=0.1, na_frac=0.1,
             scaled_frac=0.25, scaled_tol=0.1, reputation=None, algorithm="PCA", catch_tolerance=0.1,
             alpha=0.1, max_components=5, variance_threshold=0.9, hierarchy_threshold=0.5,
             cluster_threshold=None, keep_rounds=False, keep_outputs=False, device=None, kmeans_restarts=None,
             tall=False):
    """T timesteps of B random N x E rounds on the GPU: generate, consensus, score, carry.

    Timestep t draws its rounds (liars stay the same people through the trajectory), runs the
    batched consensus with the previous timestep's ``smooth_rep`` as reputation (``reputation``
    (B, N) or None = uniform at t = 0), and scores every round against the drawn truth.

    Returns a dict of device tensors: ``metrics (T,B,6)`` (columns :data:`METRICS`), ``summary
    (T,6)`` (their means over the rounds, in an order fixed by the library: the same bytes
    whatever the launch geometry) and ``reputation (B,N)``, the last ``smooth_rep``.
    ``keep_rounds`` adds ``rounds`` (the last timestep's, as :func:`generate`), ``keep_outputs``
    adds ``outputs`` (the last timestep's consensus outputs, as ``consensus_batched``).

    Stream semantics are ``consensus_batched``'s: rounds up to 256 x 64 are asynchronous on
    torch's current stream with no host in the loop, "hierarchical" and "clusterfeck" included
    (one workgroup per round above 64 x 32) -- synchronise before reading on the host; "cokurtosis"
    is refused (it needs caller scores), and so is "k-means" unless ``kmeans_restarts`` is given.

    ``kmeans_restarts`` (an int >= 1; None = today's refusal): "k-means" runs, its initial code books
    drawn on the device every timestep from a further stream of the generator
    (``pcx_simulate_kmeans_f64``) -- :func:`kmeans_books` shows them, and timestep t
    equals ``consensus_batched(kmeans_init=kmeans_books(...))`` on :func:`generate`'s rounds.

    ``tall=True`` (``pcx_simulate_tall_f64``): the consensus step is
    ``consensus_batched(..., tall=True)`` -- rounds of 257..1024 reporters that ``batched.route(N, E,
    algorithm, tall=True)`` calls ``"tall"`` run one asynchronous launch per timestep, with no host in
    the loop, instead of the round scheduler.  It is what a tall cell of ``sweep(..., tall=True)`` is
    compared against.  Not with ``kmeans_restarts``."""
    if tall and kmeans_restarts is not None:
        raise ValueError("tall=True does not take kmeans_restarts (k-means stays within 256 reporters)")
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    rep = _device.as_device(reputation, tc.float64, dev)
    B, N, E, T = int(B), int(N), int(E), int(T)
    if rep is not None and tuple(rep.shape) != (B, N):
        raise ValueError("reputation must be (B, N)")
    s = _sim(B, N, E, T, seed, liar_frac, collude_frac, distort, na_frac, scaled_frac, scaled_tol, algorithm,
             catch_tolerance, alpha, max_components, variance_threshold, hierarchy_threshold, cluster_threshold,
             _device.ptr(rep))
    if min(B, N, E, T) < 0:  # (libpcx refuses the rest; the output shapes below need this much)
        raise ValueError("simulate: negative shape (B=%d N=%d E=%d T=%d)" % (B, N, E, T))
    out = {"metrics": tc.empty((T, B, _abi.SIM_NMETRICS), dtype=tc.float64, device=dev),
           "summary": tc.empty((T, _abi.SIM_NMETRICS), dtype=tc.float64, device=dev),
           "reputation": tc.empty((B, N), dtype=tc.float64, device=dev)}
    res = _abi.SimResult()
    res.metrics, res.summary, res.reputation = (out[k].data_ptr() for k in ("metrics", "summary", "reputation"))
    if keep_rounds:
        out["rounds"], res.last = _device_rounds(tc, dev, B, N, E)
    if keep_outputs:
        outs = {}
        for name, kind, dt in _abi.BATCH_OUTPUTS:
            if name in ("original", "filled"):
                continue
            outs[name] = tc.empty(_abi.out_shape(kind, B, N, E), dtype=_torch_dtype(tc, dt), device=dev)
            setattr(res.last_out, name, outs[name].data_ptr())
        out["outputs"] = outs
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    if tall:
        _lib.check(_lib.lib().pcx_simulate_tall_f64(h, C.byref(s), C.byref(res)))
    elif kmeans_restarts is None:
        _lib.check(_lib.lib().pcx_simulate_f64(h, C.byref(s), C.byref(res)))
    else:
        _lib.check(_lib.lib().pcx_simulate_kmeans_f64(h, C.byref(s), int(kmeans_restarts), C.byref(res)))
    out["_inputs"] = (rep,)  # alive until the caller syncs
    return out


def kmeans_books_host(B, N, t=0, seed=0, restarts=_abi.KMEANS_RESTARTS):
    """The initial k-means code books of timestep ``t`` drawn on the CPU (``pcx_sim_kmeans_books_host``;
    no GPU needed): int32 ``(B, restarts, k)`` with k = ceil(sqrt(N)), every book k distinct rows of
    [0, N) -- bit for bit what :func:`kmeans_books` writes on the device and what
    ``simulate(algorithm="k-means", kmeans_restarts=restarts)`` reads at that timestep."""
    from .batched import kmeans_k

    s = _sim(B, N, 1, max(1, int(t) + 1), seed, 0.0, 0.0, 0.0, 0.0, 0.0)
    books = np.empty((max(int(B), 0), max(int(restarts), 0), kmeans_k(int(N)) if int(N) >= 1 else 0), dtype=np.int32)
    _lib.check(_lib.lib().pcx_sim_kmeans_books_host(C.byref(s), int(restarts), int(t), books.ctypes.data))
    return books


def kmeans_books(B, N, t=0, seed=0, restarts=_abi.KMEANS_RESTARTS, device=None):
    """:func:`kmeans_books_host` on the device (``pcx_sim_kmeans_books_f64``): an int32 tensor
    ``(B, restarts, k)``.  Asynchronous on torch's current stream."""
    from .batched import kmeans_k

    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    s = _sim(B, N, 1, max(1, int(t) + 1), seed, 0.0, 0.0, 0.0, 0.0, 0.0)
    books = tc.empty((max(int(B), 0), max(int(restarts), 0), kmeans_k(int(N)) if int(N) >= 1 else 0), dtype=tc.int32,
                     device=dev)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_kmeans_books_f64(h, C.byref(s), int(restarts), int(t), books.data_ptr()))
    return books


# ---------------------------------------------------------------- sweeps
CELL_FIELDS = ("rounds", "reporters", "events", "seed", "liar_frac", "collude_frac", "distort", "na_frac",
               "scaled_frac")
_CELL_DEFAULTS = {"reporters": 50, "events": 20, "seed": 0, "liar_frac": 0.3, "collude_frac": 0.5, "distort": 0.1,
                  "na_frac": 0.1, "scaled_frac": 0.25}  # simulate()'s
_OFFSETS = ("rounds", "reporters", "events", "cells")


def _cells(cells):
    """The cells as a list of full dicts, the pcx_sim_cell array and the per-cell starts."""
    norm = []
    for c, cell in enumerate(cells):
        if not isinstance(cell, dict):
            cell = tuple(cell)
            if not 1 <= len(cell) <= len(CELL_FIELDS):
                raise ValueError("cell %d: a tuple cell is (%s), from the left" % (c, ", ".join(CELL_FIELDS)))
            cell = dict(zip(CELL_FIELDS, cell))
        unknown = set(cell) - set(CELL_FIELDS) - set(_abi.PARAM_KEYS)  # (a dict cell may carry its own parameters)
        if unknown:
            raise ValueError("cell %d: unknown field(s) %s" % (c, sorted(unknown)))
        if "rounds" not in cell:
            raise ValueError("cell %d: needs 'rounds'" % c)
        norm.append(dict(_CELL_DEFAULTS, **cell))
    arr = (_abi.SimCell * max(len(norm), 1))()
    for k, d in zip(arr, norm):
        k.n_rounds, k.n_reporters, k.n_events = int(d["rounds"]), int(d["reporters"]), int(d["events"])
        k.seed = int(d["seed"]) & 0xFFFFFFFFFFFFFFFF
        for f in ("liar_frac", "collude_frac", "distort", "na_frac", "scaled_frac"):
            setattr(k, f, float(d[f]))
    R = np.array([int(d["rounds"]) for d in norm], dtype=np.int64)
    N = np.array([int(d["reporters"]) for d in norm], dtype=np.int64)
    E = np.array([int(d["events"]) for d in norm], dtype=np.int64)
    zero = np.zeros(1, dtype=np.int64)
    offsets = {"rounds": np.concatenate([zero, np.cumsum(R)]), "reporters": np.concatenate([zero, np.cumsum(R * N)]),
               "events": np.concatenate([zero, np.cumsum(R * E)]), "cells": np.concatenate([zero, np.cumsum(R * N * E)])}
    return norm, arr, offsets


def _sweep(cells, T=1, scaled_tol=0.1, algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5,
           variance_threshold=0.9, hierarchy_threshold=0.5, cluster_threshold=None, reputation0=None):
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    norm, arr, offsets = _cells(cells)
    # (max_components is capped at E_c on the device; cluster_threshold None = the device's per-round rule)
    s = _abi.SimSweep(len(norm), C.addressof(arr), int(T), float(scaled_tol), float(catch_tolerance), float(alpha),
                      alg, int(max_components), float(variance_threshold), float(hierarchy_threshold),
                      0.0 if cluster_threshold is None else float(cluster_threshold), reputation0)
    return s, arr, norm, offsets


def _cell_params(norm, algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
                 hierarchy_threshold=0.5, cluster_threshold=None, **_):
    """The pcx_round_params array [C] of cells that carry parameters of their own (a missing key takes
    the call's keyword value), or None when no cell does: then the existing entries run, unchanged."""
    if not any(k in d for d in norm for k in _abi.PARAM_KEYS):
        return None
    shared = dict(algorithm=algorithm, catch_tolerance=catch_tolerance, alpha=alpha, max_components=max_components,
                  variance_threshold=variance_threshold, hierarchy_threshold=hierarchy_threshold,
                  cluster_threshold=cluster_threshold)
    sets = [dict(shared, **{k: d[k] for k in _abi.PARAM_KEYS if k in d}) for d in norm]
    return (_abi.RoundParams * len(sets))(*[_abi.round_params(q) for q in sets])


def sweep_plan(cells, T=1, algorithm="PCA", tall=False, **params):
    """Validate a sweep without a device (``pcx_sim_sweep_plan``): ``(totals, counts, lds_bytes)`` as int64
    arrays of four: totals = (B, sum R N, sum R E, sum R N E); counts / lds_bytes are
    ``ragged_plan(wide=True)``'s for the sweep's rounds.  Raises with the cell's index on refusal.
    With cells that carry parameters of their own (``pcx_sim_study_params_check``) counts / lds_bytes
    are summed / the maximum over the cells, each by its own algorithm.

    ``tall=True`` (``pcx_sim_sweep_plan_tall``): cells up to 1024 x 64, refused by index for what
    ``batched.ragged_plan_tall`` refuses of their rounds.  The cells above 256 reporters count in
    totals and in no launch class: they are one more launch segment (``batched.tall_plan`` has a
    round's LDS plan)."""
    s, arr, norm, _ = _sweep(cells, T, algorithm=algorithm, **params)
    out = [(C.c_int64 * 4)() for _ in range(3)]
    bad = C.c_int64(-2)
    cp = _cell_params(norm, algorithm=algorithm, **params)
    if tall:
        _lib.check(_lib.lib().pcx_sim_sweep_plan_tall(C.byref(s), None if cp is None else C.cast(cp, C.c_void_p),
                                                      out[0], out[1], out[2], C.byref(bad)))
        return tuple(np.array(list(x), dtype=np.int64) for x in out)
    if cp is None:
        _lib.check(_lib.lib().pcx_sim_sweep_plan(C.byref(s), out[0], out[1], out[2], C.byref(bad)))
        return tuple(np.array(list(x), dtype=np.int64) for x in out)
    _lib.check(_lib.lib().pcx_sim_study_params_check(C.byref(s), C.cast(cp, C.c_void_p), None, C.byref(bad)))
    totals, counts, lds = (np.zeros(4, dtype=np.int64) for _ in range(3))
    names = {v: k for k, v in _abi.ALGORITHMS.items()}
    for alg in sorted({q.algorithm for q in cp}):  # the cells of one algorithm, as a sweep that shares it
        part = [{k: v for k, v in d.items() if k not in _abi.PARAM_KEYS} for d, q in zip(norm, cp) if q.algorithm == alg]
        t, c, l = sweep_plan(part, T, algorithm=names[alg])
        totals, counts, lds = totals + t, counts + c, np.maximum(lds, l)
    return totals, counts, lds


def _flat_len(kind, offsets):
    return int({"N": offsets["reporters"], "E": offsets["events"], "NE": offsets["cells"]}[kind][-1])


def sweep_generate_host(cells, t=0):
    """The rounds of timestep ``t`` of every cell drawn on the CPU (``pcx_sim_sweep_generate_host``):
    flat numpy arrays named as :func:`generate_host`'s, the cells' rounds end to end, and ``offsets``,
    a dict of int64 [C + 1] starts per cell: ``rounds``, ``reporters`` (``liar``), ``events``
    (``scaled``, ``lo``, ``hi``, ``truth``) and ``cells`` (``reports``)."""
    s, arr, _, offsets = _sweep(cells, max(1, int(t) + 1))
    rounds, c = {}, _abi.SimRounds()
    for name, kind, dt in _abi.SIM_ROUNDS:
        a = np.empty(_flat_len(kind, offsets), dtype=_NP[dt])
        rounds[name] = a
        setattr(c, name, a.ctypes.data)
    _lib.check(_lib.lib().pcx_sim_sweep_generate_host(C.byref(s), int(t), C.byref(c)))
    rounds["offsets"] = offsets
    return rounds


def _device_flat_rounds(t, dev, offsets, fields=None):
    rounds, c = {}, _abi.SimRounds()
    for name, kind, dt in _abi.SIM_ROUNDS:
        if fields is not None and name not in fields:
            continue
        x = t.empty(_flat_len(kind, offsets), dtype=_torch_dtype(t, dt), device=dev)
        rounds[name] = x
        setattr(c, name, x.data_ptr())
    return rounds, c


def sweep_generate(cells, t=0, fields=None, device=None):
    """:func:`sweep_generate_host` on the device: flat torch tensors (``fields``: only these arrays,
    the others are not written).  Asynchronous on torch's current stream."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    s, arr, _, offsets = _sweep(cells, max(1, int(t) + 1))
    rounds, c = _device_flat_rounds(tc, dev, offsets, fields)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_sweep_generate_f64(h, C.byref(s), int(t), C.byref(c)))
    rounds["offsets"] = offsets
    return rounds


def _sweep_books_offsets(norm, restarts):
    """int64 [B + 1]: where each round's ``restarts x k`` book rows start in a sweep's flat book array
    (``pcx_kmeans_plan`` over the sweep's rounds, the rule's k)."""
    from .batched import kmeans_plan

    shapes = [(int(d["reporters"]), int(d["events"])) for d in norm for _ in range(int(d["rounds"]))]
    return kmeans_plan(shapes, restarts)


def sweep_kmeans_books_host(cells, t=0, restarts=_abi.KMEANS_RESTARTS):
    """The k-means code books of timestep ``t`` of every round of a sweep, on the CPU
    (``pcx_sim_sweep_kmeans_books_host``; no GPU needed): ``(books, offsets)`` -- a flat int32 array,
    round b's ``(restarts, ceil(sqrt(N_c)))`` rows at ``offsets[b]`` (int64 [B + 1]), drawn under its
    cell's seed with the round's index inside the cell: cell c's slice is that cell's own
    :func:`kmeans_books_host`."""
    s, arr, norm, _ = _sweep(cells, max(1, int(t) + 1))
    _lib.check(_lib.lib().pcx_sim_study_kmeans_check(C.byref(s), None, None, int(restarts), C.byref(C.c_int64(-2))))
    offsets = _sweep_books_offsets(norm, restarts)
    books = np.empty(int(offsets[-1]), dtype=np.int32)
    _lib.check(_lib.lib().pcx_sim_sweep_kmeans_books_host(C.byref(s), int(restarts), int(t), books.ctypes.data))
    return books, offsets


def sweep_kmeans_books(cells, t=0, restarts=_abi.KMEANS_RESTARTS, device=None):
    """:func:`sweep_kmeans_books_host` on the device (``pcx_sim_sweep_kmeans_books_f64``): a flat int32
    tensor and the numpy offsets.  Asynchronous on torch's current stream."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    s, arr, norm, _ = _sweep(cells, max(1, int(t) + 1))
    _lib.check(_lib.lib().pcx_sim_study_kmeans_check(C.byref(s), None, None, int(restarts), C.byref(C.c_int64(-2))))
    offsets = _sweep_books_offsets(norm, restarts)
    books = tc.empty(int(offsets[-1]), dtype=tc.int32, device=dev)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_sweep_kmeans_books_f64(h, C.byref(s), int(restarts), int(t), books.data_ptr()))
    return books, offsets


def sweep_metrics(cells, rounds, old_rep, smooth_rep, outcomes_final, scaled_tol=0.1, summary=True, device=None):
    """Score a sweep's flat rounds (``pcx_sim_sweep_metrics_f64``): ``metrics (B,6)`` and, unless
    ``summary`` is false, ``summary (C,6)``, every cell's means over its rounds."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    s, arr, norm, offsets = _sweep(cells, 1, scaled_tol=scaled_tol)
    c, keep = _abi.SimRounds(), []
    for name, kind, dt in _abi.SIM_ROUNDS:
        if name != "reports":
            x = _device.as_device(rounds[name], _torch_dtype(tc, dt), dev)
            if tuple(x.shape) != (_flat_len(kind, offsets),):
                raise ValueError("rounds[%r] must be flat, %d long" % (name, _flat_len(kind, offsets)))
            keep.append(x)
            setattr(c, name, x.data_ptr())
    old, smooth, outc = (_device.as_device(x, tc.float64, dev) for x in (old_rep, smooth_rep, outcomes_final))
    tn, te = _flat_len("N", offsets), _flat_len("E", offsets)
    if tuple(old.shape) != (tn,) or tuple(smooth.shape) != (tn,) or tuple(outc.shape) != (te,):
        raise ValueError("old_rep / smooth_rep must be flat [sum R N] and outcomes_final flat [sum R E]")
    B = int(offsets["rounds"][-1])
    m = tc.empty((B, _abi.SIM_NMETRICS), dtype=tc.float64, device=dev)
    sm = tc.empty((len(norm), _abi.SIM_NMETRICS), dtype=tc.float64, device=dev) if summary else None
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_sweep_metrics_f64(h, C.byref(s), C.byref(c), old.data_ptr(), smooth.data_ptr(),
                                                    outc.data_ptr(), m.data_ptr(), _device.ptr(sm)))
    return {"metrics": m, "summary": sm, "offsets": offsets, "_inputs": (keep, old, smooth, outc)}


def sweep(cells, T=1, scaled_tol=0.1, algorithm="PCA", catch_tolerance=0.1, alpha=0.1, max_components=5,
          variance_threshold=0.9, hierarchy_threshold=0.5, cluster_threshold=None, reputation=None,
          keep_rounds=False, keep_outputs=False, device=None, kmeans_restarts=None, tall=False):
    """T timesteps of a whole study in one call: C cells, each with its own rounds, shape, rates and seed.

    ``cells`` is a list of dicts (or tuples, from the left) with ``rounds``, ``reporters``, ``events``,
    ``seed``, ``liar_frac``, ``collude_frac``, ``distort``, ``na_frac``, ``scaled_frac``; what a dict
    leaves out is :func:`simulate`'s default.  Shapes go up to 256 x 64.  The timesteps and ``scaled_tol``
    are shared.  A dict cell may also carry consensus parameters of its own (``algorithm``,
    ``catch_tolerance``, ``alpha``, ``max_components``, ``variance_threshold``, ``hierarchy_threshold``,
    ``cluster_threshold``; a missing key takes the call's keyword value): the call then goes through
    ``pcx_simulate_study_params_f64``, still one wide ragged batch per timestep with no more launches
    for more parameter sets.  The rounds of all cells lie end to end in cell order
    in :func:`consensus_ragged`'s flat layout and run as one wide ragged batch per timestep.

    Cell c's slice of every output is byte for byte ``simulate(R_c, N_c, E_c, T, seed_c, ...)``: the
    generator counts a round inside its cell and takes the cell's seed as its key.  So cells that
    share a seed see COMMON RANDOM NUMBERS (the same reporters lie, the same events are scaled,
    wherever the rates allow it): the usual variance reduction for a parameter curve.  Cells with
    different seeds are independent.  ("big-five" caps ``max_components`` at E_c per cell;
    "clusterfeck" without a ``cluster_threshold`` takes the device's log10(E_c)/1.77 per cell.)

    Returns device tensors ``metrics (T,B,6)`` with B = sum R_c, ``summary (T,C,6)`` (each cell's
    means in :func:`simulate`'s order), the flat ``reputation`` [sum R_c N_c], and ``offsets``, numpy
    int64 [C + 1] starts per cell (``rounds``, ``reporters``, ``events``, ``cells``) to slice with.
    ``reputation`` in: a flat starting reputation or None (uniform).  ``keep_rounds`` /
    ``keep_outputs`` add the last timestep's flat ``rounds`` / consensus ``outputs``.

    ``kmeans_restarts`` (an int >= 1; None = k-means refused, as before) lets "k-means" in, shared or as
    a cell's own ``algorithm`` (``pcx_simulate_study_kmeans_f64``): the books of the
    k-means cells' rounds are drawn on the device every timestep, under the cell's seed, and a k-means
    cell is byte for byte its own ``simulate(..., algorithm="k-means", kmeans_restarts=...)``.

    ``tall=True`` (``pcx_simulate_study_tall_f64``): shapes go up to 1024 x 64, so a
    ``grid(reporters=[128, 256, 512, 1024], ...)`` is one call.  A cell above 256 reporters must be of
    the tall route under its algorithm (``batched.route(N, E, algorithm, tall=True) == "tall"``,
    ``batched.tall_plan``: no clustering; big-five / fixed-variance where the plan fits) or the call
    is refused by cell; its rounds run one workgroup each in one more launch per timestep, and its
    slice is byte for byte ``simulate(R_c, N_c, E_c, T, seed_c, ..., tall=True)``.  Without such a
    cell the call is the one without ``tall``.  Not with ``kmeans_restarts``.

    Asynchronous on torch's current stream, with no host wait between the timesteps.  A sweep runs
    the generic ragged kernels: a study of ONE shape belongs on :func:`simulate`, whose compiled
    equal-shape kernel is faster."""
    return _run_sweep(cells, T, scaled_tol, algorithm, catch_tolerance, alpha, max_components, variance_threshold,
                      hierarchy_threshold, cluster_threshold, reputation, keep_rounds, keep_outputs, device,
                      kmeans_restarts=kmeans_restarts, tall=tall)


def _run_sweep(cells, T, scaled_tol, algorithm, catch_tolerance, alpha, max_components, variance_threshold,
               hierarchy_threshold, cluster_threshold, reputation, keep_rounds, keep_outputs, device,
               with_study=False, pair_with=None, keep_detail=False, kmeans_restarts=None, tall=False):
    """:func:`sweep` (``pcx_simulate_sweep_f64``) or, ``with_study``, :func:`study` (``pcx_simulate_study_f64``)."""
    if tall and kmeans_restarts is not None:
        raise ValueError("tall=True does not take kmeans_restarts (k-means stays within 256 reporters)")
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    rep = _device.as_device(reputation, tc.float64, dev)
    s, arr, norm, offsets = _sweep(cells, T, scaled_tol, algorithm, catch_tolerance, alpha, max_components,
                                   variance_threshold, hierarchy_threshold, cluster_threshold, _device.ptr(rep))
    shared = dict(algorithm=algorithm, catch_tolerance=catch_tolerance, alpha=alpha, max_components=max_components,
                  variance_threshold=variance_threshold, hierarchy_threshold=hierarchy_threshold,
                  cluster_threshold=cluster_threshold)
    cp = _cell_params(norm, **shared)  # None: no cell has parameters of its own
    st = base = None
    km = kmeans_restarts is not None
    if km:  # one check of the cells, their sets (k-means allowed), the restarts and the pairing
        base = pair_base(norm, pair_with) if with_study else None
        _lib.check(_lib.lib().pcx_sim_study_kmeans_check(C.byref(s), None if cp is None else C.cast(cp, C.c_void_p),
                                                         None if base is None else base.ctypes.data,
                                                         int(kmeans_restarts), C.byref(C.c_int64(-2))))
    elif tall:  # one check of the cells up to 1024 reporters, their sets and the pairing
        base = pair_base(norm, pair_with) if with_study else None
        _lib.check(_lib.lib().pcx_sim_study_tall_check(C.byref(s), None if cp is None else C.cast(cp, C.c_void_p),
                                                       None if base is None else base.ctypes.data,
                                                       C.byref(C.c_int64(-2))))
    elif cp is None:
        sweep_plan(cells, T, scaled_tol=scaled_tol, **shared)  # refuses by cell
    else:  # one check of the cells, their parameter sets and the pairing
        base = pair_base(norm, pair_with) if with_study else None
        _lib.check(_lib.lib().pcx_sim_study_params_check(C.byref(s), C.cast(cp, C.c_void_p),
                                                         None if base is None else base.ctypes.data,
                                                         C.byref(C.c_int64(-2))))
    T, Cn, B, tn = int(T), len(norm), int(offsets["rounds"][-1]), _flat_len("N", offsets)
    if rep is not None and tuple(rep.shape) != (tn,):
        raise ValueError("reputation must be flat, sum R_c N_c = %d long" % tn)
    out = {"metrics": tc.empty((T, B, _abi.SIM_NMETRICS), dtype=tc.float64, device=dev),
           "summary": tc.empty((T, Cn, _abi.SIM_NMETRICS), dtype=tc.float64, device=dev),
           "reputation": tc.empty((tn,), dtype=tc.float64, device=dev), "offsets": offsets}
    res = _abi.SimResult()
    res.metrics, res.summary, res.reputation = (out[k].data_ptr() for k in ("metrics", "summary", "reputation"))
    if keep_rounds:
        out["rounds"], res.last = _device_flat_rounds(tc, dev, offsets)
    if keep_outputs:
        outs = {}
        totals = tuple(_flat_len(k, offsets) for k in ("N", "E", "NE"))
        for name, kind, dt in _abi.BATCH_OUTPUTS:
            if name in ("original", "filled"):
                continue
            outs[name] = tc.empty(_abi.ragged_out_len(kind, B, totals), dtype=_torch_dtype(tc, dt), device=dev)
            setattr(res.last_out, name, outs[name].data_ptr())
        out["outputs"] = outs
    if with_study:
        if cp is None and not km and not tall:
            base = study_check(norm, pair_with, T, algorithm=algorithm, scaled_tol=scaled_tol,
                               max_components=max_components)  # refuses by cell
        st = _abi.SimStudyResult()
        out["stats"] = tc.empty((T, Cn, _abi.SIM_NVALUES, _abi.SIM_NSTATS), dtype=tc.float64, device=dev)
        st.stats = out["stats"].data_ptr()
        if base is not None:
            out["paired"] = tc.empty((T, Cn, _abi.SIM_NVALUES, _abi.SIM_NPAIRED), dtype=tc.float64, device=dev)
            out["pair_base"] = base
            st.paired = out["paired"].data_ptr()
        if keep_detail:
            out["detail"] = tc.empty((T, B, _abi.SIM_NDETAIL), dtype=tc.float64, device=dev)
            st.detail = out["detail"].data_ptr()
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    if km:
        _lib.check(_lib.lib().pcx_simulate_study_kmeans_f64(
            h, C.byref(s), None if cp is None else C.cast(cp, C.c_void_p), None if base is None else base.ctypes.data,
            int(kmeans_restarts), C.byref(res), None if st is None else C.byref(st)))
    elif tall:
        _lib.check(_lib.lib().pcx_simulate_study_tall_f64(
            h, C.byref(s), None if cp is None else C.cast(cp, C.c_void_p), None if base is None else base.ctypes.data,
            C.byref(res), None if st is None else C.byref(st)))
    elif cp is not None:
        _lib.check(_lib.lib().pcx_simulate_study_params_f64(
            h, C.byref(s), C.cast(cp, C.c_void_p), None if base is None else base.ctypes.data, C.byref(res),
            None if st is None else C.byref(st)))
    elif with_study:
        _lib.check(_lib.lib().pcx_simulate_study_f64(h, C.byref(s), None if base is None else base.ctypes.data,
                                                     C.byref(res), C.byref(st)))
    else:
        _lib.check(_lib.lib().pcx_simulate_sweep_f64(h, C.byref(s), C.byref(res)))
    out["_inputs"] = (rep,)  # alive until the caller syncs
    return out


# ---------------------------------------------------------------- studies
def pair_base(cells, pair_with):
    """``pair_with`` as the library's ``pair_base``: an int32 array [C] (-1: no base) or None.
    ``"first"`` pairs each cell with the first cell of the list that has its shape, rounds and seed
    (that first cell itself gets -1); a sequence gives the base indices."""
    if pair_with is None:
        return None
    norm = _cells(cells)[0]
    if isinstance(pair_with, str):
        if pair_with != "first":
            raise ValueError("pair_with is a list of base cells or 'first', not %r" % (pair_with,))
        first, base = {}, []
        for c, d in enumerate(norm):
            key = (int(d["reporters"]), int(d["events"]), int(d["rounds"]), int(d["seed"]) & 0xFFFFFFFFFFFFFFFF)
            base.append(first.setdefault(key, c))
        return np.array([-1 if b == c else b for c, b in enumerate(base)], dtype=np.int32)
    base = np.array([int(b) for b in pair_with], dtype=np.int64)
    if base.shape != (len(norm),):
        raise ValueError("pair_with needs one base per cell (%d), got %d" % (len(norm), base.size))
    if base.size and (base.min() < -(1 << 31) or base.max() >= (1 << 31)):
        raise ValueError("pair_with: a base is no int32")
    return base.astype(np.int32)


def study_check(cells, pair_with=None, T=1, algorithm="PCA", tall=False, **params):
    """Validate a study without a device (``pcx_sim_study_check``): what :func:`sweep_plan` refuses, then
    a base outside the cell list, a cell that is its own base, a base with another number of rounds.
    Raises with the cell's index; returns the ``pair_base`` array (or None).  ``tall`` as in
    :func:`sweep_plan` (``pcx_sim_study_tall_check``)."""
    s, arr, norm, _ = _sweep(cells, T, algorithm=algorithm, **params)
    base = pair_base(cells, pair_with)
    bad = C.c_int64(-2)
    cp = _cell_params(norm, algorithm=algorithm, **params)
    if tall:
        _lib.check(_lib.lib().pcx_sim_study_tall_check(C.byref(s), None if cp is None else C.cast(cp, C.c_void_p),
                                                       None if base is None else base.ctypes.data, C.byref(bad)))
    elif cp is None:
        _lib.check(_lib.lib().pcx_sim_study_check(C.byref(s), None if base is None else base.ctypes.data, C.byref(bad)))
    else:  # cells with parameters of their own
        _lib.check(_lib.lib().pcx_sim_study_params_check(C.byref(s), C.cast(cp, C.c_void_p),
                                                         None if base is None else base.ctypes.data, C.byref(bad)))
    return base


def _host_rounds(rounds, offsets=None, shape=None):
    """The pcx_sim_rounds of numpy arrays (everything but ``reports``), checked against the flat
    lengths of ``offsets`` or the equal shape (B, N, E)."""
    c, keep = _abi.SimRounds(), []
    for name, kind, dt in _abi.SIM_ROUNDS:
        if name == "reports":
            continue
        a = np.ascontiguousarray(rounds[name], dtype=_NP[dt])
        want = (_flat_len(kind, offsets),) if offsets is not None else _abi.out_shape(kind, *shape)
        if tuple(a.shape) != tuple(want):
            raise ValueError("rounds[%r] must have shape %s" % (name, tuple(want)))
        keep.append(a)
        setattr(c, name, a.ctypes.data)
    return c, keep


def detail_host(rounds, old_rep, smooth_rep, outcomes_final, scaled_tol=0.1):
    """The twelve :data:`DETAIL` metrics of B equal-shape rounds on the CPU (``pcx_sim_detail_host``; no
    GPU needed): numpy in, ``(B, 12)`` out -- bit for bit what :func:`detail` gives on the device."""
    old, smooth, outc = (np.ascontiguousarray(x, dtype=np.float64) for x in (old_rep, smooth_rep, outcomes_final))
    if old.ndim != 2 or outc.ndim != 2 or smooth.shape != old.shape or outc.shape[0] != old.shape[0]:
        raise ValueError("old_rep / smooth_rep must be (B, N) and outcomes_final (B, E)")
    (B, N), E = old.shape, outc.shape[1]
    c, keep = _host_rounds(rounds, shape=(B, N, E))
    s = _sim(B, N, E, 1, 0, 0.0, 0.0, 0.0, 0.0, 0.0, scaled_tol=scaled_tol)
    d = np.empty((B, _abi.SIM_NDETAIL), dtype=np.float64)
    _lib.check(_lib.lib().pcx_sim_detail_host(C.byref(s), C.byref(c), old.ctypes.data, smooth.ctypes.data,
                                              outc.ctypes.data, d.ctypes.data))
    return d


def detail(rounds, old_rep, smooth_rep, outcomes_final, scaled_tol=0.1, device=None):
    """:func:`detail_host` on the device (``pcx_sim_detail_f64``): a ``(B, 12)`` tensor.  Asynchronous."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    c, keep = _abi.SimRounds(), []
    for name, _, dt in _abi.SIM_ROUNDS:
        if name != "reports":
            x = _device.as_device(rounds[name], _torch_dtype(tc, dt), dev)
            keep.append(x)
            setattr(c, name, x.data_ptr())
    B, N = keep[-1].shape
    E = keep[0].shape[1]
    old, smooth, outc = (_device.as_device(x, tc.float64, dev) for x in (old_rep, smooth_rep, outcomes_final))
    if tuple(old.shape) != (B, N) or tuple(smooth.shape) != (B, N) or tuple(outc.shape) != (B, E):
        raise ValueError("old_rep / smooth_rep must be (B, N) and outcomes_final (B, E)")
    for x in keep[:-1]:
        if tuple(x.shape) != (B, E):
            raise ValueError("the event arrays of rounds must be (B, E)")
    s = _sim(B, N, E, 1, 0, 0.0, 0.0, 0.0, 0.0, 0.0, scaled_tol=scaled_tol)
    d = tc.empty((B, _abi.SIM_NDETAIL), dtype=tc.float64, device=dev)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_detail_f64(h, C.byref(s), C.byref(c), old.data_ptr(), smooth.data_ptr(),
                                             outc.data_ptr(), d.data_ptr()))
    d._pcx_inputs = (keep, old, smooth, outc)  # alive until the caller syncs
    return d


def sweep_detail_host(cells, rounds, old_rep, smooth_rep, outcomes_final, scaled_tol=0.1):
    """The :data:`DETAIL` metrics of a sweep's flat rounds on the CPU (``pcx_sim_sweep_detail_host``; no
    GPU needed): numpy in, ``(B, 12)`` out in the flat round order of ``metrics``."""
    s, arr, norm, offsets = _sweep(cells, 1, scaled_tol=scaled_tol)
    sweep_plan(cells, 1, scaled_tol=scaled_tol)  # refuses by cell before any array is read
    c, keep = _host_rounds(rounds, offsets=offsets)
    old, smooth, outc = (np.ascontiguousarray(x, dtype=np.float64) for x in (old_rep, smooth_rep, outcomes_final))
    tn, te = _flat_len("N", offsets), _flat_len("E", offsets)
    if old.shape != (tn,) or smooth.shape != (tn,) or outc.shape != (te,):
        raise ValueError("old_rep / smooth_rep must be flat [sum R N] and outcomes_final flat [sum R E]")
    d = np.empty((int(offsets["rounds"][-1]), _abi.SIM_NDETAIL), dtype=np.float64)
    _lib.check(_lib.lib().pcx_sim_sweep_detail_host(C.byref(s), C.byref(c), old.ctypes.data, smooth.ctypes.data,
                                                    outc.ctypes.data, d.ctypes.data))
    return d


def sweep_detail(cells, rounds, old_rep, smooth_rep, outcomes_final, scaled_tol=0.1, device=None):
    """:func:`sweep_detail_host` on the device (``pcx_sim_sweep_detail_f64``): a ``(B, 12)`` tensor.
    Asynchronous on torch's current stream."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    s, arr, norm, offsets = _sweep(cells, 1, scaled_tol=scaled_tol)
    sweep_plan(cells, 1, scaled_tol=scaled_tol)
    c, keep = _abi.SimRounds(), []
    for name, kind, dt in _abi.SIM_ROUNDS:
        if name != "reports":
            x = _device.as_device(rounds[name], _torch_dtype(tc, dt), dev)
            if tuple(x.shape) != (_flat_len(kind, offsets),):
                raise ValueError("rounds[%r] must be flat, %d long" % (name, _flat_len(kind, offsets)))
            keep.append(x)
            setattr(c, name, x.data_ptr())
    old, smooth, outc = (_device.as_device(x, tc.float64, dev) for x in (old_rep, smooth_rep, outcomes_final))
    tn, te = _flat_len("N", offsets), _flat_len("E", offsets)
    if tuple(old.shape) != (tn,) or tuple(smooth.shape) != (tn,) or tuple(outc.shape) != (te,):
        raise ValueError("old_rep / smooth_rep must be flat [sum R N] and outcomes_final flat [sum R E]")
    d = tc.empty((int(offsets["rounds"][-1]), _abi.SIM_NDETAIL), dtype=tc.float64, device=dev)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_sweep_detail_f64(h, C.byref(s), C.byref(c), old.data_ptr(), smooth.data_ptr(),
                                                   outc.data_ptr(), d.data_ptr()))
    d._pcx_inputs = (keep, old, smooth, outc)  # alive until the caller syncs
    return d


def _stats_shapes(cells, metrics_shape, detail_shape):
    norm, _, offsets = _cells(cells)
    B = int(offsets["rounds"][-1])
    if len(metrics_shape) != 3 or tuple(metrics_shape[1:]) != (B, _abi.SIM_NMETRICS):
        raise ValueError("metrics must be (T, %d, %d)" % (B, _abi.SIM_NMETRICS))
    T = int(metrics_shape[0])
    if tuple(detail_shape) != (T, B, _abi.SIM_NDETAIL):
        raise ValueError("detail must be (%d, %d, %d)" % (T, B, _abi.SIM_NDETAIL))
    if T < 1:
        raise ValueError("metrics and detail need at least one timestep")
    return T, len(norm)


def sweep_stats_host(cells, metrics, detail, pair_with=None):
    """Per-cell statistics on the CPU (``pcx_sim_sweep_stats_host``; no GPU needed) of ``metrics (T,B,6)``
    and ``detail (T,B,12)``: a dict with ``stats (T,C,18,5)`` (:data:`VALUES` x :data:`STATS`) and, with
    ``pair_with`` (see :func:`study`), ``paired (T,C,18,3)`` and ``pair_base``.  The library's summation
    order replayed in a loop: bit for bit :func:`sweep_stats`."""
    m, d = (np.ascontiguousarray(x, dtype=np.float64) for x in (metrics, detail))
    T, Cn = _stats_shapes(cells, m.shape, d.shape)
    base = study_check(cells, pair_with, T)
    s, arr, _, _ = _sweep(cells, T)
    out = {"stats": np.empty((T, Cn, _abi.SIM_NVALUES, _abi.SIM_NSTATS), dtype=np.float64)}
    if base is not None:
        out["paired"] = np.empty((T, Cn, _abi.SIM_NVALUES, _abi.SIM_NPAIRED), dtype=np.float64)
        out["pair_base"] = base
    _lib.check(_lib.lib().pcx_sim_sweep_stats_host(
        C.byref(s), m.ctypes.data, d.ctypes.data, None if base is None else base.ctypes.data,
        out["stats"].ctypes.data, out["paired"].ctypes.data if base is not None else None))
    return out


def sweep_stats(cells, metrics, detail, pair_with=None, device=None):
    """:func:`sweep_stats_host` on the device (``pcx_sim_sweep_stats_f64``), device tensors in and out.
    One launch for all timesteps, asynchronous on torch's current stream."""
    tc = _device.require_gpu()
    dev = tc.device(device) if device is not None else tc.device("cuda", tc.cuda.current_device())
    m, d = (_device.as_device(x, tc.float64, dev) for x in (metrics, detail))
    T, Cn = _stats_shapes(cells, tuple(m.shape), tuple(d.shape))
    base = study_check(cells, pair_with, T)
    s, arr, _, _ = _sweep(cells, T)
    out = {"stats": tc.empty((T, Cn, _abi.SIM_NVALUES, _abi.SIM_NSTATS), dtype=tc.float64, device=dev)}
    if base is not None:
        out["paired"] = tc.empty((T, Cn, _abi.SIM_NVALUES, _abi.SIM_NPAIRED), dtype=tc.float64, device=dev)
        out["pair_base"] = base
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_sim_sweep_stats_f64(
        h, C.byref(s), m.data_ptr(), d.data_ptr(), None if base is None else base.ctypes.data,
        out["stats"].data_ptr(), out["paired"].data_ptr() if base is not None else None))
    out["_inputs"] = (m, d)  # alive until the caller syncs
    return out


def study(cells, T=1, pair_with=None, keep_detail=False, scaled_tol=0.1, algorithm="PCA", catch_tolerance=0.1,
          alpha=0.1, max_components=5, variance_threshold=0.9, hierarchy_threshold=0.5, cluster_threshold=None,
          reputation=None, keep_rounds=False, keep_outputs=False, device=None, kmeans_restarts=None, tall=False):
    """:func:`sweep` with a study's result (``pcx_simulate_study_f64``): every key of
    :func:`sweep`'s dict, byte for byte, plus

    * ``stats (T,C,18,5)``: per timestep, cell and value (:data:`VALUES`: the six :data:`METRICS`, then
      the twelve :data:`DETAIL` metrics) ``{n, mean, var, min, max}`` (:data:`STATS`) over the cell's
      rounds whose value is not NaN.  ``mean`` of a metric without NaNs is ``summary``'s bytes;
      :func:`stderr` turns ``var`` and ``n`` into a standard error;
    * with ``pair_with``, ``paired (T,C,18,3)``: ``{n, mean, var}`` of ``value_c[b] - value_base[b]``,
      round by round, and ``pair_base``, the int32 base per cell.  ``pair_with`` is a list of base cell
      indices (-1: none; a base has its cell's number of rounds) or ``"first"``: each cell is paired with
      the first cell of the list that has its shape, rounds and seed (that first cell gets -1).  Cells
      that share a seed see common random numbers, so the paired standard error along a parameter
      curve is far below the difference of two independent cells';
    * with ``keep_detail``, ``detail (T,B,12)``, the per-round :data:`DETAIL` metrics.

    The detail metrics are written on the device inside the loop (one more launch per timestep), the
    statistics by one launch after the last timestep; the call stays asynchronous on torch's current
    stream with no host wait.  Refusals are :func:`sweep`'s and :func:`study_check`'s.
    ``kmeans_restarts`` as in :func:`sweep`: with it a cell may be k-means, and ``pair_with="first"``
    pairs a PCA cell and a k-means cell of one seed and shape on the same drawn rounds.
    ``tall`` as in :func:`sweep`: cells up to 1024 reporters, scored, paired and summarised like the others."""
    return _run_sweep(cells, T, scaled_tol, algorithm, catch_tolerance, alpha, max_components, variance_threshold,
                      hierarchy_threshold, cluster_threshold, reputation, keep_rounds, keep_outputs, device,
                      with_study=True, pair_with=pair_with, keep_detail=keep_detail, kmeans_restarts=kmeans_restarts,
                      tall=tall)


def stderr(stats_or_paired):
    """Standard errors ``sqrt(var / n)`` of a ``stats`` or ``paired`` array (``[..., 0]`` is n and
    ``[..., 2]`` var in both), on the host: numpy, NaN where n < 2."""
    x = stats_or_paired
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(x[..., 2] / x[..., 0])


_GRID_AXES = ("reporters", "events", "liar_frac", "collude_frac", "distort", "na_frac", "scaled_frac") + _abi.PARAM_KEYS


def grid(rounds, seed=0, independent=False, **axes):
    """The cell list of a cartesian product: every axis (``reporters``, ``events``, ``liar_frac``,
    ``collude_frac``, ``distort``, ``na_frac``, ``scaled_frac``, and the consensus parameters
    ``algorithm``, ``catch_tolerance``, ``alpha``, ``max_components``, ``variance_threshold``,
    ``hierarchy_threshold``, ``cluster_threshold``) a value or a sequence of values, the
    first axis given varying slowest; ``rounds`` per cell.  All cells share ``seed`` (common random
    numbers along every axis) unless ``independent``: then cell k has ``seed + k``.  Along a parameter
    axis the cells draw the same rounds: ``study(pair_with="first")`` pairs them."""
    import itertools

    unknown = set(axes) - set(_GRID_AXES)
    if unknown:
        raise ValueError("grid: unknown axis %s (axes: %s)" % (sorted(unknown), ", ".join(_GRID_AXES)))
    names = list(axes)
    values = [list(v) if isinstance(v, (list, tuple, np.ndarray, range)) else [v] for v in axes.values()]
    cells = []
    for k, combo in enumerate(itertools.product(*values)):
        cell = {"rounds": int(rounds), "seed": int(seed) + (k if independent else 0)}
        cell.update(zip(names, (v.item() if isinstance(v, np.generic) else v for v in combo)))
        cells.append(cell)
    return cells


def _comma_list(kind):
    def parse(text):
        return [kind(x) for x in text.split(",")]
    return parse


def main(argv=None):
    import argparse
    import json

    ap = argparse.ArgumentParser(prog="python -m pyconsensus_amd.simulate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=1024, help="B, rounds per timestep")
    ap.add_argument("--reporters", type=_comma_list(int), default=[50], help="N; a comma list runs a grid")
    ap.add_argument("--events", type=_comma_list(int), default=[20], help="E; a comma list runs a grid")
    ap.add_argument("--timesteps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    flt = _comma_list(float)
    ap.add_argument("--liars", type=flt, default=[0.3], help="liar_frac (or a comma list)")
    ap.add_argument("--collude", type=flt, default=[0.5], help="collude_frac (or a comma list)")
    ap.add_argument("--distort", type=flt, default=[0.1], help="(or a comma list)")
    ap.add_argument("--missing", type=flt, default=[0.1], help="na_frac (or a comma list)")
    ap.add_argument("--scaled", type=flt, default=[0.25], help="scaled_frac (or a comma list)")
    ap.add_argument("--scaled-tol", type=float, default=0.1)
    ap.add_argument("--algorithm", type=_comma_list(str), default=["PCA"],
                    help="a comma list runs every cell under each algorithm, in one call")
    ap.add_argument("--kmeans-restarts", type=int, default=None,
                    help="restarts of every k-means round (default 20 where --algorithm names k-means)")
    ap.add_argument("--tall", action="store_true",
                    help="rounds and cells up to 1024 reporters (those above 256 on the tall workgroup kernel)")
    ap.add_argument("--alpha", type=flt, default=None, help="the reputation smoothing (or a comma list)")
    ap.add_argument("--catch", type=flt, default=None, help="catch_tolerance (or a comma list)")
    ap.add_argument("--stats", action="store_true",
                    help="run a study: every timestep gains 'detail' (the means of the detail metrics) and "
                         "'stderr' (the standard errors of all eighteen values)")
    ap.add_argument("--paired", action="store_true",
                    help="(implies --stats) pair each cell with the first of its shape: 'vs_first', "
                         "{name: [mean, stderr]} of the round-by-round differences")
    a = ap.parse_args(argv)
    lists = {"reporters": a.reporters, "events": a.events, "liar_frac": a.liars, "collude_frac": a.collude,
             "distort": a.distort, "na_frac": a.missing, "scaled_frac": a.scaled}
    # the consensus parameters: a single value is the call's keyword, a list an axis of the grid (its
    # cells carry the key, and their JSON objects show it)
    a.shared = {}
    for key, values in (("algorithm", a.algorithm), ("alpha", a.alpha), ("catch_tolerance", a.catch)):
        if values is not None and len(values) > 1:
            lists[key] = values
        elif values is not None:
            a.shared[key] = values[0]
    if a.kmeans_restarts is not None or "k-means" in a.algorithm:  # naming k-means enables it
        a.shared["kmeans_restarts"] = _abi.KMEANS_RESTARTS if a.kmeans_restarts is None else a.kmeans_restarts
    if a.tall:
        a.shared["tall"] = True
    a.algorithm = ",".join(a.algorithm)
    if a.stats or a.paired:
        return _main_study(a, lists)
    if any(len(v) > 1 for v in lists.values()):  # a grid: --rounds per cell, one shared seed
        cells = grid(a.rounds, seed=a.seed, **lists)
        r = sweep(cells, a.timesteps, scaled_tol=a.scaled_tol, **a.shared)
        summary = r["summary"].cpu().numpy()  # (the copy synchronises)
        print(json.dumps({"rounds": a.rounds, "seed": a.seed, "algorithm": a.algorithm,
                          "cells": [dict({k: v for k, v in cell.items() if k not in ("rounds", "seed")},
                                         summary=[dict(zip(METRICS, (float(v) for v in row)), timestep=t)
                                                  for t, row in enumerate(summary[:, c])])
                                    for c, cell in enumerate(cells)]}))
        return 0
    a.reporters, a.events, a.liars, a.collude, a.distort, a.missing, a.scaled = (v[0] for v in lists.values())
    r = simulate(a.rounds, a.reporters, a.events, a.timesteps, seed=a.seed, liar_frac=a.liars,
                 collude_frac=a.collude, distort=a.distort, na_frac=a.missing, scaled_frac=a.scaled,
                 scaled_tol=a.scaled_tol, **a.shared)
    summary = r["summary"].cpu().numpy()  # (the copy synchronises)
    print(json.dumps({"rounds": a.rounds, "reporters": a.reporters, "events": a.events, "seed": a.seed,
                      "algorithm": a.algorithm,
                      "summary": [dict(zip(METRICS, (float(v) for v in row)), timestep=t)
                                  for t, row in enumerate(summary)]}))
    return 0


def _main_study(a, lists):
    """--stats / --paired: the same objects as without the flags, every timestep's dict extended."""
    import json

    cells = grid(a.rounds, seed=a.seed, **lists)
    r = study(cells, a.timesteps, pair_with="first" if a.paired else None, scaled_tol=a.scaled_tol, **a.shared)
    summary, stats = r["summary"].cpu().numpy(), r["stats"].cpu().numpy()  # (the copies synchronise)
    se = stderr(stats)
    if a.paired:
        paired, pse, base = r["paired"].cpu().numpy(), stderr(r["paired"]), r["pair_base"]

    def timestep(c, t):
        d = dict(zip(METRICS, (float(v) for v in summary[t, c])), timestep=t)
        d["detail"] = dict(zip(DETAIL, (float(v) for v in stats[t, c, len(METRICS):, 1])))
        d["stderr"] = dict(zip(VALUES, (float(v) for v in se[t, c])))
        if a.paired and base[c] >= 0:
            d["vs_first"] = {k: [float(paired[t, c, v, 1]), float(pse[t, c, v])] for v, k in enumerate(VALUES)}
        return d

    if any(len(v) > 1 for v in lists.values()):
        print(json.dumps({"rounds": a.rounds, "seed": a.seed, "algorithm": a.algorithm,
                          "cells": [dict({k: v for k, v in cell.items() if k not in ("rounds", "seed")},
                                         summary=[timestep(c, t) for t in range(a.timesteps)])
                                    for c, cell in enumerate(cells)]}))
    else:  # one cell: the equal-shape call's object
        print(json.dumps({"rounds": a.rounds, "reporters": lists["reporters"][0], "events": lists["events"][0],
                          "seed": a.seed, "algorithm": a.algorithm,
                          "summary": [timestep(0, t) for t in range(a.timesteps)]}))
    return 0


if __name__ == "__main__":
    import sys

    sys.exit(main())
