"""On-device Monte Carlo simulator: draw random rounds, run consensus on them, score them.

The Simulator.jl-style driver of the batched regime (README.rst:52-56) without the host in
the loop.  Per timestep libpcx generates B rounds of N x E reports on the device (a
counter-based Philox4x32-10 generator, csrc/pcx_sim.h; DESIGN.md "Simulator" is its
specification), runs :func:`pyconsensus_amd.consensus_batched`'s kernel on them, reduces each
round to :data:`METRICS` against the truth it drew, and carries ``smooth_rep`` into the next
timestep's reputation.

    python -m pyconsensus_amd.simulate --rounds 65536 --timesteps 8 --seed 1

prints the per-timestep means of the metrics as JSON.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _device, _lib
from .batched import clusterfeck_threshold

METRICS = ("correct", "liar_rep_before", "liar_rep_after", "liars_bonus", "beats", "n_liars")
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
             cluster_threshold=None, keep_rounds=False, keep_outputs=False, device=None):
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
    (one workgroup per round above 64 x 32) -- synchronise before reading on the host; "k-means"
    and "cokurtosis" are refused (they need host draws / caller scores)."""
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
    _lib.check(_lib.lib().pcx_simulate_f64(h, C.byref(s), C.byref(res)))
    out["_inputs"] = (rep,)  # alive until the caller syncs
    return out


def main(argv=None):
    import argparse
    import json

    ap = argparse.ArgumentParser(prog="python -m pyconsensus_amd.simulate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=1024, help="B, rounds per timestep")
    ap.add_argument("--reporters", type=int, default=50)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--timesteps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--liars", type=float, default=0.3, help="liar_frac")
    ap.add_argument("--collude", type=float, default=0.5, help="collude_frac")
    ap.add_argument("--distort", type=float, default=0.1)
    ap.add_argument("--missing", type=float, default=0.1, help="na_frac")
    ap.add_argument("--scaled", type=float, default=0.25, help="scaled_frac")
    ap.add_argument("--scaled-tol", type=float, default=0.1)
    ap.add_argument("--algorithm", default="PCA")
    a = ap.parse_args(argv)
    r = simulate(a.rounds, a.reporters, a.events, a.timesteps, seed=a.seed, liar_frac=a.liars,
                 collude_frac=a.collude, distort=a.distort, na_frac=a.missing, scaled_frac=a.scaled,
                 scaled_tol=a.scaled_tol, algorithm=a.algorithm)
    summary = r["summary"].cpu().numpy()  # (the copy synchronises)
    print(json.dumps({"rounds": a.rounds, "reporters": a.reporters, "events": a.events, "seed": a.seed,
                      "algorithm": a.algorithm,
                      "summary": [dict(zip(METRICS, (float(v) for v in row)), timestep=t)
                                  for t, row in enumerate(summary)]}))
    return 0


if __name__ == "__main__":
    import sys

    sys.exit(main())
