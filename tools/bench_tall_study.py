"""What tall cells in one study buy, and what the per-round descriptor costs on tall rounds (DESIGN.md
5.4.5 / 5.5.3).  One JSON line per measurement; medians of --reps timed runs after a warm-up, with min - max.

``--measure study``: a reporter-axis study, grid(reporters=[128, 256, 512, 1024], events=32, liar_frac=[0.1,
0.3]), 256 rounds a cell, T = 8, PCA.  ``one_call``: study(cells, T, tall=True).  ``split``: the only way
without the tall entries -- the cells up to 256 reporters in one study() and one simulate() per larger cell
(the round scheduler, a blocking call).  Host clock from before the first call to after a final
synchronise.  With PCX_LIB on a library from before the tall entries only ``split`` runs: the parent's
own code as the yardstick.

``--measure descriptor``: pcx_consensus_ragged_tall_f64 against pcx_consensus_batched_tall_f64 on the same
--rounds rounds of 512 x 64 (PCA, inputs resident on the device, seven outputs), called through ctypes so
that no host packing is timed; the sides alternate run by run; HIP-event time around each call.

usage: python tools/bench_tall_study.py --measure study|descriptor [--reps 7] [--rounds N]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stat(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", choices=("study", "descriptor"), required=True)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=None, help="study: rounds a cell (256); descriptor: rounds (4096)")
    a = ap.parse_args()

    import numpy as np
    import torch

    import pyconsensus_amd.simulate  # noqa: F401
    from pyconsensus_amd import _abi, _device, _lib
    S = sys.modules["pyconsensus_amd.simulate"]
    assert torch.cuda.is_available(), "bench_tall_study needs the GPU"
    have_tall = hasattr(_lib.lib(), "pcx_simulate_study_tall_f64")

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if a.measure == "study":
        R, T = a.rounds or 256, 8
        cells = S.grid(R, seed=7, reporters=[128, 256, 512, 1024], events=32, liar_frac=[0.1, 0.3])
        small = [c for c in cells if c["reporters"] <= 256]
        big = [c for c in cells if c["reporters"] > 256]

        def split():
            keep = [S.study(small, T)]
            for c in big:
                keep.append(S.simulate(c["rounds"], c["reporters"], c["events"], T, seed=c["seed"],
                                       liar_frac=c["liar_frac"]))
            return keep

        sides = {"split": split}
        if have_tall:
            sides["one_call"] = lambda: S.study(cells, T, tall=True)
        for fn in sides.values():
            fn()
        times = {k: [] for k in sides}
        for _ in range(a.reps):
            for k, fn in sides.items():
                times[k].append(host_ms(fn))
        print(json.dumps({"measure": "study", "rounds_per_cell": R, "timesteps": T, "cells": len(cells),
                          "library": os.environ.get("PCX_LIB", "this tree"),
                          **{k: stat(v) for k, v in times.items()}}))
        return 0

    B, N, E = a.rounds or 4096, 512, 64
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(5)
    Rm = torch.randint(1, 3, (B, N, E), generator=g, device=dev).to(torch.float64)
    Rm[torch.rand((B, N, E), generator=g, device=dev) < 0.1] = float("nan")
    rep = torch.randint(1, 100, (B, N), generator=g, device=dev).to(torch.float64)
    names = ("smooth_rep", "this_rep", "outcomes_final", "certainty", "reporter_bonus", "author_bonus", "branch")
    kinds = {n: (k, dt) for n, k, dt in _abi.BATCH_OUTPUTS}
    outs, res = {}, _abi.BatchResult()
    for n in names:
        k, dt = kinds[n]
        outs[n] = torch.empty(_abi.out_shape(k, B, N, E), dtype=torch.float64 if dt == "f8" else torch.int32, device=dev)
        setattr(res, n, outs[n].data_ptr())
    batch = _abi.Batch(B, N, E, Rm.data_ptr(), rep.data_ptr(), None, None, None, 0, 0, 0.1, 0.1, 0, 5, 0.9, None, 0.5,
                       0.0, 0, 0, None)
    ns, es = np.full(B, N, dtype=np.int32), np.full(B, E, dtype=np.int32)
    rag = _abi.Ragged(B, ns.ctypes.data, es.ctypes.data, Rm.data_ptr(), rep.data_ptr(), None, None, None, 0, 0, 0.1, 0.1,
                      5, 0.9, None, 0.5, 0.0)
    sets = (_abi.RoundParams * 1)(_abi.round_params(dict(algorithm="PCA", catch_tolerance=0.1, alpha=0.1,
                                                         max_components=5, variance_threshold=0.9,
                                                         hierarchy_threshold=0.5, cluster_threshold=None)))
    of = np.zeros(B, dtype=np.int32)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    L = _lib.lib()
    sides = {
        "batched_tall": lambda: _lib.check(L.pcx_consensus_batched_tall_f64(h, C.byref(batch), C.byref(res))),
        "ragged_tall": lambda: _lib.check(L.pcx_consensus_ragged_tall_f64(h, C.byref(rag), 1, C.cast(sets, C.c_void_p),
                                                                          of.ctypes.data, C.byref(res))),
    }

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ref = {}
    for k, fn in sides.items():  # warm-up, and the two sides give the same bytes
        fn()
        torch.cuda.synchronize()
        ref[k] = {n: outs[n].clone() for n in names}
    same = all(torch.equal(ref["batched_tall"][n].view(torch.int64 if ref["batched_tall"][n].dtype == torch.float64
                                                       else torch.int32),
                           ref["ragged_tall"][n].view(torch.int64 if ref["ragged_tall"][n].dtype == torch.float64
                                                      else torch.int32)) for n in names)
    times = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, fn in sides.items():
            times[k].append(event_ms(fn))
    out = {k: stat(v) for k, v in times.items()}
    print(json.dumps({"measure": "descriptor", "rounds": B, "shape": [N, E], "same_bytes": bool(same), **out,
                      "ragged_over_batched": out["ragged_tall"]["median_ms"] / out["batched_tall"]["median_ms"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
