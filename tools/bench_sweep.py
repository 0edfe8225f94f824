"""Cost of a simulator sweep (pyconsensus_amd.simulate.sweep) against the only route
without it: one simulate() call per cell in a loop on the same stream, synchronised once at the end.

One JSON line per measurement.  Device time from HIP events around the whole call(s), after a warm-up
of both sides; the two sides alternate run by run in one invocation; medians with min - max.

* ``grid``: a grid a study would run: 20 values of liar_frac x N in {20, 50, 100, 200} x E in {10, 20, 40},
  240 cells of 256 rounds, T = 8, PCA.
* ``single``: one cell of 65,536 x 50 x 20, T = 8.  Here the sweep is expected to LOSE: it runs the generic
  one-wave kernel where simulate() runs the instance compiled for 50 x 20.
* ``generate``: the sweep generator alone on the grid (the call's device time, table upload included) and
  the bytes it writes; the kernels' own times come from a kernel trace of ``--only grid`` in a run of its own.

usage: python tools/bench_sweep.py [--only grid|single|generate] [--reps 9] [--timesteps 8] [--rounds 256]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("grid", "single", "generate"), default=None)
    ap.add_argument("--reps", type=int, default=9, help="timed runs per side (at least 7 for a figure to keep)")
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=256, help="rounds per cell of the grid")
    ap.add_argument("--single-rounds", type=int, default=65536)
    a = ap.parse_args()
    T = a.timesteps

    import numpy as np
    import torch

    import pyconsensus_amd.simulate  # noqa: F401
    S = sys.modules["pyconsensus_amd.simulate"]
    assert torch.cuda.is_available(), "bench_sweep needs the GPU"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def per_cell(cells):
        out = []
        for c in cells:
            out.append(S.simulate(c["rounds"], c["reporters"], c["events"], T, seed=c["seed"],
                                  **{k: v for k, v in c.items() if k.endswith("_frac") or k == "distort"}))
        return out

    def compare(name, cells, extra):
        norm = S._cells(cells)[0]
        sides = {"sweep": lambda: S.sweep(norm, T), "simulate_per_cell": lambda: per_cell(norm)}
        for fn in sides.values():  # warm both sides up: code objects, work buffers, torch's allocator
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(a.reps):  # alternate the sides
            for k, fn in sides.items():
                ms[k].append(timed(fn)[0])
        # the two sides computed the same thing
        sw, ref = S.sweep(norm, T), per_cell(norm)
        torch.cuda.synchronize()
        same = all(np.array_equal(sw["summary"][:, c].cpu().numpy(), r["summary"].cpu().numpy(), equal_nan=True)
                   for c, r in enumerate(ref))
        med = {k: statistics.median(v) for k, v in ms.items()}
        rounds = sum(c["rounds"] for c in norm)
        print(json.dumps(dict(extra, measurement=name, cells=len(norm), rounds=rounds, timesteps=T, reps=a.reps,
                              median_ms=med, min_max_ms={k: [min(v), max(v)] for k, v in ms.items()},
                              sweep_over_per_cell=med["sweep"] / med["simulate_per_cell"],
                              per_cell_over_sweep=med["simulate_per_cell"] / med["sweep"],
                              sweep_rounds_per_s=rounds * T / (med["sweep"] * 1e-3), same_summaries=same)), flush=True)

    grid = S.grid(a.rounds, seed=1, liar_frac=[round(0.025 * (k + 1), 3) for k in range(20)],
                  reporters=[20, 50, 100, 200], events=[10, 20, 40])
    if a.only in (None, "grid"):
        compare("grid", grid, {"grid": "20 liar_frac x N {20,50,100,200} x E {10,20,40}", "rounds_per_cell": a.rounds})
    if a.only in (None, "single"):
        compare("single", [dict(rounds=a.single_rounds, reporters=50, events=20, seed=1)], {"shape": "50 x 20"})
    if a.only in (None, "generate"):
        off = S._cells(grid)[2]
        nbytes = int(off["cells"][-1] * 8 + 3 * off["events"][-1] * 8 + off["events"][-1] + off["reporters"][-1])
        for _ in range(3):
            S.sweep_generate(grid, 0)
        torch.cuda.synchronize()
        ms = [timed(lambda: S.sweep_generate(grid, t % T))[0] for t in range(max(a.reps, 7))]
        med = statistics.median(ms)
        print(json.dumps({"measurement": "generate", "cells": len(grid), "rounds": int(off["rounds"][-1]),
                          "bytes_written": nbytes, "call_median_ms": med, "call_min_max_ms": [min(ms), max(ms)],
                          "call_GB_per_s": nbytes / (med * 1e-3) / 1e9}), flush=True)


if __name__ == "__main__":
    main()
