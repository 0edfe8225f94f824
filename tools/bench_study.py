"""Cost of a simulator study (pyconsensus_amd.simulate.study) over the sweep it extends:
the 240-cell grid of tools/bench_sweep.py at T = 8, ``study(grid, T, pair_with="first")`` and
``sweep(grid, T)`` alternately on one box.

One JSON line.  Device time from HIP events around the whole call, after a warm-up of both sides; the
sides alternate run by run; medians with min - max.  ``study - sweep`` is to be set against what the study
adds per call: T launches of k_sim_study_detail (one lane per round, as k_sim_sweep_metrics) and one of
k_sim_study_stats, whose times come from a kernel trace of this script in a run of its own.

``--sweep-only`` times sweep() alone (the yardstick for the loop the two calls share: run it with PCX_LIB
on the parent's library and on this one alternately).

usage: python tools/bench_study.py [--reps 9] [--timesteps 8] [--rounds 256] [--sweep-only]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9, help="timed runs per side (at least 7 for a figure to keep)")
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=256, help="rounds per cell of the grid")
    ap.add_argument("--sweep-only", action="store_true", help="time sweep() alone (works with a library without studies)")
    a = ap.parse_args()
    T = a.timesteps

    import numpy as np
    import torch

    import pyconsensus_amd.simulate  # noqa: F401
    S = sys.modules["pyconsensus_amd.simulate"]
    assert torch.cuda.is_available(), "bench_study needs the GPU"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    grid = S._cells(S.grid(a.rounds, seed=1, liar_frac=[round(0.025 * (k + 1), 3) for k in range(20)],
                           reporters=[20, 50, 100, 200], events=[10, 20, 40]))[0]
    sides = {"sweep": lambda: S.sweep(grid, T)}
    if not a.sweep_only:
        sides["study"] = lambda: S.study(grid, T, pair_with="first")
    for fn in sides.values():  # warm both sides up: code objects, work buffers, torch's allocator
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(a.reps):  # alternate the sides
        for k, fn in sides.items():
            ms[k].append(timed(fn)[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    rounds = sum(c["rounds"] for c in grid)
    line = dict(measurement="sweep_only" if a.sweep_only else "study", lib=os.environ.get("PCX_LIB", "in-tree"),
                grid="20 liar_frac x N {20,50,100,200} x E {10,20,40}", cells=len(grid), rounds=rounds,
                rounds_per_cell=a.rounds, timesteps=T, reps=a.reps, median_ms=med,
                min_max_ms={k: [min(v), max(v)] for k, v in ms.items()})
    if not a.sweep_only:
        st, sw = S.study(grid, T, pair_with="first"), S.sweep(grid, T)
        torch.cuda.synchronize()
        line.update(study_minus_sweep_ms=med["study"] - med["sweep"], study_over_sweep=med["study"] / med["sweep"],
                    paired_cells=int((st["pair_base"] >= 0).sum()),
                    same_summaries=bool(np.array_equal(st["summary"].cpu().numpy(), sw["summary"].cpu().numpy(),
                                                       equal_nan=True)))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
