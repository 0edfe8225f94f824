"""What per-cell consensus parameters cost and buy (pyconsensus_amd.simulate.study with cells that carry
parameters of their own: pcx_simulate_study_params_f64).  Two measurements, one JSON
line each, the sides of a measurement alternating run by run on one box after a warm-up of all of them;
medians with min - max.

``--measure indirection``: the 240-cell grid of tools/bench_sweep.py (256 rounds a cell, T = 8) through
``study(grid, T, pair_with="first")`` on the shared-parameter entry (``shared``, and the same command once
more as ``shared_again``: its own spread is the yardstick) and with every cell carrying the same one
parameter set as keys (``params``: the new entry, the table read per round).  Device time from HIP events
around the call.

``--measure one_call``: a 40-cell grid under six parameter sets, as ONE study of 240 cells (``one_call``)
against six studies of 40 cells on the shared-parameter entry, one per set (``six_calls``).  Both end to
end: host clock from before the first call to after a final synchronise (HIP-event time beside it).
``--six-only`` times the six calls alone: run it with PCX_LIB on the parent's library for the parent's
code as the yardstick.

usage: python tools/bench_params.py --measure indirection|one_call [--reps 9] [--timesteps 8] [--rounds 256]
                                    [--six-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = [{"algorithm": "PCA", "alpha": 0.1}, {"algorithm": "PCA", "alpha": 0.3}, {"algorithm": "PCA", "alpha": 0.5},
        {"algorithm": "absolute"}, {"algorithm": "fixed-variance"}, {"algorithm": "hierarchical"}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", choices=("indirection", "one_call"), required=True)
    ap.add_argument("--reps", type=int, default=9, help="timed runs per side (at least 7 for a figure to keep)")
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=256, help="rounds per cell")
    ap.add_argument("--six-only", action="store_true", help="one_call: the six shared-parameter calls alone")
    a = ap.parse_args()
    T = a.timesteps

    import numpy as np
    import torch

    import pyconsensus_amd.simulate  # noqa: F401
    S = sys.modules["pyconsensus_amd.simulate"]
    assert torch.cuda.is_available(), "bench_params needs the GPU"

    def timed(fn):
        """(HIP-event ms, host ms to the end of a final synchronise, result)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, r

    if a.measure == "indirection":
        grid = S.grid(a.rounds, seed=1, liar_frac=[round(0.025 * (k + 1), 3) for k in range(20)],
                      reporters=[20, 50, 100, 200], events=[10, 20, 40])
        keyed = [dict(c, alpha=0.1, algorithm="PCA") for c in grid]
        sides = {"shared": lambda: S.study(grid, T, pair_with="first"),
                 "params": lambda: S.study(keyed, T, pair_with="first"),
                 "shared_again": lambda: S.study(grid, T, pair_with="first")}
        what = dict(grid="20 liar_frac x N {20,50,100,200} x E {10,20,40}", cells=len(grid))
    else:
        grid = S.grid(a.rounds, seed=1, liar_frac=[round(0.05 * (k + 1), 3) for k in range(10)], reporters=[50, 100],
                      events=[10, 20])
        every = [dict(c, **q) for q in SETS for c in grid]
        sides = {"six_calls": lambda: [S.study(grid, T, pair_with="first", **q) for q in SETS]}
        if not a.six_only:
            sides["one_call"] = lambda: S.study(every, T, pair_with="first")
        what = dict(grid="10 liar_frac x N {50,100} x E {10,20}", cells=len(grid), sets=len(SETS))
    for fn in sides.values():  # warm every side up: code objects, work buffers, torch's allocator
        fn()
        fn()
    torch.cuda.synchronize()
    dev, host = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(a.reps):  # alternate the sides
        for k, fn in sides.items():
            d, h, _ = timed(fn)
            dev[k].append(d)
            host[k].append(h)
    line = dict(measurement=a.measure, lib=os.environ.get("PCX_LIB", "in-tree"), rounds_per_cell=a.rounds, timesteps=T,
                reps=a.reps, **what)
    for name, ms in (("event_ms", dev), ("end_to_end_ms", host)):
        line[name] = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()}
    if a.measure == "indirection":
        m = line["event_ms"]
        line["params_over_shared"] = m["params"]["median"] / m["shared"]["median"]
        line["shared_again_over_shared"] = m["shared_again"]["median"] / m["shared"]["median"]
        x, y = sides["shared"](), sides["params"]()
        torch.cuda.synchronize()
        line["same_bytes"] = all(bool(np.array_equal(x[k].cpu().numpy(), y[k].cpu().numpy(), equal_nan=True))
                                 for k in ("metrics", "summary", "stats", "paired", "reputation"))
    elif not a.six_only:
        m = line["end_to_end_ms"]
        line["six_calls_over_one_call"] = m["six_calls"]["median"] / m["one_call"]["median"]
        six, one = sides["six_calls"](), sides["one_call"]()
        torch.cuda.synchronize()
        C = len(grid)
        line["same_bytes"] = all(bool(np.array_equal(one["summary"][:, k * C:(k + 1) * C].cpu().numpy(),
                                                     six[k]["summary"].cpu().numpy(), equal_nan=True))
                                 for k in range(len(SETS)))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
