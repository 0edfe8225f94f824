"""Throughput of batched rounds above the one-wavefront kernel: B rounds of N x E through
pcx_consensus_batched_f64 on the workgroup-per-round kernel (csrc/pcx_medium.hip), then on the
worker-stream scheduler (csrc/pcx_rounds.cpp, PCX_NO_MEDIUM=1) at several pool sizes.

usage: python tools/bench_rounds.py [B] [N] [E] [wg] [--algorithm NAME] [--reps R]
                                    [--sched-rounds S] [--workers 1,4,8,16,32] [--tall]
One JSON line per path / pool size, with every timed repetition, their median and spread
(max - min); "wg": the workgroup kernel only.  --tall: rounds of 257 to 1024 reporters on the tall
form of the workgroup kernel (csrc/pcx_tall.hip, tall=True) where the route takes them, then the
scheduler as the default route runs them.  The scheduler runs S rounds (default B).  k-means
draws its kmeans_init once, outside the timed region.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("B", nargs="?", type=int, default=1024)
    ap.add_argument("N", nargs="?", type=int, default=100)
    ap.add_argument("E", nargs="?", type=int, default=50)
    ap.add_argument("mode", nargs="?", default="all", choices=("all", "wg"))
    ap.add_argument("--algorithm", default="PCA")
    ap.add_argument("--reps", type=int, default=1, help="timed repetitions per line")
    ap.add_argument("--sched-rounds", type=int, default=None, help="rounds the scheduler runs (default B)")
    ap.add_argument("--workers", default="1,4,8,16,32", help="scheduler pool sizes")
    ap.add_argument("--tall", action="store_true", help="time the tall route (tall=True) before the scheduler")
    a = ap.parse_args()
    B, N, E = a.B, a.N, a.E
    import numpy as np
    import torch

    from pyconsensus_amd import _lib, synthetic
    from pyconsensus_amd.batched import consensus_batched, kmeans_draws, route

    R, sc, lo, hi, rep = synthetic.rounds(B, N, E, seed=3)
    dev = torch.device("cuda", 0)
    Rt, rt = torch.as_tensor(R, device=dev), torch.as_tensor(rep, device=dev)
    sct, lot, hit = (torch.as_tensor(x, device=dev) for x in (sc.astype("uint8"), lo, hi))
    kw = dict(algorithm=a.algorithm)
    kinit = None
    if a.algorithm == "k-means":
        kinit = torch.as_tensor(kmeans_draws(B, N, random_state=np.random.RandomState(3)), device=dev)
    if a.algorithm == "hierarchical":
        kw["hierarchy_threshold"] = 1.5 if E >= 33 else 0.5

    def run(nb, **more):
        if kinit is not None:
            kw["kmeans_init"] = kinit[:nb]
        consensus_batched(Rt[:nb], rt[:nb], sct[:nb], lot[:nb], hit[:nb], **kw, **more)
        torch.cuda.synchronize()

    def timed(nb, **more):
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            run(nb, **more)
            ts.append(time.perf_counter() - t0)
        med = statistics.median(ts)
        return {"rounds": nb, "N": N, "E": E, "algorithm": a.algorithm, "seconds": med, "rounds_per_s": nb / med,
                "spread_s": max(ts) - min(ts), "all_s": ts}

    # the workgroup-per-round kernel, N <= 256, E <= 64 (PCX_LIB builds before the route query: assumed)
    if not hasattr(_lib.lib(), "pcx_batched_route") or route(N, E, a.algorithm) == "workgroup":
        for _ in range(2):
            run(B)
        print(json.dumps(dict(timed(B), path="workgroup kernel")), flush=True)
    if a.tall and route(N, E, a.algorithm, tall=True) == "tall":
        for _ in range(2):
            run(B, tall=True)
        print(json.dumps(dict(timed(B, tall=True), path="tall kernel")), flush=True)
    if a.mode == "wg":
        return
    os.environ["PCX_NO_MEDIUM"] = "1"  # the worker-stream scheduler (csrc/pcx_rounds.cpp)
    S = B if a.sched_rounds is None else min(a.sched_rounds, B)
    for workers in (int(w) for w in a.workers.split(",")):
        os.environ["PCX_ROUND_WORKERS"] = str(workers)
        _lib._ctx.clear()  # fresh context: the pool size is read when it grows
        run(min(workers, S))  # warm
        print(json.dumps(dict(timed(S), path="scheduler", workers=workers)), flush=True)


if __name__ == "__main__":
    main()
