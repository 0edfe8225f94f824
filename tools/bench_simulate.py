"""Cost of the on-device Monte Carlo simulator (pyconsensus_amd.simulate) at the headline shape.

Two measurements, one JSON line each (DESIGN.md "Simulator" records them):

* ``kernels``: per timestep, the device time (HIP events around each call, after a warm-up) of
  k_sim_generate, of the batched consensus alone on the rounds just generated (the three
  outputs a trajectory carries, and every output), of k_sim_metrics and of k_sim_summary (the
  metrics call with a summary minus the one without); the generator's write rate over the
  bytes it writes (reports + lo/hi/truth + scaled + liar flags).
* ``end_to_end``: rounds per second through ``simulate`` (T timesteps, device events), against
  the only route without it: ``synthetic.rounds`` on the host, the upload, ``consensus_batched``,
  the download of smooth_rep / old_rep / outcomes_final and a numpy scoring pass (one timestep;
  that generator returns neither the truth nor the liars, so the scoring runs the metric
  arithmetic on stand-ins of the same shapes).

usage: python tools/bench_simulate.py [--rounds 65536] [--reporters 50] [--events 20]
                                      [--timesteps 8] [--reps 5] [--no-host]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=65536)
    ap.add_argument("--reporters", type=int, default=50)
    ap.add_argument("--events", type=int, default=20)
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (about 10 s)")
    a = ap.parse_args()
    B, N, E, T = a.rounds, a.reporters, a.events, a.timesteps

    import numpy as np
    import torch

    from pyconsensus_amd import _abi, _device, _lib, synthetic
    from pyconsensus_amd.batched import consensus_batched
    from pyconsensus_amd.simulate import _device_rounds, _sim, simulate

    assert torch.cuda.is_available(), "bench_simulate needs the GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    p = dict(liar_frac=0.3, collude_frac=0.5, distort=0.1, na_frac=0.1, scaled_frac=0.25)
    sim = _sim(B, N, E, T, 1, scaled_tol=0.1, **p)
    rounds, cr = _device_rounds(torch, dev, B, N, E)
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    met = torch.empty((B, _abi.SIM_NMETRICS), dtype=torch.float64, device=dev)
    summ = torch.empty((_abi.SIM_NMETRICS,), dtype=torch.float64, device=dev)
    three = ("old_rep", "smooth_rep", "outcomes_final")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def gen(t):
        _lib.check(lib.pcx_sim_generate_f64(h, C.byref(sim), t, C.byref(cr)))

    def score(out, with_summary):
        _lib.check(lib.pcx_sim_metrics_f64(h, C.byref(sim), C.byref(cr), out["old_rep"].data_ptr(),
                                           out["smooth_rep"].data_ptr(), out["outcomes_final"].data_ptr(),
                                           met.data_ptr(), summ.data_ptr() if with_summary else None))

    def cons(outputs):
        return consensus_batched(rounds["reports"], None, rounds["scaled"], rounds["lo"], rounds["hi"],
                                 outputs=outputs, device=dev)

    ms = {k: [] for k in ("generate", "consensus_3", "consensus_all", "metrics", "metrics_summary")}
    for rep in range(a.reps + 1):  # rep 0 warms every call up
        for t in range(T):
            row = {}
            row["generate"], _ = timed(lambda: gen(t))
            row["consensus_3"], out = timed(lambda: cons(three))
            row["consensus_all"], _ = timed(lambda: cons(None))
            row["metrics"], _ = timed(lambda: score(out, False))
            row["metrics_summary"], _ = timed(lambda: score(out, True))
            if rep:
                for k, v in row.items():
                    ms[k].append(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    gen_bytes = B * N * E * 8 + 3 * B * E * 8 + B * E + B * N
    print(json.dumps({
        "measurement": "kernels", "rounds": B, "reporters": N, "events": E, "timesteps": T, "reps": a.reps,
        "median_ms": {"k_sim_generate": med["generate"], "consensus_batched_3_outputs": med["consensus_3"],
                      "consensus_batched_all_outputs": med["consensus_all"], "k_sim_metrics": med["metrics"],
                      "k_sim_summary": med["metrics_summary"] - med["metrics"]},
        "min_ms": {k: min(v) for k, v in ms.items()}, "max_ms": {k: max(v) for k, v in ms.items()},
        "generate_bytes": gen_bytes, "generate_GB_per_s": gen_bytes / (med["generate"] * 1e-3) / 1e9,
    }), flush=True)

    # ---------------------------------------------------------------- end to end
    def run_sim():
        return simulate(B, N, E, T, seed=1, **p)

    run_sim()
    torch.cuda.synchronize()
    e2e = [timed(run_sim)[0] for _ in range(a.reps)]
    sim_ms = statistics.median(e2e)
    res = {"measurement": "end_to_end", "rounds": B, "reporters": N, "events": E, "timesteps": T,
           "simulate_ms": sim_ms, "simulate_ms_min_max": [min(e2e), max(e2e)],
           "simulate_rounds_per_s": B * T / (sim_ms * 1e-3)}
    if not a.no_host:
        consensus_batched(rounds["reports"][:256], None, rounds["scaled"][:256], rounds["lo"][:256],
                          rounds["hi"][:256], outputs=three, device=dev)
        torch.cuda.synchronize()
        leg = {}
        t0 = time.perf_counter()
        R, sc, lo, hi, rep0 = synthetic.rounds(B, N, E, seed=1)
        leg["generate_host_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        up = [torch.as_tensor(x, device=dev) for x in (R, rep0, sc.astype(np.uint8), lo, hi)]
        torch.cuda.synchronize()
        leg["upload_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        out = consensus_batched(*up, outputs=three, device=dev)
        torch.cuda.synchronize()
        leg["consensus_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        old, smooth, outc = (out[k].cpu().numpy() for k in three)
        leg["download_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        truth = outc.copy()  # stand-ins: that generator returns no truth and no liar flags
        liars = (np.arange(B * N).reshape(B, N) % 3) == 0
        with np.errstate(invalid="ignore"):
            ok = np.where(sc, np.abs(outc - truth) <= 0.1 * (hi - lo), outc == truth)
        before, after = np.zeros(B), np.zeros(B)
        for i in range(N):
            before = np.where(liars[:, i], before + old[:, i], before)
            after = np.where(liars[:, i], after + smooth[:, i], after)
        m = np.stack([ok.sum(axis=1) / float(E), before, after, after - before, (after > before) * 1.0,
                      liars.sum(axis=1) * 1.0], axis=1)
        m.mean(axis=0)
        leg["scoring_s"] = time.perf_counter() - t0
        total = sum(leg.values())
        res.update(host_route=leg, host_route_s_per_timestep=total, host_route_rounds_per_s=B / total,
                   speedup=(B * T / (sim_ms * 1e-3)) / (B / total))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
