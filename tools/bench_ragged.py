"""Cost of ragged batches (batched.consensus_ragged) against what equal-shape launches offer.

Three workloads of ``--rounds`` rounds (default 65,536), one JSON line each (DESIGN.md 5.5 records them).
Device times are HIP events around ``--calls`` library calls in a row with the inputs already on the
device (per call), medians over ``--reps`` runs after a warm-up, the two sides of a comparison run
alternately:

* ``descriptor``: one generic shape (default 48 x 20) through pcx_consensus_ragged_f64 against the
  same rounds through pcx_consensus_batched_f64 -- the same code plus the descriptor's scalar load.
* ``mixed``: shapes uniform in N in [8, 64], E in [2, 32].  The ragged launch's device time; then
  from host data, wall clock to the synchronised outputs: consensus_ragged (packing, one upload, one
  launch) against one consensus_batched launch per distinct shape (bucketing on the host included),
  and the Oracle loop on a 512-round sample.
* ``c3``: all 50 x 20 rounds, ragged (the generic instance) against the compiled instance.

``--wide``: the wide entry (rounds up to 256 x 64, pcx_consensus_ragged_wide_f64), one
JSON line each:

* ``wide_descriptor``: 4,096 rounds of 100 x 50, then 1,024 of 256 x 64, through the wide entry against
  pcx_consensus_batched_f64 on the same data (the workgroup kernel with and without the descriptor).
* ``wide_mixed``: ``--rounds`` rounds (default 8,192 here), N in [8, 256], E in [2, 64]: device time, then
  from host data against one consensus_batched launch per distinct shape and the Oracle loop on a sample.
* ``wide_classes``: 4,096 rounds of 100 x 50 and 64 of 256 x 64 in one call, one launch per launch class
  against PCX_RAGGED_ONE_CLASS=1 (one launch at the largest LDS), alternating.

usage: python tools/bench_ragged.py [--rounds 65536] [--reps 7] [--calls 8] [--shape 48x20]
                                    [--oracle-sample 512] [--wide]
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
    ap.add_argument("--rounds", type=int, default=None, help="default 65536 (8192 with --wide)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=8, help="calls in a row per timed run")
    ap.add_argument("--shape", default="48x20")
    ap.add_argument("--oracle-sample", type=int, default=None, help="default 512 (256 with --wide)")
    ap.add_argument("--wide", action="store_true", help="the wide entry's measurements instead")
    a = ap.parse_args()
    B = a.rounds or (8192 if a.wide else 65536)
    a.oracle_sample = a.oracle_sample or (256 if a.wide else 512)

    import numpy as np
    import torch

    from pyconsensus_amd import Oracle, _abi, _device, _lib, synthetic
    from pyconsensus_amd.batched import consensus_batched, consensus_ragged

    assert torch.cuda.is_available(), "bench_ragged needs the GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    names = [(n, k, dt) for n, k, dt in _abi.BATCH_OUTPUTS if n not in ("filled", "original")]

    def timed(fn):
        """Device ms per call over ``--calls`` calls in a row: a ragged call builds its descriptor table
        on the host before it enqueues anything, which an idle stream would wait out; behind the
        previous call's kernel it overlaps, as it does in a driver that keeps the stream busy."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    def result(ns, es):
        """A BatchResult over fresh device outputs for rounds of shapes (ns, es)."""
        totals = (int(ns.sum()), int(es.sum()), int((ns.astype(np.int64) * es).sum()))
        res, keep = _abi.BatchResult(), []
        for n, k, dt in names:
            x = torch.empty(_abi.ragged_out_len(k, len(ns), totals), dtype=torch.float64 if dt == "f8" else torch.int32,
                            device=dev)
            keep.append(x)
            setattr(res, n, x.data_ptr())
        return res, keep

    def ragged_call(d, ns, es, entry=None):
        entry = entry or lib.pcx_consensus_ragged_f64
        inp = _abi.Ragged(len(ns), ns.ctypes.data, es.ctypes.data, d["R"].data_ptr(), d["rep"].data_ptr(),
                          d["sc"].data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr(), 0, _abi.ALG_PCA, 0.1, 0.1, 5,
                          0.9, None, 0.5, 0.0)
        res, keep = result(ns, es)
        return lambda: _lib.check(entry(h, C.byref(inp), C.byref(res))), keep

    def batched_call(d, N, E, B=B):
        inp = _abi.Batch(B, N, E, d["R"].data_ptr(), d["rep"].data_ptr(), d["sc"].data_ptr(), d["lo"].data_ptr(),
                         d["hi"].data_ptr(), 0, 0, 0.1, 0.1, _abi.ALG_PCA, min(5, E), 0.9, None, 0.5, 0.0, 0, 0, None)
        ns, es = np.full(B, N, dtype=np.int32), np.full(B, E, dtype=np.int32)
        res, keep = result(ns, es)
        return lambda: _lib.check(lib.pcx_consensus_batched_f64(h, C.byref(inp), C.byref(res))), keep

    def upload(R, rep, sc, lo, hi):
        f = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt).reshape(-1), device=dev)
        return dict(R=f(R, np.float64), rep=f(rep, np.float64), sc=f(sc, np.uint8), lo=f(lo, np.float64),
                    hi=f(hi, np.float64))

    def alternate(fa, fb, B=B):
        fa(), fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(timed(fa))
            tb.append(timed(fb))
        s = lambda t: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                       "rounds_per_s": B / (statistics.median(t) * 1e-3)}
        return s(ta), s(tb)

    def uniform(N, E, seed, what, other):
        d = upload(*[x for x in _reorder(synthetic.rounds(B, N, E, seed=seed))])
        ns, es = np.full(B, N, dtype=np.int32), np.full(B, E, dtype=np.int32)
        fr, k1 = ragged_call(d, ns, es)
        fb, k2 = batched_call(d, N, E)
        r, b = alternate(fr, fb)
        print(json.dumps({"measurement": what, "rounds": B, "reporters": N, "events": E, "reps": a.reps, "calls": a.calls,
                          "ragged": r, other: b, "ragged_over_" + other: r["median_ms"] / b["median_ms"]}), flush=True)

    def _reorder(t):  # synthetic.rounds -> (R, rep, scaled, lo, hi)
        R, sc, lo, hi, rep = t
        return R, rep, sc, lo, hi

    def flat(parts):  # batches of different shapes -> the ragged call's flat arrays
        return [np.concatenate([np.ascontiguousarray(p[j]).reshape(-1) for p in parts]) for j in range(5)]

    def mixed_rounds(n_hi, e_hi, seed):
        """B rounds, N uniform in [8, n_hi], E in [2, e_hi]: (ns, es, per-round inputs, distinct shapes)."""
        rng = np.random.default_rng(seed)
        ns = rng.integers(8, n_hi + 1, B).astype(np.int32)
        es = rng.integers(2, e_hi + 1, B).astype(np.int32)
        rounds, shapes = [None] * B, {}
        for b in range(B):
            shapes.setdefault((int(ns[b]), int(es[b])), []).append(b)
        for k, ((N, E), idx) in enumerate(sorted(shapes.items())):
            R, sc, lo, hi, rep = synthetic.rounds(len(idx), N, E, seed=10000 + k)
            for i, b in enumerate(idx):
                rounds[b] = (R[i], rep[i], sc[i].astype(np.uint8), lo[i], hi[i])
        return ns, es, rounds, len(shapes)

    def from_host(rounds, n_shapes, ns, es, dev_ms, what, **kw):
        """Wall clock from host data to the synchronised outputs: the ragged call, one consensus_batched
        launch per distinct shape (bucketing included), the Oracle loop on a sample; prints the line."""
        col = lambda j: [r[j] for r in rounds]

        def run_ragged():
            consensus_ragged(col(0), col(1), col(2), col(3), col(4), device=dev, **kw)
            torch.cuda.synchronize()

        def run_buckets():
            groups = {}
            for b, r in enumerate(rounds):
                groups.setdefault(r[0].shape, []).append(b)
            outs = []
            for idx in groups.values():
                st = lambda j: np.stack([rounds[b][j] for b in idx])
                outs.append(consensus_batched(st(0), st(1), st(2), st(3), st(4), device=dev))
            torch.cuda.synchronize()
            return len(groups)

        def wall(fn):
            t0 = time.perf_counter()
            r = fn()
            return time.perf_counter() - t0, r

        run_ragged(), run_buckets()
        wr, wb = [], []
        for _ in range(max(3, a.reps // 2)):
            wr.append(wall(run_ragged)[0])
            t, nb = wall(run_buckets)
            wb.append(t)
        S = min(a.oracle_sample, B)

        def run_oracle():
            for R, rep, sc, lo, hi in rounds[:S]:
                Oracle(reports=R.copy(), event_bounds=synthetic.bounds_list(sc, lo, hi), reputation=rep).consensus()

        run_oracle()
        wo = wall(run_oracle)[0]
        med = statistics.median
        print(json.dumps({
            "measurement": what, "rounds": B, "distinct_shapes": n_shapes, "reps": a.reps,
            "cells": int((ns.astype(np.int64) * es).sum()),
            "ragged_device": {"median_ms": med(dev_ms), "min_ms": min(dev_ms), "max_ms": max(dev_ms),
                              "rounds_per_s": B / (med(dev_ms) * 1e-3)},
            "ragged_from_host": {"median_s": med(wr), "min_s": min(wr), "max_s": max(wr), "rounds_per_s": B / med(wr)},
            "launch_per_shape_from_host": {"launches": nb, "median_s": med(wb), "min_s": min(wb), "max_s": max(wb),
                                           "rounds_per_s": B / med(wb)},
            "oracle_loop": {"sample": S, "s": wo, "rounds_per_s": S / wo},
            "speedup_vs_launch_per_shape": med(wb) / med(wr),
            "speedup_vs_oracle_loop": (B / med(wr)) / (S / wo),
        }), flush=True)

    if a.wide:
        wide_entry = lib.pcx_consensus_ragged_wide_f64
        # ------------------------------------------------------------ W1: the descriptor's cost
        for nb, N, E, seed in ((4096, 100, 50, 41), (1024, 256, 64, 42)):
            d = upload(*_reorder(synthetic.rounds(nb, N, E, seed=seed)))
            ns, es = np.full(nb, N, dtype=np.int32), np.full(nb, E, dtype=np.int32)
            fr, k1 = ragged_call(d, ns, es, wide_entry)
            fb, k2 = batched_call(d, N, E, nb)
            r, b = alternate(fr, fb, nb)
            print(json.dumps({"measurement": "wide_descriptor", "rounds": nb, "reporters": N, "events": E,
                              "reps": a.reps, "calls": a.calls, "ragged_wide": r, "batched": b,
                              "ragged_wide_over_batched": r["median_ms"] / b["median_ms"]}), flush=True)
            del d, k1, k2
        # ------------------------------------------------------------ W2: the launch classes
        parts = [_reorder(synthetic.rounds(4096, 100, 50, seed=43)), _reorder(synthetic.rounds(64, 256, 64, seed=44))]
        d = upload(*flat(parts))
        ns = np.concatenate([np.full(4096, 100), np.full(64, 256)]).astype(np.int32)
        es = np.concatenate([np.full(4096, 50), np.full(64, 64)]).astype(np.int32)
        fr, keep = ragged_call(d, ns, es, wide_entry)

        def one_class():
            os.environ["PCX_RAGGED_ONE_CLASS"] = "1"  # (read per call)
            try:
                fr()
            finally:
                del os.environ["PCX_RAGGED_ONE_CLASS"]

        r, o = alternate(fr, one_class, len(ns))
        print(json.dumps({"measurement": "wide_classes", "rounds": len(ns),
                          "mix": "4096 x (100 x 50) + 64 x (256 x 64)", "reps": a.reps, "calls": a.calls, "per_class": r, "one_class": o,
                          "one_class_over_per_class": o["median_ms"] / r["median_ms"]}), flush=True)
        del d, keep
        # ------------------------------------------------------------ W3: mixed shapes
        ns, es, rounds, n_shapes = mixed_rounds(256, 64, 9)
        d = upload(*flat([[r[j] for j in range(5)] for r in rounds]))
        fr, keep = ragged_call(d, ns, es, wide_entry)
        fr()
        torch.cuda.synchronize()
        dev_ms = [timed(fr) for _ in range(a.reps)]
        from_host(rounds, n_shapes, ns, es, dev_ms, "wide_mixed", wide=True)
        return

    # ---------------------------------------------------------------- 1: the descriptor's cost
    N1, E1 = (int(x) for x in a.shape.split("x"))
    uniform(N1, E1, 31, "descriptor", "batched_generic")

    # ---------------------------------------------------------------- 2: mixed shapes
    ns, es, rounds, n_shapes = mixed_rounds(64, 32, 7)
    d = upload(*flat([[r[j] for j in range(5)] for r in rounds]))
    fr, keep = ragged_call(d, ns, es)
    fr()
    torch.cuda.synchronize()
    dev_ms = [timed(fr) for _ in range(a.reps)]
    from_host(rounds, n_shapes, ns, es, dev_ms, "mixed")
    del d, keep, rounds

    # ---------------------------------------------------------------- 3: the compiled shape, for the record
    uniform(50, 20, 20261015, "c3", "batched_compiled")


if __name__ == "__main__":
    main()
