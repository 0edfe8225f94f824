"""What k-means in ragged batches and in the simulator costs and buys.  One JSON
line per measurement, the sides of a measurement alternating run by run in one process after a warm-up
of all of them; medians with min - max, as tools/bench_params.py.

``--measure ragged``: tools/bench_ragged.py's mix (rounds of many distinct shapes, N uniform in [8, 64],
E in [2, 32]) under k-means with the reference's 20 restarts.  ``ragged``: ONE
``consensus_ragged(kmeans_init=...)`` call; ``buckets``: one ``consensus_batched`` per distinct shape
(the equal-shape kernel, which this change leaves as it was).  ``device``: the inputs and the books
are on the device already, HIP events around the launches (the ragged side through
pcx_consensus_ragged_kmeans_f64 directly; the buckets through consensus_batched with device tensors
and two outputs).  ``host``: numpy in, host clock to a final synchronise.

``--measure study``: a grid under {PCA, k-means} as ONE ``study(pair_with="first", kmeans_restarts=R)``
(``one_study``) against what the library allowed before: PCA by ``study`` and k-means by the
host-driven loop, cell by cell and timestep by timestep (``generate`` ->
``consensus_batched(kmeans_init=kmeans_books_host(...))`` -> ``metrics``, smooth_rep carried)
(``pca_study_plus_host_loop``).  Host clock to a final synchronise.  ``--study-only`` runs ``one_study``
alone ``--reps`` times: the command for a ``rocprofv3 --kernel-trace --stats`` run of its own, which
tells the books kernel's share of a timestep.

The headline is untouched by construction (every existing kernel keeps its code:
profiles/kmeans_ragged/resources.txt); ``bench.py --gpus 1`` with PCX_LIB on the parent's library and on
this one alternately is the measurement of it.

usage: python tools/bench_kmeans.py --measure ragged|study [--reps 9] [--rounds 4096] [--restarts 20]
                                    [--timesteps 4] [--study-only]
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
    ap.add_argument("--measure", choices=("ragged", "study"), required=True)
    ap.add_argument("--reps", type=int, default=9, help="timed runs per side (at least 7 for a figure to keep)")
    ap.add_argument("--rounds", type=int, default=4096, help="ragged: rounds of the mix; study: rounds per cell / 16")
    ap.add_argument("--restarts", type=int, default=20)
    ap.add_argument("--timesteps", type=int, default=4)
    ap.add_argument("--study-only", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch

    import pyconsensus_amd.simulate  # noqa: F401
    from pyconsensus_amd import _abi, _device, _lib, synthetic
    from pyconsensus_amd.batched import (_params_array, consensus_batched, consensus_ragged, kmeans_draws_ragged,
                                         param_sets)

    S = sys.modules["pyconsensus_amd.simulate"]
    assert torch.cuda.is_available(), "bench_kmeans needs the GPU"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, r

    def run(sides, line, which):
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
        for name, ms in (("event_ms", dev), ("end_to_end_ms", host)):
            if name in which:
                line[name] = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()}
        return line

    if a.measure == "ragged":
        B = a.rounds
        rng = np.random.default_rng(7)
        ns, es = rng.integers(8, 65, B), rng.integers(2, 33, B)
        shapes = {}
        for b in range(B):
            shapes.setdefault((int(ns[b]), int(es[b])), []).append(b)
        rounds = [None] * B
        per_shape = {}
        for k, ((N, E), idx) in enumerate(sorted(shapes.items())):
            R, sc, lo, hi, rep = synthetic.rounds(len(idx), N, E, seed=100 + k)
            per_shape[(N, E)] = (R, rep, sc, lo, hi)
            for r, b in enumerate(idx):
                rounds[b] = (R[r], rep[r], sc[r], lo[r], hi[r])
        books = kmeans_draws_ragged([int(n) for n in ns], a.restarts, np.random.RandomState(1))
        lists = [[rounds[b][k] for b in range(B)] for k in range(5)]
        shape_books = {s: np.stack([books[b] for b in idx]) for s, idx in shapes.items()}
        want = ("smooth_rep", "outcomes_final")

        # host data: numpy in, a final synchronise
        host_sides = {
            "ragged": lambda: consensus_ragged(*lists, algorithm="k-means", kmeans_init=books, outputs=want),
            "buckets": lambda: [consensus_batched(*per_shape[s], algorithm="k-means", kmeans_init=shape_books[s],
                                                  outputs=want) for s in sorted(shapes)]}
        line = dict(measurement="ragged_kmeans", rounds=B, distinct_shapes=len(shapes), restarts=a.restarts,
                    reps=a.reps, lib=os.environ.get("PCX_LIB", "in-tree"))
        run(host_sides, line, ("end_to_end_ms",))

        # device data: everything resident, events around the launches
        first = consensus_ragged(*lists, algorithm="k-means", kmeans_init=books, outputs=want)
        torch.cuda.synchronize()
        Rd, repd, scd, lod, hid, _, kmd = first["_inputs"]
        n32, e32 = np.ascontiguousarray(ns, dtype=np.int32), np.ascontiguousarray(es, dtype=np.int32)
        inp = _abi.Ragged(B, n32.ctypes.data, e32.ctypes.data, Rd.data_ptr(), repd.data_ptr(), scd.data_ptr(),
                          lod.data_ptr(), hid.data_ptr(), 0, 0, 0.1, 0.1, 5, 0.9, None, 0.5, 0.0)
        sets, of = param_sets([None] * B, dict(algorithm="k-means", catch_tolerance=0.1, alpha=0.1, max_components=5,
                                               variance_threshold=0.9, hierarchy_threshold=0.5,
                                               cluster_threshold=None), "per_round")
        arr = _params_array(sets)
        kb = _abi.KmeansBooks(a.restarts, None, kmd.data_ptr())
        res = _abi.BatchResult()
        res.smooth_rep, res.outcomes_final = first["smooth_rep"].data_ptr(), first["outcomes_final"].data_ptr()
        h = _lib.bind_stream(0, _device.current_stream_handle(torch.device("cuda", 0)))

        def ragged_device():
            _lib.check(_lib.lib().pcx_consensus_ragged_kmeans_f64(h, C.byref(inp), len(sets), C.cast(arr, C.c_void_p),
                                                                  of.ctypes.data, C.byref(kb), C.byref(res)))

        dev_in = {s: tuple(torch.as_tensor(x).cuda() for x in per_shape[s]) + (torch.as_tensor(shape_books[s]).cuda(),)
                  for s in shapes}

        def buckets_device():
            return [consensus_batched(*dev_in[s][:5], algorithm="k-means", kmeans_init=dev_in[s][5], outputs=want)
                    for s in sorted(shapes)]

        dline = {}
        run({"ragged": ragged_device, "buckets": buckets_device}, dline, ("event_ms",))
        line["event_ms"] = dline["event_ms"]
        for name in ("event_ms", "end_to_end_ms"):
            line["buckets_over_ragged_" + name] = line[name]["buckets"]["median"] / line[name]["ragged"]["median"]
        print(json.dumps(line), flush=True)
        return

    # ---------------------------------------------------------------- study
    T, R = a.timesteps, max(a.rounds // 16, 1)
    grid = S.grid(R, seed=1, liar_frac=[0.1, 0.2, 0.3, 0.4, 0.5], reporters=[20, 50], events=[10, 20])
    both = [dict(c, algorithm=alg) for c in grid for alg in ("PCA", "k-means")]

    def one_study():
        return S.study(both, T, pair_with="first", kmeans_restarts=a.restarts)

    def host_loop():
        out = [S.study(grid, T)]
        for c in grid:
            rep = None
            rates = {k: c[k] for k in ("liar_frac",)}
            for t in range(T):
                g = S.generate(c["rounds"], c["reporters"], c["events"], t=t, seed=c["seed"], **rates)
                o = consensus_batched(g["reports"], rep, g["scaled"], g["lo"], g["hi"], algorithm="k-means",
                                      kmeans_init=S.kmeans_books_host(c["rounds"], c["reporters"], t=t, seed=c["seed"],
                                                                      restarts=a.restarts),
                                      outputs=("old_rep", "smooth_rep", "outcomes_final"))
                out.append(S.metrics(g, o["old_rep"], o["smooth_rep"], o["outcomes_final"]))
                rep = o["smooth_rep"]
        return out

    sides = {"one_study": one_study}
    if not a.study_only:
        sides["pca_study_plus_host_loop"] = host_loop
    line = dict(measurement="study_kmeans", cells=len(grid), rounds_per_cell=R, timesteps=T, restarts=a.restarts,
                reps=a.reps, grid="5 liar_frac x N {20,50} x E {10,20} x {PCA, k-means}",
                lib=os.environ.get("PCX_LIB", "in-tree"))
    run(sides, line, ("event_ms", "end_to_end_ms"))
    if not a.study_only:
        m = line["end_to_end_ms"]
        line["host_loop_over_one_study"] = m["pca_study_plus_host_loop"]["median"] / m["one_study"]["median"]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
