"""Batched Monte Carlo regime: B independent oracle rounds in one launch.

Each round is exactly ``Oracle(reports[b], event_bounds_b, reputation[b]).consensus()``
(pyconsensus/__init__.py:102-611).  This is the regime of Simulator.jl-style Monte
Carlo drivers (README.rst:52-56), which loop consensus() over many random rounds.
Rounds of at most 64 reporters x 32 events run in one wavefront each of
``batched_round_kernel`` (csrc/pcx_batched.hip); rounds up to 256 x 64 in one workgroup each of
``medium_round_kernel`` (csrc/pcx_medium.hip), every algorithm (k-means with up to 16 codes);
larger rounds run as single-matrix consensuses, many in flight on a pool of worker streams
(csrc/pcx_rounds.cpp).  :func:`route` tells which of the three a shape takes.
Rounds of DIFFERENT shapes (each at most 64 x 32) run in one launch of the one-wave kernel through
:func:`consensus_ragged`; with ``wide=True`` rounds up to 256 x 64 join them, on the ragged form of
the workgroup kernel.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _device, _lib

MAX_REPORTERS = 64  # one wavefront per round up to here (and MAX_EVENTS)
MAX_EVENTS = 32
WIDE_MAX_REPORTERS = 256  # one workgroup per round up to here (and WIDE_MAX_EVENTS)
WIDE_MAX_EVENTS = 64


def kmeans_k(N):
    """Code-book size of the reference's k-means, int(ceil(sqrt(N))) (__init__.py:396)."""
    return int(np.ceil(np.sqrt(N)))


kmeans_k_default = kmeans_k  # (route()'s parameter shadows the name)


def kmeans_draws(B, N, restarts=_abi.KMEANS_RESTARTS, random_state=None):
    """Initial code-book rows of B k-means rounds, [B][restarts][k] int32.

    scipy.cluster.vq.kmeans(obs, k) (seed=None, __init__.py:397) draws each restart's
    code book as ``rng.choice(N, size=k, replace=False)`` on numpy's global RandomState;
    these are the same draws in the same order (round after round), so a batch consumes
    the global stream exactly as B sequential reference consensus() calls would."""
    rs = np.random.mtrand._rand if random_state is None else random_state
    k = kmeans_k(N)
    out = np.empty((B, restarts, k), dtype=np.int32)
    for b in range(B):
        for r in range(restarts):
            out[b, r] = rs.choice(N, size=k, replace=False)
    return out


ROUTES = ("wave", "workgroup", "scheduler")  # include/pcx.h enum pcx_route


def route(N, E, algorithm="PCA", kmeans_k=None):
    """Where ``consensus_batched`` runs rounds of N x E: ``"wave"`` (one wavefront per round, up to
    64 x 32) and ``"workgroup"`` (one workgroup per round, up to 256 x 64; k-means with at most 16
    codes) are ONE asynchronous kernel launch; ``"scheduler"`` is the host-driven round scheduler,
    which returns once every output is written.  ``kmeans_k`` defaults to :func:`kmeans_k` (N).
    Needs no GPU; raises ValueError for arguments ``consensus_batched`` refuses."""
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    k = kmeans_k_default(N) if kmeans_k is None else int(kmeans_k)
    r = _lib.lib().pcx_batched_route(int(N), int(E), alg, k)
    if r < 0:
        raise ValueError("no batched route for %d x %d rounds, algorithm %r, kmeans_k %d" % (N, E, algorithm, k))
    return ROUTES[r]


def clusterfeck_threshold(E):
    """The reference's default leader-clustering cut (__init__.py:187-190, 210-213)."""
    t = np.log10(E) / 1.77
    return 0.3 if t == 0 else float(t)


def consensus_batched(reports, reputation=None, scaled=None, lo=None, hi=None,
                      catch_tolerance=0.1, alpha=0.1, int_dtype=False, algorithm="PCA",
                      outputs=None, device=None, filled=False, original=False,
                      max_components=5, variance_threshold=0.9, aux_scores=None,
                      hierarchy_threshold=0.5, kmeans_init=None, cluster_threshold=None, packed=False):
    """Run B rounds of N x E reports on the GPU.

    reports:    (B, N, E) float64, NaN = missing (0.0 is missing too, as in the reference)
    reputation: (B, N) raw weights or None (uniform)
    scaled/lo/hi: event bounds, (B, E) or (E,) shared by every round; None = all binary
    outputs:    iterable of result names to produce (default: all vector/scalar outputs)
    algorithm:  "PCA" (default), "absolute", "big-five", "fixed-variance", "cokurtosis"
                (__init__.py:368-457), "k-means", "hierarchical", "clusterfeck" (:392-428);
                max_components is capped at E like Oracle (:134-137); aux_scores (B, N)
                are aux["cokurt"] of each round
    kmeans_init: (B, restarts, k) initial code-book rows (default: :func:`kmeans_draws`
                on numpy's global RandomState, as the reference's scipy call draws them)
    cluster_threshold: clusterfeck's cut (default: the reference's log10(E)/1.77 rule)
    packed:     numpy inputs travel to the device in ONE copy and every output is a view of ONE
                device buffer (``out["_packed"]``; :func:`unpack_round` brings it back in one
                copy) -- the drop-in's per-call path, where each separate small copy costs ~10 us

    Returns a dict of torch tensors on the device, named like the ABI fields
    (``smooth_rep``, ``outcomes_final``, ...).  Three regimes (:func:`route`):
    rounds up to 64 x 32 (one wave per round) and up to 256 x 64 (one workgroup per round; every
    algorithm, the clusterings included, k-means with code books of at most 16 rows -- the
    reference's own ceil(sqrt(N)) up to there; kmeans_init is read on the device) are ONE kernel
    launch, asynchronous on torch's current stream -- synchronise before reading the outputs on
    the host; the round scheduler (rounds above 256 x 64, k-means with larger code books) returns
    only once every output is written.
    """
    t = _device.require_gpu()
    dev = t.device(device) if device is not None else t.device("cuda", t.cuda.current_device())
    if packed and all(x is None or isinstance(x, np.ndarray) for x in (reports, reputation, scaled, lo, hi)):
        reports, reputation, scaled, lo, hi = _upload_packed(
            [(reports, np.float64), (reputation, np.float64), (scaled, np.uint8), (lo, np.float64),
             (hi, np.float64)], dev)
    R = _device.as_device(reports, t.float64, dev)
    if R.dim() != 3:
        raise ValueError("reports must be (B, N, E)")
    B, N, E = R.shape
    if N < 1 or E < 1:
        raise ValueError("batched rounds need N >= 1 and E >= 1 (got %d x %d)" % (N, E))
    rep = _device.as_device(reputation, t.float64, dev)
    if rep is not None and tuple(rep.shape) != (B, N):
        raise ValueError("reputation must be (B, N)")
    shared = 0
    sc = lo_ = hi_ = None
    if scaled is not None:
        sc = _device.as_device(scaled, t.uint8, dev)
        lo_ = _device.as_device(lo, t.float64, dev)
        hi_ = _device.as_device(hi, t.float64, dev)
        shared = int(sc.dim() == 1)
        want = (E,) if shared else (B, E)
        for a in (sc, lo_, hi_):
            if tuple(a.shape) != want:
                raise ValueError("scaled/lo/hi must all be %s" % (want,))
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    aux = None
    if alg == _abi.ALG_COKURTOSIS:
        if aux_scores is None:
            raise ValueError("cokurtosis needs aux_scores (aux['cokurt'] of every round)")
        aux = _device.as_device(aux_scores, t.float64, dev)
        if tuple(aux.shape) != (B, N):
            raise ValueError("aux_scores must be (B, N)")
    kinit = None
    k = restarts = 0
    if alg == _abi.ALG_KMEANS:
        if kmeans_init is None:
            kmeans_init = kmeans_draws(B, N)
        kinit = _device.as_device(kmeans_init, t.int32, dev)
        if kinit.dim() != 3 or kinit.shape[0] != B:
            raise ValueError("kmeans_init must be (B, restarts, k)")
        restarts, k = int(kinit.shape[1]), int(kinit.shape[2])
        if not (1 <= k <= N) or restarts < 1 or int(kinit.min()) < 0 or int(kinit.max()) >= N:
            raise ValueError("kmeans_init rows must lie in [0, N) with 1 <= k <= N")
    cthr = clusterfeck_threshold(E) if cluster_threshold is None else float(cluster_threshold)
    mc = int(max_components) if E >= int(max_components) else E  # __init__.py:134-137
    inp = _abi.Batch(B, N, E, _device.ptr(R), _device.ptr(rep), _device.ptr(sc), _device.ptr(lo_),
                     _device.ptr(hi_), shared, int(bool(int_dtype)), float(catch_tolerance),
                     float(alpha), alg, mc, float(variance_threshold), _device.ptr(aux),
                     float(hierarchy_threshold), cthr, k, restarts, _device.ptr(kinit))
    res = _abi.BatchResult()
    outs = {}
    want = [(name, kind, dt) for name, kind, dt in _abi.BATCH_OUTPUTS
            if not (name == "filled" and not filled or name == "original" and not original)
            and not (outputs is not None and name not in outputs and name not in ("filled", "original"))]
    if packed:  # one device buffer, one 16-byte-aligned view per output
        layout, off = [], 0
        for name, kind, dt in want:
            shape = _abi.out_shape(kind, B, N, E)
            nb = int(np.prod(shape)) * (8 if dt == "f8" else 4)
            layout.append((name, off, nb, dt, shape))
            off += (nb + 15) // 16 * 16
        buf = t.empty(max(off, 16), dtype=t.uint8, device=dev)
        for name, o, nb, dt, shape in layout:
            x = buf[o:o + nb].view(t.float64 if dt == "f8" else t.int32).view(shape)
            outs[name] = x
            setattr(res, name, x.data_ptr())
        outs["_packed"] = buf
        outs["_layout"] = layout
    else:
        for name, kind, dt in want:
            tdt = t.float64 if dt == "f8" else t.int32
            x = t.empty(_abi.out_shape(kind, B, N, E), dtype=tdt, device=dev)
            outs[name] = x
            setattr(res, name, x.data_ptr())
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    _lib.check(_lib.lib().pcx_consensus_batched_f64(h, C.byref(inp), C.byref(res)))
    outs["_inputs"] = (R, rep, sc, lo_, hi_, aux, kinit)  # keep inputs alive until the caller syncs
    return outs


def _upload_packed(items, dev):
    """numpy arrays (or None) -> device tensors, as views of ONE host-to-device copy."""
    t = _device.torch()
    parts, off = [], 0
    for a, dt in items:
        if a is None:
            parts.append(None)
            continue
        a = np.ascontiguousarray(a, dtype=dt)
        parts.append((a, off))
        off += (a.nbytes + 15) // 16 * 16
    host = np.empty(max(off, 16), dtype=np.uint8)
    for p in parts:
        if p is not None:
            host[p[1]:p[1] + p[0].nbytes] = p[0].reshape(-1).view(np.uint8)
    d = t.from_numpy(host).to(dev)
    tdt = {np.float64: t.float64, np.uint8: t.uint8}
    return [None if p is None else d[p[1]:p[1] + p[0].nbytes].view(tdt[dt]).view(p[0].shape)
            for p, (_, dt) in zip(parts, items)]


def unpack_round(out, b=0):
    """Round ``b`` of a ``packed=True`` result as numpy arrays, from ONE device-to-host copy."""
    host = out["_packed"].cpu().numpy()
    g = {}
    for name, o, nb, dt, shape in out["_layout"]:
        g[name] = host[o:o + nb].view(np.float64 if dt == "f8" else np.int32).reshape(shape)[b]
    return g


# ---------------------------------------------------------------- ragged batches
def _ragged_vectors(seq, counts, dtype, what):
    """B vectors of lengths ``counts`` (or None) -> one flat array, round after round."""
    if seq is None:
        return None
    if len(seq) != len(counts):
        raise ValueError("%s must hold one vector per round (%d), got %d" % (what, len(counts), len(seq)))
    parts = []
    for b, (v, n) in enumerate(zip(seq, counts)):
        v = np.asarray(v, dtype=dtype)
        if v.ndim != 1 or v.shape[0] != n:
            raise ValueError("%s[%d] must be a vector of length %d, got shape %s" % (what, b, n, v.shape))
        parts.append(v)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)


def ragged_plan(shapes, algorithm="PCA", wide=False):
    """(totals, lds_bytes) of a ragged batch of ``shapes`` [(N_b, E_b), ...]: totals = (sum N_b,
    sum E_b, sum N_b * E_b), the flat arrays' lengths, and the launch's dynamic LDS.  Needs no GPU;
    raises PcxError naming the first round the one-wave kernel does not take (or k-means).

    ``wide=True``: rounds up to 256 x 64 (pcx_ragged_plan_wide); returns (totals, counts, lds_bytes)
    with 4-tuples counts / lds_bytes: index 0 the rounds of at most 64 x 32 (the one-wave kernel's
    launch), index c = 1..3 the workgroup kernel's rounds of launch class c -- c rounds per CU by
    their LDS -- and that launch's dynamic LDS."""
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    sh = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    if wide:
        totals, counts, lds4, bad = (C.c_int64 * 3)(), (C.c_int64 * 4)(), (C.c_int64 * 4)(), C.c_int64(-1)
        _lib.check(_lib.lib().pcx_ragged_plan_wide(len(sh), n.ctypes.data, e.ctypes.data, alg, totals, counts, lds4,
                                                   C.byref(bad)))
        return tuple(int(x) for x in totals), tuple(int(x) for x in counts), tuple(int(x) for x in lds4)
    totals, lds, bad = (C.c_int64 * 3)(), C.c_int64(0), C.c_int64(-1)
    _lib.check(_lib.lib().pcx_ragged_plan(len(sh), n.ctypes.data, e.ctypes.data, alg, totals, C.byref(lds),
                                          C.byref(bad)))
    return tuple(int(x) for x in totals), int(lds.value)


def param_sets(entries, defaults, what):
    """De-duplicate per-round (or per-cell) parameter dicts into parameter sets: ``entries`` is a
    sequence of dicts over ``_abi.PARAM_KEYS`` (or None), a missing key takes ``defaults[key]``.
    Returns (the sets as full dicts, in order of first use; int32 index of each entry's set)."""
    sets, index, of = [], {}, np.zeros(len(entries), dtype=np.int32)
    for b, d in enumerate(entries):
        d = {} if d is None else dict(d)
        unknown = sorted(set(d) - set(_abi.PARAM_KEYS))
        if unknown:
            raise ValueError("%s[%d]: unknown parameter(s) %s (allowed: %s)"
                             % (what, b, ", ".join(unknown), ", ".join(_abi.PARAM_KEYS)))
        full = dict(defaults, **d)
        key = tuple(full[k] for k in _abi.PARAM_KEYS)
        if key not in index:
            index[key] = len(sets)
            sets.append(full)
        of[b] = index[key]
    return sets, of


def _params_array(sets):
    return (_abi.RoundParams * max(len(sets), 1))(*[_abi.round_params(q) for q in sets])


def ragged_plan_params(shapes, sets, param_of):
    """(totals, n_launches) of a ragged batch of ``shapes`` whose round b takes ``sets[param_of[b]]``
    (full dicts over ``_abi.PARAM_KEYS``; pcx_ragged_plan_params, wide limits).  Needs no GPU; raises
    PcxError naming the first offending round or parameter set."""
    sh = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    of = np.ascontiguousarray(param_of, dtype=np.int32)
    arr = _params_array(sets)
    totals, nl, bad_r, bad_p = (C.c_int64 * 3)(), C.c_int64(0), C.c_int64(-1), C.c_int64(-1)
    _lib.check(_lib.lib().pcx_ragged_plan_params(len(sh), n.ctypes.data, e.ctypes.data, len(sets),
                                                 C.cast(arr, C.c_void_p), of.ctypes.data, totals, C.byref(nl),
                                                 C.byref(bad_r), C.byref(bad_p)))
    return tuple(int(x) for x in totals), int(nl.value)


def consensus_ragged(reports, reputation=None, scaled=None, lo=None, hi=None, *, catch_tolerance=0.1, alpha=0.1,
                     int_dtype=False, algorithm="PCA", outputs=None, device=None, filled=False, original=False,
                     max_components=5, variance_threshold=0.9, aux_scores=None, hierarchy_threshold=0.5,
                     cluster_threshold=None, wide=False, per_round=None):
    """Run B rounds of DIFFERENT shapes in one launch of the one-wave round kernel.

    reports:    a sequence of B arrays, round b an (N_b, E_b) matrix with N_b <= 64, E_b <= 32
    wide:       True: rounds up to 256 x 64 (pcx_consensus_ragged_wide_f64).  Those above 64 x 32
                run one workgroup each on the ragged form of ``medium_round_kernel``, one launch per
                launch class (:func:`ragged_plan`); the others on the one-wave kernel as before.
                Every round equals its own ``consensus_batched`` run.  Calls share one per-context
                scratch: keep them on one stream
    reputation: a sequence of B vectors (N_b,) or None (uniform in every round)
    scaled/lo/hi: sequences of B vectors (E_b,) or None (every event binary)
    aux_scores: cokurtosis: a sequence of B vectors (N_b,)
    per_round:  a sequence of B dicts (or None) over "algorithm", "catch_tolerance", "alpha",
                "max_components", "variance_threshold", "hierarchy_threshold", "cluster_threshold":
                round b's own consensus parameters, a missing key taking the call's keyword value
                (pcx_consensus_ragged_params_f64: still one call, and no more launches for more
                sets).  Round b equals round b of the same call with its set as the keywords.
                ``aux_scores`` is needed if some round's algorithm is cokurtosis (an entry of a
                round that is not may be None).  ``wide=False`` keeps the 64 x 32 limit
    algorithm:  as :func:`consensus_batched` but "k-means" (its code-book size depends on N_b);
                "big-five" caps max_components at E_b per round, "clusterfeck" takes the reference's
                log10(E_b)/1.77 cut per round unless cluster_threshold is given

    Each round is exactly its own ``Oracle(...).consensus()``: nothing is padded.  The inputs travel
    to the device in one copy.  Returns flat device tensors named as in :func:`consensus_batched`,
    every round's values end to end in round order (per-reporter outputs [sum N_b], per-event outputs
    [sum E_b], ``original`` / ``filled`` [sum N_b * E_b], the rest [B]), all views of one device
    buffer ``"_packed"``; ``"_shapes"`` (B, 2) and the int64 [B + 1] offsets ``"_reporter_offsets"``,
    ``"_event_offsets"``, ``"_cell_offsets"``.  :func:`ragged_round` slices one round out;
    :func:`ragged_to_host` brings everything back in one copy.  Asynchronous on torch's current
    stream, like the one-wave regime of :func:`consensus_batched`."""
    mats = []
    for b, r in enumerate(reports):
        r = np.asarray(r, dtype=np.float64)
        if r.ndim != 2:
            raise ValueError("reports[%d] must be an (N, E) matrix, got shape %s" % (b, r.shape))
        mats.append(r)
    B = len(mats)
    shapes = np.array([m.shape for m in mats], dtype=np.int32).reshape(B, 2)
    ns, es = np.ascontiguousarray(shapes[:, 0]), np.ascontiguousarray(shapes[:, 1])
    rep = _ragged_vectors(reputation, ns, np.float64, "reputation")
    if (scaled is None) != (lo is None) or (scaled is None) != (hi is None):
        raise ValueError("scaled, lo and hi are given together or not at all")
    sc = _ragged_vectors(scaled, es, np.uint8, "scaled")
    lo_ = _ragged_vectors(lo, es, np.float64, "lo")
    hi_ = _ragged_vectors(hi, es, np.float64, "hi")
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    sets = param_of = None
    if per_round is not None:
        if len(per_round) != B:
            raise ValueError("per_round must hold one entry per round (%d), got %d" % (B, len(per_round)))
        sets, param_of = param_sets(per_round, dict(
            algorithm=algorithm, catch_tolerance=catch_tolerance, alpha=alpha, max_components=max_components,
            variance_threshold=variance_threshold, hierarchy_threshold=hierarchy_threshold,
            cluster_threshold=cluster_threshold), "per_round")
    aux = None
    if alg == _abi.ALG_COKURTOSIS if sets is None else any(q["algorithm"] == "cokurtosis" for q in sets):
        if aux_scores is None:
            raise ValueError("cokurtosis needs aux_scores (aux['cokurt'] of every round)")
        if sets is not None:  # read for the cokurtosis rounds only
            if len(aux_scores) != B:
                raise ValueError("aux_scores must hold one vector per round (%d), got %d" % (B, len(aux_scores)))
            aux_scores = [np.zeros(n) if v is None and sets[param_of[b]]["algorithm"] != "cokurtosis" else v
                          for b, (v, n) in enumerate(zip(aux_scores, ns))]
        aux = _ragged_vectors(aux_scores, ns, np.float64, "aux_scores")
    if sets is None:
        totals = ragged_plan(shapes, algorithm, wide=wide)[0]  # refuses k-means and rounds past the limits, by index
    else:
        if not wide:
            ragged_plan(shapes, "PCA", wide=False)  # the one-wave limits, by index
        totals = ragged_plan_params(shapes, sets, param_of)[0]  # refuses by round or by parameter set
    t = _device.require_gpu()
    dev = t.device(device) if device is not None else t.device("cuda", t.cuda.current_device())
    flat = np.concatenate([m.reshape(-1) for m in mats]) if B else np.zeros(0)
    R, rep_d, sc_d, lo_d, hi_d, aux_d = _upload_packed(
        [(flat, np.float64), (rep, np.float64), (sc, np.uint8), (lo_, np.float64), (hi_, np.float64),
         (aux, np.float64)], dev)
    inp = _abi.Ragged(B, ns.ctypes.data, es.ctypes.data, _device.ptr(R), _device.ptr(rep_d), _device.ptr(sc_d),
                      _device.ptr(lo_d), _device.ptr(hi_d), int(bool(int_dtype)), alg, float(catch_tolerance),
                      float(alpha), int(max_components), float(variance_threshold), _device.ptr(aux_d),
                      float(hierarchy_threshold), 0.0 if cluster_threshold is None else float(cluster_threshold))
    res = _abi.BatchResult()
    want = [(name, kind, dt) for name, kind, dt in _abi.BATCH_OUTPUTS
            if not (name == "filled" and not filled or name == "original" and not original)
            and not (outputs is not None and name not in outputs and name not in ("filled", "original"))]
    layout, off = [], 0
    for name, kind, dt in want:
        n = _abi.ragged_out_len(kind, B, totals)
        nb = n * (8 if dt == "f8" else 4)
        layout.append((name, off, nb, dt, (n,)))
        off += (nb + 15) // 16 * 16
    buf = t.empty(max(off, 16), dtype=t.uint8, device=dev)
    outs = {}
    for name, o, nb, dt, shape in layout:
        x = buf[o:o + nb].view(t.float64 if dt == "f8" else t.int32)
        outs[name] = x
        setattr(res, name, x.data_ptr())
    h = _lib.bind_stream(dev.index, _device.current_stream_handle(dev))
    if sets is None:
        entry = _lib.lib().pcx_consensus_ragged_wide_f64 if wide else _lib.lib().pcx_consensus_ragged_f64
        _lib.check(entry(h, C.byref(inp), C.byref(res)))
    else:
        arr = _params_array(sets)
        _lib.check(_lib.lib().pcx_consensus_ragged_params_f64(h, C.byref(inp), len(sets), C.cast(arr, C.c_void_p),
                                                              param_of.ctypes.data, C.byref(res)))
        outs["_param_sets"], outs["_param_of"] = sets, param_of
    zero = np.zeros(1, dtype=np.int64)
    outs["_packed"] = buf
    outs["_layout"] = layout
    outs["_shapes"] = shapes
    outs["_reporter_offsets"] = np.concatenate([zero, np.cumsum(ns, dtype=np.int64)])
    outs["_event_offsets"] = np.concatenate([zero, np.cumsum(es, dtype=np.int64)])
    outs["_cell_offsets"] = np.concatenate([zero, np.cumsum(ns.astype(np.int64) * es, dtype=np.int64)])
    outs["_inputs"] = (R, rep_d, sc_d, lo_d, hi_d, aux_d)  # keep inputs alive until the caller syncs
    return outs


_RAGGED_KIND = {name: kind for name, kind, _ in _abi.BATCH_OUTPUTS}


def ragged_round(out, b):
    """Round ``b`` of a :func:`consensus_ragged` (or :func:`ragged_to_host`) result: every output as
    a view, ``original`` / ``filled`` reshaped to (N_b, E_b), the per-round scalars as 0-d views."""
    N, E = (int(x) for x in out["_shapes"][b])
    r0, e0, c0 = (int(out[k][b]) for k in ("_reporter_offsets", "_event_offsets", "_cell_offsets"))
    g = {}
    for name, v in out.items():
        if name.startswith("_"):
            continue
        kind = _RAGGED_KIND[name]
        if kind == "N":
            g[name] = v[r0:r0 + N]
        elif kind == "E":
            g[name] = v[e0:e0 + E]
        elif kind == "NE":
            g[name] = v[c0:c0 + N * E].reshape(N, E)
        else:
            g[name] = v[b]
    return g


def ragged_to_host(out):
    """A :func:`consensus_ragged` result as flat numpy arrays, from ONE device-to-host copy (which
    waits for the launch); the shapes and offsets are carried over for :func:`ragged_round`."""
    host = out["_packed"].cpu().numpy()
    g = {k: out[k] for k in ("_shapes", "_reporter_offsets", "_event_offsets", "_cell_offsets")}
    for name, o, nb, dt, shape in out["_layout"]:
        g[name] = host[o:o + nb].view(np.float64 if dt == "f8" else np.int32)
    return g
