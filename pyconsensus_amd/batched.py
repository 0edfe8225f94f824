"""Batched Monte Carlo regime: B independent oracle rounds in one launch.

Each round is exactly ``Oracle(reports[b], event_bounds_b, reputation[b]).consensus()``
(pyconsensus/__init__.py:102-611).  This is the regime of Simulator.jl-style Monte
Carlo drivers (README.rst:52-56), which loop consensus() over many random rounds.
Rounds of at most 64 reporters x 32 events run in one wavefront each of
``batched_round_kernel`` (csrc/pcx_batched.hip); rounds up to 256 x 64 in one workgroup each of
``medium_round_kernel`` (csrc/pcx_medium.hip), every algorithm (k-means with up to 16 codes);
larger rounds run as single-matrix consensuses, many in flight on a pool of worker streams
(csrc/pcx_rounds.cpp).  :func:`route` tells which of the three a shape takes.
With ``tall=True`` rounds of 257 to 1024 reporters and at most 64 events run in one workgroup each of
``tall_round_kernel`` (csrc/pcx_tall.hip) instead: one asynchronous launch, the SPEC's bits.
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
TALL_MAX_REPORTERS = 1024  # one workgroup per round up to here with tall=True (and WIDE_MAX_EVENTS)


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


def kmeans_draws_ragged(n_reporters, restarts=_abi.KMEANS_RESTARTS, random_state=None, k=None):
    """Initial code-book rows of k-means rounds of DIFFERENT sizes: a list of (restarts, k_b) int32
    arrays, round b's drawn as ``rs.choice(N_b, size=k_b, replace=False)`` restart after restart,
    round after round -- the RandomState (numpy's global one by default) is consumed exactly as
    :func:`kmeans_draws` called round by round consumes it, and as sequential reference consensus()
    calls would.  ``k``: the code-book sizes (default :func:`kmeans_k` of each N_b)."""
    rs = np.random.mtrand._rand if random_state is None else random_state
    out = []
    for b, N in enumerate(n_reporters):
        kb = kmeans_k(N) if k is None else int(k[b])
        book = np.empty((restarts, kb), dtype=np.int32)
        for r in range(restarts):
            book[r] = rs.choice(int(N), size=kb, replace=False)
        out.append(book)
    return out


def kmeans_plan(shapes, restarts=_abi.KMEANS_RESTARTS, k=None):
    """The int64 [B + 1] offsets of the flat code-book array of k-means rounds of ``shapes``
    [(N_b, E_b), ...] (pcx_kmeans_plan): round b's ``restarts x k_b`` rows start at offsets[b].
    ``k``: the code-book sizes (default: the ceil(sqrt(N_b)) rule).  Needs no GPU; raises PcxError
    naming the first round whose shape or code-book size is refused."""
    sh = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    kk = None if k is None else np.ascontiguousarray(k, dtype=np.int32)
    if kk is not None and kk.shape != (len(sh),):
        raise ValueError("k must hold one code-book size per round (%d)" % len(sh))
    offsets, bad = np.zeros(len(sh) + 1, dtype=np.int64), C.c_int64(-1)
    _lib.check(_lib.lib().pcx_kmeans_plan(len(sh), n.ctypes.data, e.ctypes.data, None if kk is None else kk.ctypes.data,
                                          int(restarts), offsets.ctypes.data, C.byref(bad)))
    return offsets


ROUTES = ("wave", "workgroup", "scheduler", "tall")  # include/pcx.h enum pcx_route


def route(N, E, algorithm="PCA", kmeans_k=None, tall=False):
    """Where ``consensus_batched`` runs rounds of N x E: ``"wave"`` (one wavefront per round, up to
    64 x 32) and ``"workgroup"`` (one workgroup per round, up to 256 x 64; k-means with at most 16
    codes) are ONE asynchronous kernel launch; ``"scheduler"`` is the host-driven round scheduler,
    which returns once every output is written.  ``kmeans_k`` defaults to :func:`kmeans_k` (N).
    ``tall=True``: where ``consensus_batched(..., tall=True)`` runs them (pcx_tall_route) -- ``"tall"``
    (one workgroup per round of ``tall_round_kernel``, ONE asynchronous launch) for 256 < N <= 1024,
    E <= 64 and "PCA", "absolute", "big-five", "fixed-variance" or "cokurtosis" where the round's LDS
    plan fits a workgroup (:func:`tall_plan`); every other shape and algorithm as without it.
    Needs no GPU; raises ValueError for arguments ``consensus_batched`` refuses."""
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    k = kmeans_k_default(N) if kmeans_k is None else int(kmeans_k)
    query = _lib.lib().pcx_tall_route if tall else _lib.lib().pcx_batched_route
    r = query(int(N), int(E), alg, k)
    if r < 0:
        raise ValueError("no batched route for %d x %d rounds, algorithm %r, kmeans_k %d" % (N, E, algorithm, k))
    return ROUTES[r]


def tall_plan(N, E, algorithm="PCA"):
    """The LDS plan of one tall N x E round (pcx_tall_plan, pcx_tall_lds_bytes), or None where
    ``route(..., tall=True)`` is not ``"tall"``: a dict of ``waves`` (weighted medians and certainties
    that run side by side: 4, 2 or 1), ``dot_rows`` (reporter rows per chunk of np.dot's block
    partials), ``dot_chunks``, ``threads`` and ``lds_bytes`` (the launch's dynamic LDS).  Needs no GPU."""
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    out = (C.c_int32 * 4)()
    if _lib.lib().pcx_tall_plan(int(N), int(E), alg, out) != 0:
        return None
    return dict(waves=int(out[0]), dot_rows=int(out[1]), dot_chunks=int(out[2]), threads=int(out[3]),
                lds_bytes=int(_lib.lib().pcx_tall_lds_bytes(int(N), int(E), alg)))


def clusterfeck_threshold(E):
    """The reference's default leader-clustering cut (__init__.py:187-190, 210-213)."""
    t = np.log10(E) / 1.77
    return 0.3 if t == 0 else float(t)


def consensus_batched(reports, reputation=None, scaled=None, lo=None, hi=None,
                      catch_tolerance=0.1, alpha=0.1, int_dtype=False, algorithm="PCA",
                      outputs=None, device=None, filled=False, original=False,
                      max_components=5, variance_threshold=0.9, aux_scores=None,
                      hierarchy_threshold=0.5, kmeans_init=None, cluster_threshold=None, packed=False,
                      tall=False):
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
    tall:       True: rounds of 257 to 1024 reporters and at most 64 events run one workgroup each
                on ``tall_round_kernel`` (pcx_consensus_batched_tall_f64) where
                ``route(N, E, algorithm, tall=True)`` says ``"tall"``: ONE asynchronous launch, every
                output bit-identical to the C SPEC built for 1024 reporters.  Every other shape and
                algorithm runs exactly as without it.  Opt-in, because above 256 reporters the round
                scheduler gives the single-matrix path's arithmetic and the tall route the SPEC's:
                the two agree within tolerance, not bit for bit

    Returns a dict of torch tensors on the device, named like the ABI fields
    (``smooth_rep``, ``outcomes_final``, ...).  Three regimes (:func:`route`):
    rounds up to 64 x 32 (one wave per round) and up to 256 x 64 (one workgroup per round; every
    algorithm, the clusterings included, k-means with code books of at most 16 rows -- the
    reference's own ceil(sqrt(N)) up to there; kmeans_init is read on the device) are ONE kernel
    launch, asynchronous on torch's current stream -- synchronise before reading the outputs on
    the host; the round scheduler (rounds above 256 x 64, k-means with larger code books) returns
    only once every output is written.  ``tall=True`` moves rounds up to 1024 x 64 from the scheduler
    to a fourth regime of that kind: one launch, asynchronous.
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
    entry = _lib.lib().pcx_consensus_batched_tall_f64 if tall else _lib.lib().pcx_consensus_batched_f64
    _lib.check(entry(h, C.byref(inp), C.byref(res)))
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
    tdt = {np.float64: t.float64, np.uint8: t.uint8, np.int32: t.int32}
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


def ragged_plan(shapes, algorithm="PCA", wide=False, kmeans_restarts=None, kmeans_k=None):
    """(totals, lds_bytes) of a ragged batch of ``shapes`` [(N_b, E_b), ...]: totals = (sum N_b,
    sum E_b, sum N_b * E_b), the flat arrays' lengths, and the launch's dynamic LDS.  Needs no GPU;
    raises PcxError naming the first round the one-wave kernel does not take (or k-means).

    ``wide=True``: rounds up to 256 x 64 (pcx_ragged_plan_wide); returns (totals, counts, lds_bytes)
    with 4-tuples counts / lds_bytes: index 0 the rounds of at most 64 x 32 (the one-wave kernel's
    launch), index c = 1..3 the workgroup kernel's rounds of launch class c -- c rounds per CU by
    their LDS -- and that launch's dynamic LDS.

    ``kmeans_restarts`` (an int) opts in to k-means (pcx_ragged_plan_kmeans): returns (totals,
    n_launches, book_offsets) as :func:`ragged_plan_kmeans` for the one shared set; ``kmeans_k``
    the code-book sizes (default: the rule).  Without it k-means is refused as before."""
    alg = _abi.ALGORITHMS.get(algorithm)
    if alg is None:
        raise NotImplementedError("algorithm %r is not on the GPU path" % (algorithm,))
    sh = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    if kmeans_restarts is not None:
        if not wide:
            ragged_plan(sh, "PCA", wide=False)  # the one-wave limits, by index
        defaults = dict(algorithm=algorithm, catch_tolerance=0.1, alpha=0.1, max_components=5, variance_threshold=0.9,
                        hierarchy_threshold=0.5, cluster_threshold=None)
        return ragged_plan_kmeans(sh, [defaults], np.zeros(len(sh), dtype=np.int32), kmeans_restarts, kmeans_k)
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


def ragged_plan_tall(shapes, sets, param_of):
    """:func:`ragged_plan_params` with rounds up to 1024 x 64 (pcx_ragged_plan_tall): (totals,
    n_launches, n_tall, tall_lds_bytes).  A round above 256 reporters must be of the tall route under
    its set's algorithm (:func:`route` with ``tall=True``, :func:`tall_plan`); such rounds form one
    more launch segment, whose dynamic LDS is the largest round's plan.  Needs no GPU; raises PcxError
    naming the first offending round or parameter set."""
    sh = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    of = np.ascontiguousarray(param_of, dtype=np.int32)
    arr = _params_array(sets)
    totals, nl, bad_r, bad_p = (C.c_int64 * 3)(), C.c_int64(0), C.c_int64(-1), C.c_int64(-1)
    nt, lds = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().pcx_ragged_plan_tall(len(sh), n.ctypes.data, e.ctypes.data, len(sets),
                                               C.cast(arr, C.c_void_p), of.ctypes.data, totals, C.byref(nl),
                                               C.byref(bad_r), C.byref(bad_p), C.byref(nt), C.byref(lds)))
    return tuple(int(x) for x in totals), int(nl.value), int(nt.value), int(lds.value)


def ragged_plan_kmeans(shapes, sets, param_of, restarts, k=None):
    """:func:`ragged_plan_params` with k-means allowed in a set (pcx_ragged_plan_kmeans): (totals,
    n_launches, book_offsets).  book_offsets is int64 [B + 1] and counts only the k-means rounds'
    ``restarts x k_b`` code-book rows (``k``: their sizes, one per round, default the
    ceil(sqrt(N_b)) rule; an entry of a round that is not k-means is not read)."""
    sh = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 2))
    n, e = np.ascontiguousarray(sh[:, 0]), np.ascontiguousarray(sh[:, 1])
    of = np.ascontiguousarray(param_of, dtype=np.int32)
    kk = None if k is None else np.ascontiguousarray(k, dtype=np.int32)
    if kk is not None and kk.shape != (len(sh),):
        raise ValueError("kmeans_k must hold one code-book size per round (%d)" % len(sh))
    arr = _params_array(sets)
    books = _abi.KmeansBooks(int(restarts), None if kk is None else kk.ctypes.data, None)
    totals, nl, bad_r, bad_p = (C.c_int64 * 3)(), C.c_int64(0), C.c_int64(-1), C.c_int64(-1)
    offsets = np.zeros(len(sh) + 1, dtype=np.int64)
    _lib.check(_lib.lib().pcx_ragged_plan_kmeans(len(sh), n.ctypes.data, e.ctypes.data, len(sets),
                                                 C.cast(arr, C.c_void_p), of.ctypes.data, C.byref(books), totals,
                                                 C.byref(nl), offsets.ctypes.data, C.byref(bad_r), C.byref(bad_p)))
    return tuple(int(x) for x in totals), int(nl.value), offsets


def _kmeans_books(kmeans_init, kmeans_restarts, kmeans_k, ns, is_km, plan):
    """consensus_ragged's ``kmeans_init`` -> (restarts, int32 k[B] or None, the books: a flat host
    int32 array, or the caller's device tensor).  ``plan(restarts, k)`` raises what the call refuses."""
    B = len(ns)
    if kmeans_k is not None:
        kmeans_k = np.asarray(kmeans_k, dtype=np.int32)
        if kmeans_k.shape != (B,):
            raise ValueError("kmeans_k must hold one code-book size per round (%d)" % B)
    if isinstance(kmeans_init, str):
        if kmeans_init != "draw":
            raise ValueError("kmeans_init must be None, \"draw\", a list of per-round arrays or a device tensor")
        restarts = _abi.KMEANS_RESTARTS if kmeans_restarts is None else int(kmeans_restarts)
        if restarts < 1:
            raise ValueError("kmeans_restarts must be >= 1")
        km = [b for b in range(B) if is_km[b]]
        plan(restarts, kmeans_k)  # (what the plan refuses is refused before a draw is made)
        drawn = kmeans_draws_ragged([ns[b] for b in km], restarts, k=None if kmeans_k is None else kmeans_k[km])
        flat = np.concatenate([d.reshape(-1) for d in drawn]) if drawn else np.zeros(0, dtype=np.int32)
        return restarts, kmeans_k, flat
    if isinstance(kmeans_init, (list, tuple)):
        if len(kmeans_init) != B:
            raise ValueError("kmeans_init must hold one entry per round (%d), got %d" % (B, len(kmeans_init)))
        restarts = None if kmeans_restarts is None else int(kmeans_restarts)
        ks, parts = np.zeros(B, dtype=np.int32), []
        for b in range(B):
            if not is_km[b]:
                continue
            if kmeans_init[b] is None:
                raise ValueError("kmeans_init[%d] is None, and round %d is k-means" % (b, b))
            a = np.asarray(kmeans_init[b])
            if a.ndim != 2 or a.dtype.kind not in "iu":
                raise ValueError("kmeans_init[%d] must be an integer (restarts, k) array, got shape %s" % (b, a.shape))
            restarts = a.shape[0] if restarts is None else restarts
            if a.shape[0] != restarts:
                raise ValueError("kmeans_init[%d] has %d restarts, the call %d" % (b, a.shape[0], restarts))
            if kmeans_k is not None and a.shape[1] != kmeans_k[b]:
                raise ValueError("kmeans_init[%d] has %d rows a book, kmeans_k[%d] = %d" % (b, a.shape[1], b, kmeans_k[b]))
            if a.size and (int(a.min()) < 0 or int(a.max()) >= ns[b]):
                raise ValueError("kmeans_init[%d] rows must lie in [0, %d)" % (b, ns[b]))
            ks[b] = a.shape[1]
            parts.append(a.astype(np.int32).reshape(-1))
        if restarts is None:  # no k-means round: nothing is read
            restarts = _abi.KMEANS_RESTARTS
        flat = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
        return restarts, ks, flat
    t = _device.torch()
    if not isinstance(kmeans_init, t.Tensor):
        raise ValueError("kmeans_init must be None, \"draw\", a list of per-round arrays or a device tensor")
    if kmeans_restarts is None:
        raise ValueError("a device tensor of code books needs kmeans_restarts")
    if kmeans_init.dtype != t.int32 or kmeans_init.dim() != 1 or not kmeans_init.is_contiguous() or not kmeans_init.is_cuda:
        raise ValueError("a kmeans_init tensor must be a flat contiguous int32 device tensor")
    return int(kmeans_restarts), kmeans_k, kmeans_init


def consensus_ragged(reports, reputation=None, scaled=None, lo=None, hi=None, *, catch_tolerance=0.1, alpha=0.1,
                     int_dtype=False, algorithm="PCA", outputs=None, device=None, filled=False, original=False,
                     max_components=5, variance_threshold=0.9, aux_scores=None, hierarchy_threshold=0.5,
                     cluster_threshold=None, wide=False, per_round=None, kmeans_init=None, kmeans_restarts=None,
                     kmeans_k=None, tall=False):
    """Run B rounds of DIFFERENT shapes in one launch of the one-wave round kernel.

    reports:    a sequence of B arrays, round b an (N_b, E_b) matrix with N_b <= 64, E_b <= 32
    wide:       True: rounds up to 256 x 64 (pcx_consensus_ragged_wide_f64).  Those above 64 x 32
                run one workgroup each on the ragged form of ``medium_round_kernel``, one launch per
                launch class (:func:`ragged_plan`); the others on the one-wave kernel as before.
                Every round equals its own ``consensus_batched`` run.  Calls share one per-context
                scratch: keep them on one stream
    tall:       True: rounds up to 1024 x 64 (pcx_consensus_ragged_tall_f64), with or without
                ``per_round``.  A round above 256 reporters runs one workgroup of the tall kernel's
                per-round form, all of them in one more launch segment behind the others, and equals
                ``consensus_batched(..., tall=True)`` on that round alone; it must be of the tall
                route under its algorithm (:func:`route` with ``tall=True``, :func:`tall_plan`: no
                clustering, and big-five / fixed-variance only where the plan fits) or the call is
                refused by round.  The other rounds are those of the ``wide=True`` call.  Not with
                ``kmeans_init``
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
    algorithm:  as :func:`consensus_batched`; "k-means" needs ``kmeans_init`` (below) and is refused
                without it; "big-five" caps max_components at E_b per round, "clusterfeck" takes the
                reference's log10(E_b)/1.77 cut per round unless cluster_threshold is given
    kmeans_init: None (default): k-means is refused, as before.  Otherwise the call takes k-means,
                shared or in ``per_round`` sets (pcx_consensus_ragged_kmeans_f64), with the k-means
                rounds' initial code books from: ``"draw"`` -- :func:`kmeans_draws_ragged` on numpy's
                global RandomState, over the k-means rounds in round order; a list of B integer
                arrays (restarts, k_b), rows in [0, N_b) (None where the round is not k-means); or one
                flat int32 device tensor, the k-means rounds' books end to end ([restarts][k_b] each,
                laid out as ``out["_kmeans_offsets"]`` / :func:`ragged_plan_kmeans` tell), which is
                read in place and needs ``kmeans_restarts``.  Round b equals ``consensus_batched`` of
                its shape with ``kmeans_init`` = its book
    kmeans_restarts: restarts of every k-means round (default 20 for "draw"; a list's own)
    kmeans_k:   B code-book sizes (default: the reference's ceil(sqrt(N_b)), or a list's own): within
                [1, min(N_b, 8)] for a round up to 64 x 32, [1, min(N_b, 16)] above

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
    if tall and (kmeans_init is not None or kmeans_restarts is not None):
        raise ValueError("tall=True does not take k-means code books (kmeans_init / kmeans_restarts)")
    sets = param_of = None
    if per_round is not None or kmeans_init is not None or tall:  # (the k-means and tall entries take parameter sets)
        if per_round is not None and len(per_round) != B:
            raise ValueError("per_round must hold one entry per round (%d), got %d" % (B, len(per_round)))
        sets, param_of = param_sets([None] * B if per_round is None else per_round, dict(
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
    km_restarts = km_k = km_books = km_offsets = None
    if sets is None:
        totals = ragged_plan(shapes, algorithm, wide=wide)[0]  # refuses k-means and rounds past the limits, by index
    elif kmeans_init is not None:
        if not wide:
            ragged_plan(shapes, "PCA", wide=False)  # the one-wave limits, by index
        is_km = [sets[q]["algorithm"] == "k-means" for q in param_of]
        km_restarts, km_k, km_books = _kmeans_books(kmeans_init, kmeans_restarts, kmeans_k, ns, is_km,
                                                    lambda r, k: ragged_plan_kmeans(shapes, sets, param_of, r, k))
        totals, _, km_offsets = ragged_plan_kmeans(shapes, sets, param_of, km_restarts, km_k)
        if len(km_books) < int(km_offsets[-1]):
            raise ValueError("kmeans_init holds %d rows, the k-means rounds' code books %d"
                             % (len(km_books), int(km_offsets[-1])))
    elif tall:
        totals = ragged_plan_tall(shapes, sets, param_of)[0]  # refuses by round or by parameter set
    else:
        if not wide:
            ragged_plan(shapes, "PCA", wide=False)  # the one-wave limits, by index
        totals = ragged_plan_params(shapes, sets, param_of)[0]  # refuses by round or by parameter set
    t = _device.require_gpu()
    dev = t.device(device) if device is not None else t.device("cuda", t.cuda.current_device())
    flat = np.concatenate([m.reshape(-1) for m in mats]) if B else np.zeros(0)
    km_host = km_books if isinstance(km_books, np.ndarray) else None  # (the host books ride in the one copy)
    R, rep_d, sc_d, lo_d, hi_d, aux_d, km_d = _upload_packed(
        [(flat, np.float64), (rep, np.float64), (sc, np.uint8), (lo_, np.float64), (hi_, np.float64),
         (aux, np.float64), (km_host, np.int32)], dev)
    if km_books is not None and km_host is None:
        if km_books.device != dev:
            raise ValueError("the kmeans_init tensor is on %s, the call on %s" % (km_books.device, dev))
        km_d = km_books  # read in place
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
    elif kmeans_init is not None:
        arr = _params_array(sets)
        # (a zero-length tensor's pointer is NULL: a batch without k-means rounds reads no book)
        books = _abi.KmeansBooks(km_restarts, None if km_k is None else km_k.ctypes.data, _device.ptr(km_d))
        _lib.check(_lib.lib().pcx_consensus_ragged_kmeans_f64(h, C.byref(inp), len(sets), C.cast(arr, C.c_void_p),
                                                              param_of.ctypes.data, C.byref(books), C.byref(res)))
        outs["_param_sets"], outs["_param_of"] = sets, param_of
        outs["_kmeans_offsets"], outs["_kmeans_restarts"], outs["_kmeans_init"] = km_offsets, km_restarts, km_d
    else:
        arr = _params_array(sets)
        entry = _lib.lib().pcx_consensus_ragged_tall_f64 if tall else _lib.lib().pcx_consensus_ragged_params_f64
        _lib.check(entry(h, C.byref(inp), len(sets), C.cast(arr, C.c_void_p), param_of.ctypes.data, C.byref(res)))
        outs["_param_sets"], outs["_param_of"] = sets, param_of
    zero = np.zeros(1, dtype=np.int64)
    outs["_packed"] = buf
    outs["_layout"] = layout
    outs["_shapes"] = shapes
    outs["_reporter_offsets"] = np.concatenate([zero, np.cumsum(ns, dtype=np.int64)])
    outs["_event_offsets"] = np.concatenate([zero, np.cumsum(es, dtype=np.int64)])
    outs["_cell_offsets"] = np.concatenate([zero, np.cumsum(ns.astype(np.int64) * es, dtype=np.int64)])
    outs["_inputs"] = (R, rep_d, sc_d, lo_d, hi_d, aux_d, km_d)  # keep inputs alive until the caller syncs
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
