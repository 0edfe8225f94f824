"""Many independent consensus problems of different shapes, in a few ragged launches.

``consensus_many(problems)`` returns what ``[Oracle(**p).consensus() for p in problems]`` returns,
but the problems of at most 64 reporters x 32 events run together on the one-wave round kernel
(:func:`pyconsensus_amd.batched.consensus_ragged`): one launch and one copy back per group of
problems that share the integer dtype, bounds given or not, and reputation given or not.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from .batched import (MAX_EVENTS, MAX_REPORTERS, WIDE_MAX_EVENTS, WIDE_MAX_REPORTERS, consensus_ragged,
                      kmeans_draws_ragged, ragged_round, ragged_to_host)
from .oracle import Oracle

_SHARED = ("catch_tolerance", "alpha", "algorithm", "variance_threshold", "hierarchy_threshold", "device")


def consensus_many(problems, wide=False, **oracle_kwargs):
    """Run every problem's ``Oracle(**problem, **oracle_kwargs).consensus()``.

    problems: a sequence of dicts of Oracle constructor arguments (``reports``, ``event_bounds``,
              ``reputation``, ``aux`` for cokurtosis, ...)
    Returns the list of result dicts, in order; each equals that problem's own
    ``Oracle(...).consensus()`` in values and container types (the dicts are built by the same code).
    A problem above 64 x 32 goes through ``Oracle`` itself, in list order.

    ``algorithm="k-means"``: the problems within the limits join the ragged groups like the others
    (``consensus_ragged(kmeans_init=...)``; ``last_info["path"] == "ragged"``).  The reference draws
    every restart's code book from numpy's global RandomState call by call, so the draws are made in
    list order, whichever path a problem takes: a k-means problem of a group draws its books
    (:func:`pyconsensus_amd.batched.kmeans_draws_ragged`) where its turn comes, and one too large for
    the batch runs through ``Oracle`` at its place in the list.  After ``np.random.seed(s)`` the call
    therefore returns what the ``Oracle`` loop returns after the same seed, and leaves
    ``np.random.get_state()`` where the loop leaves it.

    wide=True: problems up to 256 x 64 join the ragged groups as well (``consensus_ragged(wide=True)``,
    one workgroup per such problem; ``last_info["path"] == "ragged"``); larger problems still go
    through ``Oracle``.  What changes for a problem above 64 x 32: it runs in the batched
    SPEC's operation order -- what ``consensus_batched`` gives that shape -- where ``Oracle`` gives it
    the single-matrix pipeline's order.  Its discrete outputs are equal; its continuous ones agree
    within the parity tolerances of the test suite (tests/parity.py), not bit for bit -- which is why
    the keyword is opt-in."""
    max_n, max_e = (WIDE_MAX_REPORTERS, WIDE_MAX_EVENTS) if wide else (MAX_REPORTERS, MAX_EVENTS)
    oracles = [Oracle(**p, **oracle_kwargs) for p in problems]
    results = [None] * len(oracles)
    groups, alone, books = {}, [], {}
    for i, (p, o) in enumerate(zip(problems, oracles)):
        if o.algorithm not in _abi.ALGORITHMS:
            raise NotImplementedError("algorithm %r is not on the GPU path (supported: %s)"
                                      % (o.algorithm, ", ".join(sorted(_abi.ALGORITHMS))))
        if (o.num_reports > max_n or o.num_events > max_e
                or o.num_reports < 1 or o.num_events < 1 or o.devices is not None):
            if o.algorithm == "k-means":  # its draws come now, in list order
                results[i] = o.consensus()
            else:
                alone.append(i)
            continue
        if o.algorithm == "k-means":  # this problem's draws, in list order
            books[i] = kmeans_draws_ragged([o.num_reports])[0]
        # (the problems' own max_components: each Oracle holds it capped at its E already)
        mc = p.get("max_components", oracle_kwargs.get("max_components", 5))
        key = (o._int_dtype, o.event_bounds is not None, o._rep_raw is not None, mc) + tuple(
            getattr(o, k) for k in _SHARED)
        groups.setdefault(key, []).append(i)
    for key, idx in groups.items():
        first = oracles[idx[0]]
        kw = {}
        if first.event_bounds is not None:
            bounds = [oracles[i]._bounds_arrays() for i in idx]
            kw.update(scaled=[b[0] for b in bounds], lo=[b[1] for b in bounds], hi=[b[2] for b in bounds])
        if first._rep_raw is not None:
            kw["reputation"] = [oracles[i]._rep_raw for i in idx]
        if first.algorithm == "cokurtosis":
            aux = [np.asarray(oracles[i].aux["cokurt"], dtype=np.float64).ravel() for i in idx]  # :456
            if any(a.size != oracles[i].num_reports for a, i in zip(aux, idx)):
                raise ValueError("aux['cokurt'] must hold one score per reporter")
            kw["aux_scores"] = aux
        if first.algorithm == "k-means":
            kw["kmeans_init"] = [books[i] for i in idx]
        out = consensus_ragged([oracles[i]._data for i in idx], filled=True, original=True,
                               int_dtype=first._int_dtype, algorithm=first.algorithm,
                               catch_tolerance=first.catch_tolerance, alpha=first.alpha, max_components=key[3],
                               variance_threshold=first.variance_threshold,
                               hierarchy_threshold=first.hierarchy_threshold, device=first.device, wide=wide, **kw)
        host = ragged_to_host(out)  # the group's one copy back
        for b, i in enumerate(idx):
            g = ragged_round(host, b)
            o = oracles[i]
            o.last_info = {"branch": int(g["branch"]), "flags": int(g["flags"]), "pi_iters": int(g["pi_iters"]),
                           "path": "ragged"}
            results[i] = o._finish(g, float(g["participation"]), float(g["avg_certainty"]), int(g["components"]))
    for i in alone:
        results[i] = oracles[i].consensus()
    return results
