"""The batched kernel's guess sums (csrc/pcx_batched_round.inc, phase a3: row-split fast sums, the exact
replay), bit for bit against the C oracle (oracle/pcx_oracle_batched.c) on every output, `branch`, `flags`
and `pi_iters` included: the batches of guess_sums_cases.py (32 rounds each) at 50 x 20 (compiled
kernel), 50 x 21 and 64 x 21 (dynamic kernel, three groups), 50 x 22 and 64 x 32 (no split), 1 x 1, 2 x 3,
3 x 4 (groups with no row) and 9 x 5, one ragged launch mixing 50 x 20, 3 x 4 and 64 x 32 rounds of five
kinds, and the kernel's own count of the binary columns it replayed (PCX_STAMPS=1, in a child process)
between the bounds the CPU restatement gives."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import guess_sums_cases as GC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUST = ("branch", "flags", "pi_iters", "scores", "adj_first_loadings", "smooth_rep", "this_rep", "outcomes_raw",
        "outcomes_final", "certainty", "consensus_reward", "reporter_bonus", "author_bonus", "participation",
        "avg_certainty", "original", "filled")
CASES = [(kind, N, E) for N, E in GC.SHAPES for kind in GC.KINDS]
RAGGED_SHAPES = [(50, 20), (3, 4), (64, 32)]
RAGGED_KINDS = ("plain", "threshold", "wide", "half_ties", "signed")
COUNTED = ("plain", "threshold", "uniform")


def _assert_bitexact(g, c, what):
    assert set(MUST) <= set(g) <= set(c), (what, set(MUST) - set(g), set(g) - set(c))
    for k, v in g.items():
        same = (v == c[k]) | (np.isnan(v) & np.isnan(c[k])) if v.dtype.kind == "f" else (v == c[k])
        assert np.all(same), (what, k, int(np.size(same) - np.count_nonzero(same)))


@pytest.mark.parametrize("case", CASES, ids=["%s_%dx%d" % c for c in CASES])
def test_kinds_bitexact_vs_c_oracle(gpu_lib, case):
    from pyconsensus_amd.batched import consensus_batched

    kind, N, E = case
    R, kw, c = GC.batch(kind, N, E)
    g = consensus_batched(R, filled=True, original=True, **kw)
    _assert_bitexact({k: v.cpu().numpy() for k, v in g.items() if not k.startswith("_")}, c, case)


def test_ragged_launch_bitexact_vs_c_oracle(gpu_lib):
    """Rounds of three shapes and five kinds interleaved in one launch: each round's outputs are the
    oracle's of its own batch."""
    from pyconsensus_amd.batched import consensus_ragged, ragged_round, ragged_to_host

    order = [(kind, shape, b) for b in range(0, GC.B, 4) for kind in RAGGED_KINDS for shape in RAGGED_SHAPES]
    rounds = [GC.batch(kind, *shape) for kind, shape, _ in order]
    pick = lambda key: [kw[key][b] for (_, kw, _), (_, _, b) in zip(rounds, order)]
    out = consensus_ragged([R[b] for (R, _, _), (_, _, b) in zip(rounds, order)], pick("reputation"), pick("scaled"),
                           pick("lo"), pick("hi"), filled=True, original=True)
    host = ragged_to_host(out)
    names = [k for k in host if not k.startswith("_")]
    assert {"original", "filled", "smooth_rep", "outcomes_raw", "outcomes_final", "branch"} <= set(names)
    for i, ((_, _, c), (kind, shape, b)) in enumerate(zip(rounds, order)):
        g = ragged_round(host, i)
        for name in names:
            a, r = np.asarray(g[name]), np.asarray(c[name][b])
            assert a.shape == r.shape and a.dtype == r.dtype, (kind, shape, b, name)
            same = (a == r) | (np.isnan(a) & np.isnan(r)) if a.dtype.kind == "f" else (a == r)
            assert np.all(same), (kind, shape, b, name)


CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import guess_sums_cases as GC
from pyconsensus_amd.batched import consensus_batched
for kind in %r:
    R, kw = GC.build(kind, 50, 20)
    sys.stderr.write("BATCH %%s\n" %% kind)
    sys.stderr.flush()
    consensus_batched(R, **kw)
    torch.cuda.synchronize()
"""


def test_replay_counters(gpu_lib):
    """The kernel's counters (stamp 26: binary columns whose guess came from the exact replay; 27: the
    round ran the replay), from a fresh child process with PCX_STAMPS=1: per batch the replayed count
    lies between the columns the CPU restatement refuses at half the margin and those it refuses at
    twice the margin.  A build that always replays fails on plain (none refused), one that never
    replays on threshold (column 0 of every round refused)."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), COUNTED)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PCX_STAMPS="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, kind = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("BATCH "):
            kind = line.split()[1]
        m = re.search(r"interp_sorted:([0-9.]+) guess_replayed:([0-9.]+) replay_rounds:([0-9.]+)", line)
        if m and kind:
            seen[kind] = tuple(round(float(v) * GC.B) for v in m.groups())
    assert set(seen) == set(COUNTED), r.stderr[-2000:]
    for kind in COUNTED:
        lower, upper, total = GC.replay_bounds(kind)
        sorted_, replayed, rounds = seen[kind]
        print(kind, "replayed", replayed, "bounds", lower, upper, "of", total, "replay rounds", rounds, "sorted", sorted_)
        assert lower <= replayed <= upper, (kind, lower, replayed, upper)
        assert rounds <= GC.B and (rounds > 0) == (replayed + sorted_ > 0)
    assert GC.replay_bounds("plain")[1] == 0 and seen["plain"][1] == 0
    assert seen["threshold"][1] >= GC.B and seen["threshold"][2] == GC.B
    # equal reputations are not prescreened: every round with an interpolation median replays the totals
    R, kw = GC.build("uniform", 50, 20)
    med = np.asarray(kw["scaled"]).astype(bool) & np.isnan(R).any(axis=1)
    assert seen["uniform"][2] >= np.count_nonzero(med.any(axis=1))
