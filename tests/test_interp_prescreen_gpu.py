"""The batched kernel's interpolation medians decided by the prescreen (csrc/pcx_batched.hip,
wave_wmedian_screen), bit for bit against the C oracle (oracle/pcx_oracle_batched.c) on every output,
`branch`, `flags` and `pi_iters` included: the batches of interp_prescreen_cases.py (32 rounds each) at
50 x 20 (compiled kernel), 50 x 21 (dynamic kernel), 2 x 3, 3 x 4, 9 x 5 and 64 x 32, one ragged launch
mixing 50 x 20, 3 x 4 and 64 x 32 rounds of five kinds, and the kernel's own count of the medians the
prescreen decided (PCX_STAMPS=1, in a child process) between the bounds the CPU restatement gives."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import interp_prescreen_cases as IC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUST = ("branch", "flags", "pi_iters", "scores", "adj_first_loadings", "smooth_rep", "this_rep", "outcomes_raw",
        "outcomes_final", "certainty", "consensus_reward", "reporter_bonus", "author_bonus", "participation",
        "avg_certainty", "original", "filled")
CASES = [(kind, N, E) for N, E in IC.SHAPES for kind in IC.KINDS]
RAGGED_SHAPES = [(50, 20), (3, 4), (64, 32)]
RAGGED_KINDS = ("plain", "collision", "near_half", "zero_weight", "signed")
COUNTED = ("plain", "ties", "collision", "near_half", "uniform", "zero_weight", "signed", "exact_half", "equal")


def _assert_bitexact(g, c, what):
    assert set(MUST) <= set(g) <= set(c), (what, set(MUST) - set(g), set(g) - set(c))
    for k, v in g.items():
        same = (v == c[k]) | (np.isnan(v) & np.isnan(c[k])) if v.dtype.kind == "f" else (v == c[k])
        assert np.all(same), (what, k, int(np.size(same) - np.count_nonzero(same)))


@pytest.mark.parametrize("case", CASES, ids=["%s_%dx%d" % c for c in CASES])
def test_kinds_bitexact_vs_c_oracle(gpu_lib, case):
    from pyconsensus_amd.batched import consensus_batched

    kind, N, E = case
    R, kw, c = IC.batch(kind, N, E)
    g = consensus_batched(R, filled=True, original=True, **kw)
    _assert_bitexact({k: v.cpu().numpy() for k, v in g.items() if not k.startswith("_")}, c, case)


def test_ragged_launch_bitexact_vs_c_oracle(gpu_lib):
    """Rounds of three shapes and five kinds interleaved in one launch: each round's outputs are the
    oracle's of its own batch."""
    from pyconsensus_amd.batched import consensus_ragged, ragged_round, ragged_to_host

    order = [(kind, shape, b) for b in range(0, IC.B, 4) for kind in RAGGED_KINDS for shape in RAGGED_SHAPES]
    rounds = [IC.batch(kind, *shape) for kind, shape, _ in order]
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
import interp_prescreen_cases as IC
from pyconsensus_amd.batched import consensus_batched
for kind in %r:
    R, kw = IC.build(kind, 50, 20)
    sys.stderr.write("BATCH %%s\n" %% kind)
    sys.stderr.flush()
    consensus_batched(R, **kw)
    torch.cuda.synchronize()
"""


def test_prescreen_counters(gpu_lib):
    """The kernel's counters (stamps 24 and 25: interpolation medians decided by the prescreen / sorted),
    from a fresh child process with PCX_STAMPS=1: per batch their sum is the number of scaled columns
    with a missing report, and the screened count lies between the medians the CPU restatement decides
    at twice the margin and those it decides at half of it -- so the prescreen ran, and where it must
    not decide it did not."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), COUNTED)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PCX_STAMPS="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, kind = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("BATCH "):
            kind = line.split()[1]
        m = re.search(r"interp_screened:([0-9.]+) interp_sorted:([0-9.]+)", line)
        if m and kind:
            seen[kind] = (round(float(m.group(1)) * IC.B), round(float(m.group(2)) * IC.B))
    assert set(seen) == set(COUNTED), r.stderr[-2000:]
    for kind in COUNTED:
        lower, upper, total = IC.counter_bounds(kind)
        fast, slow = seen[kind]
        print(kind, "screened", fast, "sorted", slow, "bounds", lower, upper, "of", total)
        assert fast + slow == total, (kind, fast, slow, total)
        assert lower <= fast <= upper, (kind, lower, fast, upper)
    assert seen["plain"][0] > 0
    assert seen["collision"][0] == 0 and seen["collision"][1] == IC.B
    assert seen["near_half"][0] == 0 and seen["near_half"][1] == IC.B
    assert seen["uniform"][0] == 0  # no reputations: the kernel does not prescreen
