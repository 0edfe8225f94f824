"""Diagnostic: per-phase shader-clock breakdown of batched_round_kernel on the C3 workload
(PCX_STAMPS=1 makes the library stamp s_memtime at phase boundaries; printed to stderr).

    python tools/stamps_batched.py [B]

The launches run in a child process whose stderr is passed through; the last launch's line is then
parsed and printed as one JSON line: the cycles per phase (named by the closing stamp), their sum, and
the per-round counters (outcome_shortcut / outcome_sorted, interp_screened / interp_sorted,
guess_replayed: binary guesses taken from the exact replay, replay_rounds: rounds that ran it)."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(line):
    """{"phases": {stamp: cycles}, "sum": cycles, "counters": {name: per-round mean}} of a PCX_STAMPS line."""
    body = line.split("phase:", 1)[1]
    phases = {int(k): float(v) for k, v in re.findall(r"\s(\d+):(\d+)", body)}
    counters = {k: float(v) for k, v in re.findall(r"\s([a-z_]+):([0-9.]+)", body)}
    return {"phases": phases, "sum": sum(phases.values()), "counters": counters}


def child(B):
    sys.path.insert(0, ROOT)
    import torch

    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched

    R, sc, lo, hi, rep = synthetic.rounds(B, 50, 20, seed=20261015)
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).cuda()
    args = (t(R), t(rep), t(sc, torch.uint8), t(lo), t(hi))
    for _ in range(2):
        consensus_batched(*args)
        torch.cuda.synchronize()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B)],
                       env=dict(os.environ, PCX_STAMPS="1"), stderr=subprocess.PIPE, text=True)
    sys.stderr.write(r.stderr)
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("PCX_STAMPS mean cycles per phase:")]
    if r.returncode or not lines:
        sys.exit(r.returncode or 1)
    print(json.dumps(parse(lines[-1])))


if __name__ == "__main__":
    main()
