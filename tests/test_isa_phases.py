"""tools/isa_phases.py (static per-phase instruction counts of the batched kernel) runs on the CPU:
it compiles pcx_batched.hip to assembly, splits the 50 x 20 packed instantiation at the phase-stamp
markers and prints the kernel metadata.  Skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# the kernel's clock reads in source order: 17 STAMP() phase boundaries, and the three reads of the
# median profile (wave_wmedian_rank: start, after the ranks, after the walk) in each of its two
# inlined copies (interpolation and outcome medians)
MARKERS = 17 + 2 * 3


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not installed")
def test_isa_phases_runs_on_c3_kernel():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_phases.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert "batched_round_kernelILi50ELi20ELb0ELb1E" in out.splitlines()[0]
    assert int(re.search(r"^segments (\d+)", out, re.M).group(1)) == MARKERS + 1
    rows = [ln for ln in out.splitlines() if re.match(r"\s*\d+\s+\d+", ln)]
    assert len(rows) == MARKERS + 1
    # the metadata of the 50 x 20 packed kernel: four waves per SIMD
    meta = out[out.index("metadata"):]
    c3 = meta[meta.index("batched_round_kernelILi50ELi20ELb0ELb1E"):].splitlines()[1]
    assert int(re.search(r"vgpr_count=(\d+)", c3).group(1)) <= 128, c3
    assert meta.count("_ZN3pcx20batched_round_kernel") == 5  # every instantiation's metadata
