"""bench.py's launcher contract on the CPU: ``--gpus N`` without a launcher starts the
driver's own N-rank command as a child job; a WORLD_SIZE that disagrees with ``--gpus``
is refused before anything touches the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(args, env_extra, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_world_size_mismatch_refused():
    r = _run(["--gpus", "1"], {"WORLD_SIZE": "2"})
    assert r.returncode == 2
    assert "WORLD_SIZE=2 but --gpus 1" in r.stderr
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2"})
    assert r.returncode == 2


def test_gpus_zero_refused():
    assert _run(["--gpus", "0"], {}).returncode == 2


def test_self_launch_command(monkeypatch):
    import bench

    seen = {}

    class FakeProc:
        pid = 12345

        def __init__(self, cmd, env):
            seen["cmd"], seen["env"] = cmd, env

        def wait(self, timeout=None):
            return 7

        def send_signal(self, s):  # pragma: no cover
            pass

    import signal

    old = signal.getsignal(signal.SIGTERM)
    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "5"])
    try:
        assert bench.launch_ranks(4) == 7  # the child job's status is the parent's
    finally:
        signal.signal(signal.SIGTERM, old)
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "5"]
    assert cmd[-5].endswith("bench.py")
    assert bench.LAUNCHER_ENV in seen["env"]


def test_steps_zero_refused():
    assert _run(["--gpus", "1", "--steps", "0"], {}).returncode == 2


def test_dump_outputs_sample(tmp_path):
    """--dump-outputs: every output of the result dict as float64, the same seeded sample of rounds
    on every call, the kept-alive inputs left out, every file finite with the NaN / inf entries of
    the floating-point outputs coded beside them."""
    import numpy as np
    import torch

    import bench

    B = 5000
    smooth = torch.arange(B * 3, dtype=torch.float64).reshape(B, 3)
    idx0 = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(B, size=bench.DUMP_ROUNDS, replace=False))
    smooth[idx0[0], 1], smooth[idx0[1], 0], smooth[idx0[2], 2] = float("nan"), float("inf"), float("-inf")
    out = {"smooth_rep": smooth,
           "filled": torch.arange(B * 6, dtype=torch.float64).reshape(B, 3, 2),
           "branch": torch.arange(B, dtype=torch.int32), "_inputs": (None,)}
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d), B)
    got = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["branch.npy", "filled.npy", "filled_nonfinite.npy", "round_index.npy", "smooth_rep.npy",
                           "smooth_rep_nonfinite.npy"]
    idx = got["round_index.npy"].astype(np.int64)
    assert (idx == idx0).all() and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < B
    for name, a in got.items():
        assert a.dtype == (np.float32 if name.endswith("_nonfinite.npy") else np.float64)
        assert np.isfinite(a).all()
        assert (a == np.load(tmp_path / "b" / name)).all()
    assert (got["branch.npy"] == idx).all()
    code = got["smooth_rep_nonfinite.npy"]
    assert (code[0, 1], code[1, 0], code[2, 2]) == (1, 2, 3) and (code != 0).sum() == 3
    want = smooth.numpy()[idx]
    assert (got["smooth_rep.npy"][code == 0] == want[code == 0]).all() and (got["smooth_rep.npy"][code != 0] == 0).all()
    assert (got["filled.npy"] == out["filled"].numpy()[idx]).all() and not got["filled_nonfinite.npy"].any()
    # a batch smaller than the sample is written whole
    bench.dump_outputs({"branch": out["branch"][:10]}, str(tmp_path / "c"), 10)
    assert (np.load(tmp_path / "c" / "branch.npy") == np.arange(10)).all()
    # the sample of a default run stays under the 64 MB a dump may take
    floats, ints = 8 * bench.N_REP + 9 * bench.N_EV + 2 + 2 * bench.N_REP * bench.N_EV, 4
    assert bench.DUMP_ROUNDS * ((8 + 4) * floats + 8 * (ints + 1)) <= 64e6


@pytest.mark.gpu
def test_plain_run_and_dump(gpu_lib, tmp_path):
    """A plain run carries the headline alone, and --dump-outputs holds what consensus_batched
    returns for the same inputs, bit for bit, in finite numbers: NaN only where the code file beside
    the output says so."""
    import json

    import numpy as np
    import torch

    import bench
    from pyconsensus_amd import synthetic
    from pyconsensus_amd.batched import consensus_batched

    B = 3000
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--rounds", str(B), "--dump-outputs", str(tmp_path)], {})
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["dtype"] == "f64" and line["unit"] == "rounds/s" and line["higher_is_better"]
    assert abs(line["value"] - B * 2 / (2 * line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for k in ("cpu_baseline", "vectors_only_kernel_ms", "c5", "c4", "medium", "cov_fp64", "c1", "c2"):
        assert k not in line
    R, sc, lo, hi, rep = synthetic.rounds(B, bench.N_REP, bench.N_EV, seed=bench.SEED)
    g = consensus_batched(R, rep, sc.astype(np.uint8), lo, hi, device="cuda:0", filled=True, original=True)
    torch.cuda.synchronize()
    idx = np.load(tmp_path / "round_index.npy").astype(np.int64)
    assert idx.shape == (bench.DUMP_ROUNDS,)
    names = [k for k in g if not k.startswith("_")]
    codes = [n + "_nonfinite.npy" for n in names if g[n].dtype.is_floating_point]
    assert len(codes) == len(names) - 4
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([n + ".npy" for n in names] + codes + ["round_index.npy"])
    for n in names:
        a, b = np.load(tmp_path / (n + ".npy")), g[n].cpu().numpy()[idx].astype(np.float64)
        assert a.dtype == np.float64 and a.shape == b.shape and np.isfinite(a).all()
        if n + "_nonfinite.npy" in codes:
            code = np.load(tmp_path / (n + "_nonfinite.npy"))
            assert code.dtype == np.float32 and code.shape == b.shape
            assert ((code == 1) == np.isnan(b)).all() and ((code == 0) == np.isfinite(b)).all(), n
            assert (a[code != 0] == 0).all(), n
            b = np.where(code == 0, b, 0.0)
        assert (a == b).all(), n
    assert np.load(tmp_path / "original_nonfinite.npy").any()  # the missing reports are in the sample


@pytest.mark.timeout(300)
def test_self_launch_reaches_ranks():
    """The real child job: 2 ranks start and each fails on the GPU-less host (no CUDA device),
    so the parent returns non-zero -- it does not fall back to a 1-rank run."""
    import torch

    if torch.cuda.is_available():  # pragma: no cover - a GPU box runs the real thing
        pytest.skip("CPU-only check")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--c5-steps", "0", "--no-c4", "--no-cpu-baseline"],
             {"PCX_DIST_BACKEND": "gloo"}, timeout=280)
    assert r.returncode != 0
    assert '"n_gpus": 1' not in r.stdout
