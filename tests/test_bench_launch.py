"""bench.py launches itself for --gpus N > 1: the parent starts torch.distributed.run as a CHILD process
before touching any GPU, relays rank 0's JSON line and exits with the child's code.  Exercised here on the CPU box through
--dry (gloo, no GPU work): launcher, process group, the all-reduce of the packed normal equations."""
import json
import os
import subprocess
import sys

import pytest

from conftest import FIXTURES, ROOT


def _run(*extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--backend", "gloo", "--dry"] + list(extra),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    return p


def test_self_launch_two_ranks_gloo_dry():
    p = _run("--gpus", "2", "--samples", "1000", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout          # ONE JSON line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2 and d["dry"] is True
    assert d["samples_reduced"] == 2000.0     # the count travels inside the one all-reduce payload
    # round 4: the legs a multi-GPU run adds, through their CPU plumbing -- configs[2]'s R-factor all-gather + fold, configs[4]'s split
    # of the 256 chains, and rank 0 waiting for the other ranks' processes to be gone before it would start the library child
    assert d["legs"] == ["config4", "config3_sharded", "config5_sharded"]
    assert d["r_factor_gather_fold_rel_err"] <= 1e-12
    assert d["config5_chains_per_rank"] == [128, 128] and d["config5_chains_total"] == 256
    assert d["distinct_pids"] == 2 and d["other_ranks_exited"] is True


def test_self_launch_eight_ranks_gloo_dry():
    """The driver's largest run (`--gpus 8`) through its CPU plumbing: eight ranks, every leg of the one JSON line."""
    p = _run("--gpus", "8", "--samples", "500", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["n_ranks_seen"] == 8 and d["samples_reduced"] == 4000.0
    assert d["legs"] == ["config4", "config3_sharded", "config5_sharded"]
    assert d["r_factor_gather_fold_rel_err"] <= 1e-12
    assert d["config5_chains_per_rank"] == [32] * 8 and d["distinct_pids"] == 8 and d["other_ranks_exited"] is True


def test_plain_run_has_no_side_legs_dry():
    """Without --full a run is the headline alone: the same launcher and ranks, no leg beside it."""
    p = _run("--gpus", "2", "--samples", "1000", "--steps", "7")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2 and d["samples_reduced"] == 2000.0
    assert d["legs"] == [] and d["steps"] == 7


def test_dump_indices_fixed_and_layouts_agree(tmp_path):
    """--dump-outputs: the same seeded sample subset every run, and one (k, n, P) / (k, n) form whatever the Y layout."""
    import numpy as np
    import torch
    import bench
    N, n, P = 50000, 3, 5
    idx = bench.dump_indices(N)
    assert len(idx) == bench.DUMP_SAMPLES and np.array_equal(idx, bench.dump_indices(N))
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < N
    assert np.array_equal(bench.dump_indices(100), np.arange(100))
    rng = np.random.default_rng(7)
    Ys, taus = rng.standard_normal((N, n, P)), rng.standard_normal((N, n))   # Ys[s] = the n x P regressor of sample s
    forms = {"stacked": (torch.from_numpy(np.ascontiguousarray(Ys.transpose(2, 0, 1).reshape(P, N * n))), torch.from_numpy(taus)),
             "per_sample": (torch.from_numpy(np.ascontiguousarray(Ys.transpose(0, 2, 1))), torch.from_numpy(taus)),
             "element": (torch.from_numpy(np.ascontiguousarray(Ys.transpose(2, 1, 0))), torch.from_numpy(np.ascontiguousarray(taus.T)))}
    for lay, (Y, tau) in forms.items():
        out = tmp_path / lay
        bench.dump_outputs(str(out), Y, tau, lay, N, n, P)
        assert sorted(os.listdir(out)) == ["Y.npy", "tau.npy"]
        y, t = np.load(out / "Y.npy"), np.load(out / "tau.npy")
        assert y.dtype == np.float64 and t.dtype == np.float64
        assert np.array_equal(y, Ys[idx]) and np.array_equal(t, taus[idx]), lay


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path):
    """A plain one-GPU run: exactly --steps timed steps, the headline keys and no side leg; --dump-outputs holds tau and Y of the
    last step on the seeded sample subset, against the CPU oracle on the same seeded inputs."""
    torch = pytest.importorskip("torch")
    import numpy as np
    import bench
    from oracle.oracle import OracleChain
    N = 40000
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--samples", str(N),
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "evals/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert not {"drop_in_layout", "tuned_output_placement", "config4", "extras", "config4_library", "cpu_baseline"} & set(d)
    assert sorted(os.listdir(tmp_path)) == ["Y.npy", "tau.npy"]
    Y, tau = np.load(tmp_path / "Y.npy"), np.load(tmp_path / "tau.npy")
    idx = bench.dump_indices(N)
    assert Y.dtype == np.float64 and Y.shape == (len(idx), 6, 60) and tau.shape == (len(idx), 6)
    # the inputs bench.py made: torch's seeded generator on the device, in the same order
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0x5EED0002)
    q, dq, ddq = (torch.rand((N, 6), dtype=torch.float64, device=dev, generator=gen) * 2 - 1 for _ in range(3))
    q, dq, ddq = (x.cpu().numpy()[idx] for x in (q, dq, ddq))
    ref = OracleChain(os.path.join(FIXTURES, "ur10_like.urdf"), "base_link", "wrist_3_link", bench.GRAVITY)
    Yr, tr = ref.regressor(q, dq, ddq), ref.joint_torque(q, dq, ddq)
    assert np.abs(Y - Yr).max() / max(1.0, np.abs(Yr).max()) <= 1e-11
    assert np.abs(tau - tr).max() / max(1.0, np.abs(tr).max()) <= 1e-11


def test_single_rank_dry_needs_no_launcher():
    p = _run("--gpus", "1", "--samples", "10")
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["n_ranks_seen"] == 1


def test_world_size_mismatch_is_an_error_not_an_assert():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry", "--backend", "gloo"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)
    assert p.returncode == 2 and "WORLD_SIZE=3" in p.stderr


def test_single_process_argument_path_dry():
    """`bench.py --single-process --gpus N` = configs[3] through the library's in-process RCCL path (one process, no torch.distributed,
    no launcher); on the CPU box only the argument path can run."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--single-process", "--gpus", "8", "--dry", "--samples", "1000"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert d == {"metric": "config4_library", "dry": True, "n_gpus": 8, "steps": 20, "samples_per_gpu": 1000,
                 "legs": ["config4_library", "config3_library", "config5_library"]}
