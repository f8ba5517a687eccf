"""bench.py must be launchable for N ranks by ONE command (`python bench.py --gpus N`) and by
torch.distributed.run; without GPUs the launch + rendezvous + reductions are exercised over gloo
(--dry-run) and the real run ends with a clean "needs N GPUs" message, not a launcher error."""

import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(cmd, **kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300, **kw)


def _line(out):
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_self_spawn_dry_run_weak_and_strong():
    out = _run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "2"])
    assert out.returncode == 0, out.stderr
    rec = _line(out)
    assert rec["dry_run"] and rec["n_gpus"] == 2 and rec["scaling"] == "weak"
    assert rec["walkers_total"] == 8192 and rec["walkers_rank0"] == [0, 4096]
    assert rec["rccl_ranks"] == 2 and rec["collective_backend"].startswith("gloo")  # the rank census of the bench line
    # configs 4 and 5 as N-rank workloads: independent shards / one ladder over all ranks with the
    # exchange (host-staged all-gather here) inside the timed region
    c4, c5 = rec["other_configs"]
    assert c4["n_gpus"] == 2 and c4["replicas"] == 2048
    assert c5["replicas"] == 4096 and c5["exchanges"] == 6 and c5["exchange_attempts"] > 0
    assert c5["rungs_are_a_permutation"] and c5["ranks_agree"] and "all-gather over 2 ranks" in c5["exchange_path"]
    out = _run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--steps", "2", "--scaling", "strong"])
    assert out.returncode == 0, out.stderr
    rec = _line(out)
    assert rec["scaling"] == "strong" and rec["walkers_total"] == 4096 and rec["walkers_rank0"] == [0, 2048]


def test_torchrun_form_still_works():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2",
                "--dry-run", "--steps", "2"])
    assert out.returncode == 0, out.stderr[-2000:]
    assert _line(out)["walkers_total"] == 8192


def test_without_gpus_the_error_is_about_gpus_not_the_launcher():
    import torch

    if torch.cuda.is_available():
        return  # on a GPU box this command would really run the benchmark
    out = _run([sys.executable, BENCH, "--gpus", "2", "--steps", "1"])
    assert out.returncode == 3
    assert "needs 2 AMD GPU" in out.stderr and "rendezvous work" in out.stderr
    out = _run([sys.executable, BENCH, "--gpus", "3"], )
    assert out.returncode == 3 and "needs 3 AMD GPU" in out.stderr


def test_gpus_must_match_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dry-run"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "WORLD_SIZE=2" in out.stderr


def test_dump_outputs_writes_float_arrays_within_64_mb(tmp_path):
    """--dump-outputs at the headline's shape: every array of the state as float32 / float64, the occupancy of a
    seeded sample of walkers, 64 MB at most."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    R, N, F = 4096, 4096, 8
    rng = np.random.default_rng(3)
    state = dict(occupancy=rng.integers(0, 2, (R, N), dtype=np.int32), features=rng.random((R, F)),
                 enthalpy=rng.random(R), n_accepted=np.arange(R, dtype=np.uint64),
                 n_steps=np.full(R, 10**6, dtype=np.uint64), accepted=rng.random(R) < 0.5)
    dumps = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), dict(state))
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert set(a) == {"occupancy_sample", "occupancy_walkers", "features", "enthalpy", "n_accepted", "n_steps",
                      "accepted"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64 * 2**20
    rows = a["occupancy_walkers"].astype(np.int64)
    assert len(rows) == bench.DUMP_OCC_WALKERS and len(set(rows)) == len(rows)
    np.testing.assert_array_equal(a["occupancy_sample"], state["occupancy"][rows])
    for k in ("features", "enthalpy", "n_accepted", "n_steps", "accepted"):
        np.testing.assert_array_equal(a[k], state[k].astype(np.float64).reshape(a[k].shape))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.gpu
def test_dump_outputs_are_the_state_after_the_timed_steps(tmp_path):
    """Two runs with the same arguments dump the same arrays, and every walker has taken exactly (warmup + steps)
    launches of --mc-per-step steps."""
    import numpy as np

    warmup, steps, mc = 1, 3, 2000
    dumps = []
    for d in ("a", "b"):
        out = _run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                    "--mc-per-step", str(mc), "--replicas", "256", "--no-other-configs", "--no-cpu-baseline",
                    "--dump-outputs", str(tmp_path / d)])
        assert out.returncode == 0, out.stderr[-2000:]
        assert _line(out)["steps"] == steps
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert (a["n_steps"] == (warmup + steps) * mc).all()
    assert a["enthalpy"].shape == (256,) and a["occupancy_sample"].shape == (256, 4096)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    """Without --full the line is the headline and its roofline from the committed PMC figures: nothing that takes
    runs of its own (other configurations, the CPU oracle, the live HBM probe)."""
    out = _run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--mc-per-step", "2000",
                "--replicas", "256"])
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _line(out)
    assert rec["unit"] == "attempted flips/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["steps"] == 2 and rec["warmup"] == 1
    assert not {"other_configs", "cpu_baseline", "gpu_over_cpu"} & set(rec)
    assert "runs with --full" in rec["roofline"]["measured_peak_source"]


@pytest.mark.gpu
def test_full_run_takes_the_live_hbm_probe():
    """--full measures the HBM peak live; --no-other-configs / --no-cpu-baseline still leave those two out."""
    out = _run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--mc-per-step", "2000",
                "--replicas", "256", "--full", "--no-other-configs", "--no-cpu-baseline"])
    assert out.returncode == 0, out.stderr[-2000:]
    rec = _line(out)
    assert rec["roofline"]["measured_peak_source"].startswith("live read / triad probe")
    assert not {"other_configs", "cpu_baseline"} & set(rec)
