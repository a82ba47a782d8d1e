"""CPU: bench.py's multi-GPU launcher without a GPU.

``python bench.py --gpus 2 --dry-run`` spawns two ranks itself (one process per
GPU in a real run), they rendezvous on 127.0.0.1 over gloo, time the same number
of steps between barriers and rank 0 reports the slowest rank -- the path the
driver's ``--gpus N`` runs take, with the GPU work replaced by a sleep."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=240, env=e, cwd=ROOT)


@pytest.mark.parametrize("mode", ["streams", "shard"])
def test_gpus_2_spawns_two_ranks_that_agree(mode):
    # --full: the companion configs below are not part of a plain run
    r = _bench("--gpus", "2", "--dry-run", "--full", "--steps", "4", "--warmup", "1", "--mode", mode,
               "--cpu-seconds", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # only rank 0 prints
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["warmup"] == 1
    per = out["per_rank_s"]
    assert len(per) == 2
    # both ranks timed the same barrier-bracketed region: equal to within the barrier skew
    assert abs(per[0] - per[1]) < 0.05
    # reported step time is the slowest rank's; rank 1 sleeps twice as long per step
    assert out["ms_per_step"] == pytest.approx(max(per) * 1e3 / 4, rel=1e-3)
    assert out["ms_per_step"] >= 2.0
    assert out["scaling"] == ("weak" if mode == "streams" else "strong")
    assert out["config"]["parallelism"] == f"{mode}2"
    if mode == "streams":
        # the other BASELINE configs ride along in multi-GPU runs, each with every rank's time
        for key in ("config2", "config4", "config5", "f32"):
            assert key in out, key
            assert len(out[key]["per_rank_s"]) == 2, key
        assert out["config4"]["scaling"] == "strong" and out["config5"]["scaling"] == "weak"


def test_plain_run_is_the_headline_only():
    """Without --full the line carries the headline and the timed region's roofline, nothing
    that takes a run of its own; --dump-outputs of a dry run has nothing to write."""
    r = _bench("--gpus", "1", "--dry-run", "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert key in out, key
    assert out["steps"] == 3 and out["ms_per_step"] == pytest.approx(out["per_rank_s"][0] * 1e3 / 3, rel=1e-3)
    for key in ("f32", "config2", "config4", "config4_f32", "config5", "host_fed", "demod", "cpu_baseline"):
        assert key not in out, key
    assert "copy_GBps" not in out["roofline"]


def test_dump_sample_is_fixed_and_within_budget():
    sys.path.insert(0, ROOT)
    import bench

    n, total = 65536, 500
    idx = bench.sample_rows(total, n, bench.DUMP_BUDGET - 8 * n)
    assert (idx == bench.sample_rows(total, n, bench.DUMP_BUDGET - 8 * n)).all()  # seeded: the same every run
    assert len(set(idx.tolist())) == len(idx) and idx.min() >= 0 and idx.max() < total and (idx[1:] > idx[:-1]).all()
    assert len(idx) * n * 4 + 8 * n <= bench.DUMP_BUDGET <= 64 * 10 ** 6
    assert (len(idx) + 1) * n * 4 + 8 * n > bench.DUMP_BUDGET  # and no smaller than the budget allows
    assert bench.sample_rows(16, 1024, bench.DUMP_BUDGET).tolist() == list(range(16))  # all rows when they fit


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_steps_state(tmp_path):
    """--dump-outputs on a small stream: float32 arrays a caller reads after the last timed step.
    The ring holds the last 16 rows, peak-hold covers every frame so far, the EMA lies between
    the extremes its rows ever took."""
    import numpy as np

    args = ("--gpus", "1", "--steps", "2", "--warmup", "1", "--fft-size", "1024", "--frames", "16", "--ring-rows", "16",
            "--calls-per-step", "3", "--pool-mib", "1", "--dump-outputs")
    r = _bench(*args, str(tmp_path / "a"))
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and "f32" not in out
    assert sorted(os.listdir(tmp_path / "a")) == ["ema.npy", "peaks.npy", "ring_rows.npy"]
    ring, peaks, ema = (np.load(tmp_path / "a" / f"{k}.npy") for k in ("ring_rows", "peaks", "ema"))
    assert ring.dtype == peaks.dtype == ema.dtype == np.float32
    assert ring.shape == (16, 1024) and peaks.shape == ema.shape == (1024,)
    assert np.isfinite(ring).all() and np.isfinite(peaks).all() and np.isfinite(ema).all()
    assert (peaks >= ring.max(0)).all()
    assert (ema <= peaks + 1e-4).all()  # a convex combination of rows, to within float32 rounding at these levels
    assert ring.max() > ring.mean() + 20  # the tone stands out of the noise: real spectra, not a cleared buffer


def test_world_size_mismatch_is_an_error():
    r = _bench("--gpus", "2", "--dry-run", "--steps", "1", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in r.stderr


def test_single_rank_dry_run():
    r = _bench("--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "0", "--cpu-seconds", "0", "--demod-steps", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and len(out["per_rank_s"]) == 1
