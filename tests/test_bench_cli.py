"""bench.py's command line: a plain run measures the headline figure only, `--full` switches the other legs on,
`--dump-outputs DIR` writes the last timed step's estimates (float64 re/im, a fixed seeded row sample beyond the size
cap) and the inputs are the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_the_other_legs_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.cpu_seconds == 0 and a.no_parity and a.no_extras and not a.dropin
    # the side-line switches mean nothing without --full
    a = _parse(monkeypatch, "--dropin", "--cpu-seconds", "5")
    assert a.cpu_seconds == 0 and a.no_parity and a.no_extras and not a.dropin


def test_full_keeps_every_leg_and_its_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and a.cpu_seconds == 8.0 and not a.no_parity and not a.no_extras and not a.dropin
    a = _parse(monkeypatch, "--full", "--cpu-seconds", "0", "--no-extras", "--no-parity", "--dropin")
    assert a.cpu_seconds == 0 and a.no_parity and a.no_extras and a.dropin


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_small_batch_is_written_whole(tmp_path):
    rng = np.random.default_rng(0)
    h = rng.standard_normal((37, 5)) + 1j * rng.standard_normal((37, 5))
    info = bench.dump_outputs(str(tmp_path / "d"), h)
    a = np.load(tmp_path / "d" / "h_hat.npy")
    assert a.dtype == np.float64 and a.shape == (37, 5, 2)
    np.testing.assert_array_equal(a[..., 0], h.real)
    np.testing.assert_array_equal(a[..., 1], h.imag)
    assert info["h_hat.npy"]["rows"] == "all" and info["h_hat.npy"]["shape"] == [37, 5, 2]


def test_dump_outputs_samples_fixed_rows_beyond_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16 * 4 * 10)  # room for 10 rows of N = 4
    h = (np.arange(100 * 4).reshape(100, 4) + 0.5j).astype(np.complex128)
    bench.dump_outputs(str(tmp_path / "a"), h)
    bench.dump_outputs(str(tmp_path / "b"), h)
    a, b = np.load(tmp_path / "a" / "h_hat.npy"), np.load(tmp_path / "b" / "h_hat.npy")
    assert a.shape == (10, 4, 2) and a.nbytes <= 16 * 4 * 10
    np.testing.assert_array_equal(a, b)
    rows = (a[:, 0, 0] / 4).astype(int)  # h[r, 0].real = 4 r
    assert len(set(rows)) == 10 and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(a[..., 0], h.real[rows])


def test_metric_dump_stays_below_the_size_limit():
    cfg = bench.CONFIGS["metric"]
    keep = bench.DUMP_MAX_BYTES // (16 * cfg["N"])
    assert 0 < keep < cfg["B"] and keep * cfg["N"] * 16 <= 64e6


def test_inputs_are_the_same_from_run_to_run():
    cfg = dict(bench.CONFIGS["cfg1"], B=64)
    a, b = bench.make_inputs(cfg, 0), bench.make_inputs(cfg, 0)
    for x, y in zip(a[:5], b[:5]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    """A plain run at the smallest config: the headline keys, none of the --full legs, and a dump that is the
    estimate the line's own MSE was computed from."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cfg1", "--steps",
                        "3", "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True,
                       timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["value"] > 0 and r["higher_is_better"] is True
    assert r["unit"] == "channel estimates/s" and r["dtype"] == "f64" and r["metric"] == bench.METRIC
    # value = B / step time; ms_per_step is printed to 1e-4 ms and value to 0.1
    assert abs(r["value"] - 1000 / (r["ms_per_step"] * 1e-3)) <= (1e-4 / r["ms_per_step"] + 1e-6) * r["value"] + 0.1
    assert r["parity"] is None and r["cpu_baseline"] is None and "fast_path" not in r and "dropin" not in r
    a = np.load(out / "h_hat.npy")
    assert a.dtype == np.float64 and a.shape == (1000, 32, 2) and np.isfinite(a).all()
    h = bench.make_inputs(dict(bench.CONFIGS["cfg1"]), 0)[3]
    mse = float(np.mean(np.abs(a[..., 0] + 1j * a[..., 1] - h) ** 2))
    assert abs(mse - r["mse"]) <= 1e-12 * max(1.0, abs(mse))
