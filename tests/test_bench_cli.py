"""bench.py's command line: a plain run prints only the headline figure, --full adds the
profiled pass and the rooflines, --dump-outputs writes the last timed step's state so that two
builds can be compared output for output."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "compute_roofline", "latency_bound", "step_roofline",
             "ms_per_step_profiled", "phase_ms_per_step", "cpu_baseline")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_and_within_budget(tmp_path):
    """CPU: small arrays are written whole, a large one as the same seeded sample every time,
    and n planes of any size stay within the budget."""
    B = _bench_module()
    n_arrays = 6
    cap = B.DUMP_BUDGET_BYTES // 8 // n_arrays
    big = np.arange(cap + 1000, dtype=np.float64).reshape(-1, 8)   # value == flat index
    small = np.linspace(0.0, 1.0, 77)
    for sub in ("a", "b"):
        d = B._Dump(str(tmp_path / sub), n_arrays)
        d.add("big", big)
        d.add("small", small)
        d.add("ints", np.arange(5, dtype=np.int32))
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (cap,)
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[-1] < big.size          # distinct, in-range indices
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert np.load(tmp_path / "a" / "ints.npy").dtype == np.float64
    assert n_arrays * cap * 8 <= B.DUMP_BUDGET_BYTES <= 64 << 20


def _run(*extra):
    cmd = [sys.executable, BENCH, "--gpus", "1", "--grid", "256", "--steps", "3", "--warmup", "1",
           *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dump_is_repeatable(gpu, tmp_path):
    lines = [_run("--dump-outputs", str(tmp_path / k)) for k in ("a", "b")]
    for line in lines:
        assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
        assert line["value"] == pytest.approx(256 * 256 / (line["ms_per_step"] * 1e-3))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"u.npy", "v.npy", "p.npy", "X1.npy", "X2.npy", "phi.npy", "diag_cx.npy"} <= set(names)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.all(np.isfinite(a)), n
        np.testing.assert_array_equal(a, b, err_msg=n)
    assert np.load(tmp_path / "a" / "u.npy").shape == (256, 256)
    assert np.load(tmp_path / "a" / "diag_cx.npy").shape[0] >= 3


@pytest.mark.gpu
def test_full_run_adds_the_profiled_figures(gpu):
    line = _run("--full", "--no-cpu-baseline")
    assert all(k in line for k in HEADLINE)
    assert all(k in line for k in FULL_ONLY if k != "cpu_baseline") and "cpu_baseline" not in line
    assert line["steps"] == 3 and line["ms_per_step_profiled"] > 0
    assert line["phase_ms_per_step"]["momentum"] > 0
