"""bench.py's two kinds of run: a plain run carries the timed steps alone, --full everything else as well."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = {"metric": "stiffness_assembly_elements_per_s", "unit": "elements/s", "higher_is_better": True, "dtype": "f64"}
FULL_ONLY = ("roofline", "hbm_measured", "variants", "pcg", "pcg_two_level", "pcg_multigrid", "one_shot", "strong_scaling_n1", "cpu_baseline")


def _parse(argv, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", [BENCH] + argv)
    return mod.parse()


def test_full_is_off_by_default(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "4", "--warmup", "2"], monkeypatch)
    assert a.full is False and (a.steps, a.warmup, a.grid) == (4, 2, 60)
    a = _parse(["--full", "--no-cpu"], monkeypatch)
    assert a.full is True and a.no_cpu is True


def _run(args, timeout):
    p = subprocess.run([sys.executable, BENCH] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_is_the_timed_steps_alone(tmp_path):
    d = _run(["--gpus", "1", "--grid", "6", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path)], timeout=300)
    for k, v in HEADLINE.items():
        assert d[k] == v
    assert (d["steps"], d["warmup"]) == (3, 2)
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["elements"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["config"]["elements"] == 24 * 6 ** 3
    assert not [k for k in FULL_ONLY if k in d]
    for name in ("K_rows", "K_cols", "K_values"):
        assert np.load(str(tmp_path / (name + ".npy"))).dtype == np.float64


@pytest.mark.gpu
def test_full_line_keeps_the_rest(tmp_path):
    # the 119^3 leg and the CPU baseline are left out: their own runs are minutes long
    d = _run(["--gpus", "1", "--grid", "6", "--steps", "3", "--warmup", "2", "--full", "--no-strong-n1", "--no-cpu"], timeout=600)
    for k, v in HEADLINE.items():
        assert d[k] == v
    assert d["roofline"]["kernel_ms"] > 0 and d["hbm_measured"]["triad_GBs"] > 0
    assert d["pcg"]["converged"] and d["pcg_multigrid"]["converged"]
    assert {"atomic_scatter", "deterministic", "orderings"} <= set(d["variants"])
