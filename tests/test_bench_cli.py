"""bench.py's command line: a plain run, ``--full`` and ``--dump-outputs``
(CPU engine, one small application, one step)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, tag, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
           "--engine", "cpu", "--apps", "nn,pathfinder", "--trace-dir", str(tmp_path / "traces"),
           "--dump-outputs", str(tmp_path / tag), *extra]
    env = dict(os.environ, OMP_NUM_THREADS="1", ASIM_CPU_JOBS="2")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])
    dump = {f[:-4]: np.load(tmp_path / tag / f) for f in sorted(os.listdir(tmp_path / tag))}
    return out, dump


def test_plain_run_is_lean_and_full_adds_the_rest_with_identical_dumps(native, tmp_path):
    plain, d0 = _bench(tmp_path, "plain")
    full, d1 = _bench(tmp_path, "full", "--full")
    for out in (plain, full):
        assert out["metric"] == "sim KIPS (whole node)" and out["value"] > 0 and out["higher_is_better"] is True
        assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["dtype"] and out["unit"]
    # what the headline does not need is reported under --full only
    assert "cycle_mae_vs_hw" not in plain and "cycle_mae_vs_hw" in full
    # the last timed step's results: float64, one row per rank, apps in name order
    assert sorted(d0) == ["app_cycles", "app_insn", "totals"]
    assert all(a.dtype == np.float64 for a in d0.values())
    # (nn, pathfinder and the all-reduce example that closes the step)
    assert d0["totals"].shape == (1, 2) and d0["app_insn"].shape == d0["app_cycles"].shape == (1, 3)
    assert d0["totals"][0, 0] == d0["app_insn"].sum() == plain["config"]["sim_insn_per_step_per_rank"]
    assert d0["totals"][0, 1] == d0["app_cycles"].sum() == plain["config"]["sim_cycles_per_step_per_rank"]
    assert (d0["app_insn"] > 0).all() and (d0["app_cycles"] > 0).all()
    # same arguments, same inputs: two runs agree output for output
    for k in d0:
        assert np.array_equal(d0[k], d1[k]), k
