#!/usr/bin/env python3
"""Batch time against the window on one closed-loop grid, on the host path and
on the GPU kernel.

The grid is M in {1, 2, 4, 8, 16, 32, unlimited} x {uniform, transpose,
bitcomp, neighbor} x 3 seeds = 84 batch points of an 8x8 mesh: every node
creates 64 requests at cycle 0, sizes 1/5/5/1 flits (read request, read reply,
write request, write reply), write fraction 0.3.  Two forms of the same work:

  cpu  ``icnt_closed_loop_batch(engine="cpu")``: one core, one point after the
       other (rt_simulate_closed)
  gpu  ``engine="gpu"``: one launch, one wavefront per point

Every form runs once untimed, then ``--repeats`` times timed.  The GPU form
runs in one child process under ``timeout -k 10``, the host form in another;
any failure stops the script.  The record (JSON) holds every time, whether
all results are equal (every array, the state image, every summary), the
batch-time table, how the batch was packed, and the registers, scratch and LDS
of the four sweep kernels.

    python tools/icnt_cl_bench.py --out profiles/icnt_closed_loop/record.json
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WINDOWS = (1, 2, 4, 8, 16, 32, 0)
PATTERNS = ("uniform", "transpose", "bitcomp", "neighbor")
SIZES = dict(read_request_size=1, read_reply_size=5, write_request_size=5, write_reply_size=1)


def grid(a):
    return [dict(SIZES, traffic=t, max_outstanding=m, seed=s, batch_size=a.batch_size, write_fraction=0.3,
                 reply_delay=a.reply_delay)
            for t in PATTERNS for m in WINDOWS for s in range(1, a.seeds + 1)]


def network(a) -> str:
    from accel_sim_framework_distributed_amd.models import presets
    return presets.render_icnt(presets.icnt_params(k=a.k, n=2, topology="mesh", num_vcs=a.vcs, vc_buf_size=a.buf,
                                                   internal_speedup="1.0", flit_size=32))


def timed(fn, repeats):
    res = fn()  # once untimed
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fn()
        secs.append(time.perf_counter() - t0)
    return res, secs


def worker(a) -> int:
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    if a.worker == "gpu":
        import torch  # bind torch's HIP runtime first  # noqa: F401
    from accel_sim_framework_distributed_amd import _native
    mod = _native.load()
    text, pts = network(a), grid(a)
    rec = {"points": len(pts)}
    if a.worker == "cpu":
        rec["results"], rec["cpu_seconds"] = timed(
            lambda: mod.icnt_closed_loop_batch(text, pts, engine="cpu", arrivals=True), a.repeats)
    else:
        if not mod.gpu_available():
            print("no usable HIP device", file=sys.stderr)
            return 2
        rec["results"], rec["gpu_seconds"] = timed(lambda: mod.icnt_closed_loop_batch(
            text, pts, engine="gpu", arrivals=True, mem_budget_mb=a.mem_budget_mb), a.repeats)
        rec["batch"] = dict(mod.icnt_open_loop_batch_stats())
        rec["kernels"] = {"icnt_cl_kernel": dict(mod.icnt_cl_kernel_info()),
                          "icnt_sweep_kernel": dict(mod.icnt_sweep_kernel_info()),
                          "icnt_rr_kernel": dict(mod.icnt_rr_kernel_info()),
                          "icnt_net_kernel": dict(mod.icnt_net_kernel_info())}
    with open(a.out, "wb") as f:
        pickle.dump(rec, f)
    return 0


def same(a, b) -> bool:
    import numpy as np
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="icnt_cl_record.json")
    ap.add_argument("--k", type=int, default=8, help="k x k mesh")
    ap.add_argument("--vcs", type=int, default=2)
    ap.add_argument("--buf", type=int, default=8)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--reply-delay", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mem-budget-mb", type=int, default=0)
    ap.add_argument("--gpu-timeout", type=int, default=300, help="seconds the GPU step may take")
    ap.add_argument("--worker", choices=("cpu", "gpu"), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        return worker(a)
    common = ["--k", str(a.k), "--vcs", str(a.vcs), "--buf", str(a.buf), "--batch-size", str(a.batch_size),
              "--reply-delay", str(a.reply_delay), "--seeds", str(a.seeds), "--repeats", str(a.repeats),
              "--mem-budget-mb", str(a.mem_budget_mb)]
    recs = {}
    with tempfile.TemporaryDirectory(prefix="icnt_cl_") as tmp:
        for eng in ("gpu", "cpu"):
            out = os.path.join(tmp, eng + ".pkl")
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", eng, "--out", out] + common
            if eng == "gpu":  # the GPU step under its own time limit
                cmd = ["timeout", "-k", "10", str(a.gpu_timeout)] + cmd
            print("+", " ".join(cmd), flush=True)
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"{eng} step failed (exit status {rc}): stopping", file=sys.stderr)
                return rc or 1
            with open(out, "rb") as f:
                recs[eng] = pickle.load(f)
    cpu, gpu = recs["cpu"], recs["gpu"]
    equal = same(gpu["results"], cpu["results"])
    res = cpu["results"]
    per = a.seeds
    table = {}
    for ti, t in enumerate(PATTERNS):
        for mi, m in enumerate(WINDOWS):
            g = res[(ti * len(WINDOWS) + mi) * per:(ti * len(WINDOWS) + mi + 1) * per]
            table.setdefault(t, {})[str(m)] = {
                "batch_time": [int(r["batch_time"]) for r in g],
                "round_trip_latency": sum(r["round_trip_latency"] for r in g) / per,
                "issue_stall": sum(r["issue_stall"] for r in g) / per,
                "avg_outstanding": sum(r["avg_outstanding"] for r in g) / per}
    rec = {
        "grid": {"network": f"{a.k}x{a.k} mesh, {a.vcs} VCs x {a.buf} flits, 32-byte flits", "windows": list(WINDOWS),
                 "patterns": list(PATTERNS), "seeds": a.seeds, "batch_size": a.batch_size, "sizes": SIZES,
                 "write_fraction": 0.3, "reply_delay": a.reply_delay, "points": cpu["points"],
                 "requests": sum(int(r["requests"]) for r in res),
                 "switch_passes": sum(int(r["activity"]["switch_passes"]) for r in res),
                 "deadlocked": sum(int(r["deadlocked"]) for r in res)},
        "repeats": a.repeats, "cpu_seconds": cpu["cpu_seconds"], "gpu_seconds": gpu["gpu_seconds"],
        "cpu_over_gpu": min(cpu["cpu_seconds"]) / min(gpu["gpu_seconds"]),
        "gpu_results_equal_cpu": equal, "batch": gpu["batch"], "kernels": gpu["kernels"], "table": table,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k not in ("grid", "table")}))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
