#!/usr/bin/env python3
"""Time one open-loop sweep grid on the host path and on the GPU engine.

The grid is a load-latency study of one network: 9 rates x the 7 traffic
patterns x 4 seeds = 252 points of an 8x8 mesh, 5000 cycles each.  The host
step runs the points one after the other on one core, as ``booksim.sweep``
does with ``engine="cpu"``; the GPU step sends the whole grid as one batch
(``engine="gpu"``, one wavefront per point).  Both steps run in child
processes; each GPU step runs under its own ``timeout -k 10`` and any failure
stops the script.  The record (JSON) holds both wall times, their ratio, how
the batch was packed into launches, whether the two engines' results are
equal, and the kernel's registers, LDS and scratch.

    python tools/icnt_sweep_bench.py --out profiles/icnt_sweep/record.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RATES = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.8, 1.0)
PATTERNS = ("uniform", "transpose", "bitcomp", "bitrev", "shuffle", "tornado", "neighbor")


def grid(a):
    return [(t, r, a.packet_flits, a.cycles, a.warmup, s) for t in PATTERNS for r in RATES
            for s in range(1, a.seeds + 1)]


def network(a) -> str:
    from accel_sim_framework_distributed_amd.models import presets
    return presets.render_icnt(presets.icnt_params(k=a.k, n=2, topology="mesh", num_vcs=a.vcs, vc_buf_size=a.buf,
                                                   internal_speedup="1.0"))


def worker(a) -> int:
    """One engine over the grid; writes {seconds, results, ...} to a.out."""
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    if a.worker == "gpu":
        import torch  # bind torch's HIP runtime first  # noqa: F401
    from accel_sim_framework_distributed_amd import _native
    mod = _native.load()
    text, pts = network(a), grid(a)
    rec = {"engine": a.worker, "points": len(pts)}
    if a.worker == "gpu":
        if not mod.gpu_available():
            print("no usable HIP device", file=sys.stderr)
            return 2
        mod.icnt_open_loop_batch(text, pts[:1], engine="gpu")  # the runtime's start-up is not the sweep's time
    t0 = time.perf_counter()
    if a.worker != "gpu":  # the single-threaded host loop (cpu-par: the lane-parallel pass on one lane)
        res = [mod.icnt_open_loop_batch(text, [p], engine=a.worker)[0] for p in pts]
    else:
        res = mod.icnt_open_loop_batch(text, pts, engine="gpu", mem_budget_mb=a.mem_budget_mb)
    rec["seconds"] = time.perf_counter() - t0
    if a.worker == "gpu":
        rec["batch"] = dict(mod.icnt_open_loop_batch_stats())
        rec["kernel"] = dict(mod.icnt_sweep_kernel_info())
    rec["results"] = [dict(r) for r in res]
    with open(a.out, "w") as f:
        json.dump(rec, f)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="icnt_sweep_record.json")
    ap.add_argument("--k", type=int, default=8, help="k x k mesh")
    ap.add_argument("--vcs", type=int, default=2)
    ap.add_argument("--buf", type=int, default=8)
    ap.add_argument("--cycles", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--packet-flits", type=int, default=1)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--mem-budget-mb", type=int, default=0)
    ap.add_argument("--gpu-timeout", type=int, default=900, help="seconds the GPU step may take")
    ap.add_argument("--worker", choices=("cpu", "cpu-par", "gpu"), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        return worker(a)
    common = ["--k", str(a.k), "--vcs", str(a.vcs), "--buf", str(a.buf), "--cycles", str(a.cycles), "--warmup",
              str(a.warmup), "--packet-flits", str(a.packet_flits), "--seeds", str(a.seeds), "--mem-budget-mb",
              str(a.mem_budget_mb)]
    recs = {}
    with tempfile.TemporaryDirectory(prefix="icnt_sweep_") as tmp:
        for eng in ("gpu", "cpu"):
            out = os.path.join(tmp, eng + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", eng, "--out", out] + common
            if eng == "gpu":  # every GPU step under its own time limit
                cmd = ["timeout", "-k", "10", str(a.gpu_timeout)] + cmd
            print("+", " ".join(cmd), flush=True)
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"{eng} step failed (exit status {rc}): stopping", file=sys.stderr)
                return rc or 1
            recs[eng] = json.load(open(out))
            print(f"{eng}: {recs[eng]['seconds']:.2f} s for {recs[eng]['points']} points", flush=True)
    cpu, gpu = recs["cpu"], recs["gpu"]
    equal = cpu["results"] == gpu["results"]
    rec = {
        "grid": {"network": f"{a.k}x{a.k} mesh, {a.vcs} VCs x {a.buf} flits", "rates": list(RATES),
                 "patterns": list(PATTERNS), "seeds": a.seeds, "cycles": a.cycles, "warmup": a.warmup,
                 "packet_flits": a.packet_flits, "points": cpu["points"],
                 "packets": sum(r["packets"] for r in cpu["results"]),
                 "switch_passes": sum(r["activity"]["switch_passes"] for r in cpu["results"])},
        "cpu_seconds": cpu["seconds"], "gpu_seconds": gpu["seconds"],
        "cpu_over_gpu": cpu["seconds"] / gpu["seconds"] if gpu["seconds"] else None,
        "gpu_results_equal_cpu": equal,
        "batch": gpu["batch"], "kernel": gpu["kernel"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "grid"}))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
