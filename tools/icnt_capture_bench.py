#!/usr/bin/env python3
"""Time the network capture and the sweep of a captured list over networks.

Two measurements, one record:

  capture  the same simulation with ``-icnt_capture`` off and on, on both
           cycle engines, ``--repeats`` times each after one untimed run:
           what capturing costs.  With ``--parent-so FILE`` (the native module
           of the parent commit's build) the capture-off run is also timed on
           that module, in a process of its own, and the record says whether
           the two capture-off times agree within the run-to-run spread seen
  sweep    the request subnet of the captured file over ``--networks``
           candidate networks (8x8 meshes and tori with 16 / 32 / 40 / 64-byte
           flits, 1 / 2 / 4 VCs, 4 / 8 flit buffers) through
           ``icnt_replay_networks``: ``gpu`` (one wavefront per network) against
           ``cpu`` (one network after the other), and whether the results are
           equal

The simulated machine is QV100 with 16 clusters and 8 memory channels on an
8 x 8 mesh under the router model (``-icnt_link_contention 2``); the
application is the generated pathfinder trace (``--cols``, ``--rows``).  The
GPU steps run in a child process under ``timeout -k 10``; a failing step stops
the script.

    python tools/icnt_capture_bench.py --out profiles/icnt_capture/record.json
"""
from __future__ import annotations

import argparse
import itertools
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

SMALL = {"-gpgpu_n_clusters": "16", "-gpgpu_n_mem": "8"}


def machine(tmp, a):
    from accel_sim_framework_distributed_amd.models import presets
    from accel_sim_framework_distributed_amd.tracegen import rodinia
    icnt = os.path.join(tmp, "mesh.icnt")
    with open(icnt, "w") as f:
        f.write(presets.render_icnt(presets.icnt_params(k=8, n=2, topology="mesh", num_vcs=2)))
    kl = rodinia.write_app(os.path.join(tmp, "pf"), rodinia.pathfinder(a.cols, a.rows, 2))
    extra = dict(SMALL, **{"-network_mode": "1", "-inter_config_file": icnt, "-icnt_link_contention": "2",
                           "-gpgpu_perf_sim_memcpy": "0"})
    return kl, extra


def networks(n):
    from accel_sim_framework_distributed_amd.models import presets
    grid = itertools.product(("mesh", "torus"), (16, 32, 40, 64), (2, 4, 1), (8, 4))
    out = []
    for topo, flit, vcs, buf in grid:
        if topo == "torus" and vcs < 2:
            continue  # a torus needs dateline VC classes
        out.append((f"{topo} flit{flit} vc{vcs} buf{buf}",
                    presets.render_icnt(presets.icnt_params(k=8, n=2, topology=topo, flit_size=flit, num_vcs=vcs,
                                                            vc_buf_size=buf))))
    return out[:n]


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
    gpu = a.worker == "gpu"
    if gpu:
        import torch  # bind torch's HIP runtime first  # noqa: F401
    from accel_sim_framework_distributed_amd import _native, sim
    from accel_sim_framework_distributed_amd.icnt import booksim, capture
    mod = _native.load(prefer_torch_runtime=gpu)
    if gpu and not mod.gpu_available():
        print("no usable HIP device", file=sys.stderr)
        return 2
    eng = "gpu" if gpu else "cpu"
    kl, extra = machine(a.tmp, a)
    path = os.path.join(a.tmp, f"{eng}.icap")

    def run(cap):
        r = sim.Simulator("QV100", kl, eng, extra, torch_runtime=gpu, icnt_capture=path if cap else None).run()
        return (r.tot_cycle, r.icnt_capture_request_packets, r.icnt_capture_reply_packets, r.sim_s)
    rec = {}
    off, rec["off_seconds"] = timed(lambda: run(False), a.repeats)
    if a.only_off:  # the parent commit's module: nothing to capture with
        rec["cycles"] = off[0]
        with open(a.out, "wb") as f:
            pickle.dump(rec, f)
        return 0
    on, rec["on_seconds"] = timed(lambda: run(True), a.repeats)
    rec.update(cycles=on[0], same_cycles=on[0] == off[0], request_packets=on[1], reply_packets=on[2])
    with open(path, "rb") as f:
        rec["file"] = f.read()
    q = capture.load(path).request
    nets = networks(a.networks)
    res, rec["sweep_seconds"] = timed(lambda: booksim.replay_networks(
        q.src, q.dst, q.bytes, q.tinj, [t for _, t in nets], engine=eng, arrivals=True), a.repeats)
    rec["sweep"] = res
    rec["networks"] = [n for n, _ in nets]
    if gpu:
        rec["batch"] = dict(mod.icnt_open_loop_batch_stats())
        rec["kernel"] = dict(mod.icnt_net_kernel_info())
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
    ap.add_argument("--out", default="icnt_capture_record.json")
    ap.add_argument("--cols", type=int, default=20000, help="pathfinder columns")
    ap.add_argument("--rows", type=int, default=20, help="pathfinder rows")
    ap.add_argument("--networks", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gpu-timeout", type=int, default=540, help="seconds the GPU step may take")
    ap.add_argument("--parent-so", help="the parent commit's native module: time its capture-off run too")
    ap.add_argument("--only-off", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tmp", help=argparse.SUPPRESS)
    ap.add_argument("--worker", choices=("cpu", "gpu"), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        return worker(a)
    recs = {}
    with tempfile.TemporaryDirectory(prefix="icnt_cap_") as tmp:
        common = ["--cols", str(a.cols), "--rows", str(a.rows), "--networks", str(a.networks), "--repeats",
                  str(a.repeats), "--tmp", tmp]
        steps = [("gpu", "gpu", None), ("cpu", "cpu", None)]
        if a.parent_so:
            steps += [("gpu_parent", "gpu", a.parent_so), ("cpu_parent", "cpu", a.parent_so)]
        for name, eng, so in steps:
            out = os.path.join(tmp, name + ".pkl")
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", eng, "--out", out] + common
            env = dict(os.environ)
            if so:
                cmd.append("--only-off")
                env["ASIM_NATIVE_SO"] = os.path.abspath(so)
            if eng == "gpu":  # the GPU step under its own time limit
                cmd = ["timeout", "-k", "10", str(a.gpu_timeout)] + cmd
            print("+", " ".join(cmd), flush=True)
            rc = subprocess.run(cmd, cwd=ROOT, env=env).returncode
            if rc != 0:
                print(f"{name} step failed (exit status {rc}): stopping", file=sys.stderr)
                return rc or 1
            with open(out, "rb") as f:
                recs[name] = pickle.load(f)
    cpu, gpu = recs["cpu"], recs["gpu"]
    files_equal = cpu["file"] == gpu["file"]
    sweep_equal = same(cpu["sweep"], gpu["sweep"])
    rec = {
        "simulation": {"machine": "QV100, 16 clusters, 8 memory channels, 8x8 mesh, router model",
                       "application": f"pathfinder {a.cols} x {a.rows}", "cycles": cpu["cycles"],
                       "request_packets": cpu["request_packets"], "reply_packets": cpu["reply_packets"],
                       "capture_bytes": len(cpu["file"])},
        "repeats": a.repeats,
        "capture": {e: {"off_seconds": r["off_seconds"], "on_seconds": r["on_seconds"],
                        "on_over_off": min(r["on_seconds"]) / min(r["off_seconds"]),
                        "off_spread_seconds": max(r["off_seconds"]) - min(r["off_seconds"]),
                        "same_cycles": r["same_cycles"]} for e, r in recs.items() if not e.endswith("_parent")},
        "gpu_file_equals_cpu_file": files_equal,
        "sweep": {"networks": cpu["networks"], "packets": cpu["request_packets"],
                  "cpu_seconds": cpu["sweep_seconds"], "gpu_seconds": gpu["sweep_seconds"],
                  "cpu_over_gpu": min(cpu["sweep_seconds"]) / min(gpu["sweep_seconds"]),
                  "gpu_results_equal_cpu": sweep_equal, "batch": gpu["batch"], "kernel": gpu["kernel"]},
    }
    for e in ("gpu", "cpu"):
        par = recs.get(e + "_parent")
        if not par:
            continue
        c, off, poff = rec["capture"][e], recs[e]["off_seconds"], par["off_seconds"]
        spread = max(max(off) - min(off), max(poff) - min(poff))
        c.update(parent_off_seconds=poff, off_over_parent=min(off) / min(poff), spread_seconds=spread,
                 off_equals_parent_within_spread=abs(min(off) - min(poff)) <= spread,
                 same_cycles_as_parent=par["cycles"] == recs[e]["cycles"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"capture": rec["capture"], "gpu_file_equals_cpu_file": files_equal,
                      "sweep": {k: v for k, v in rec["sweep"].items() if k != "networks"}}))
    return 0 if files_equal and sweep_equal else 1


if __name__ == "__main__":
    sys.exit(main())
