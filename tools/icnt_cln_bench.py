#!/usr/bin/env python3
"""One captured request list, closed loop, on a networks x windows grid: the
host path against the GPU kernel.

The list is the capture of a small cycle simulation made here with the CPU
engine (QV100 cut to 16 clusters and 16 L2 sub-partitions on an 8x8 mesh;
``--ctas`` single-warp CTAs, 16 line loads and 4 line stores each), turned
into requests with reply sizes by ``capture.request_list``.  The grid is eight
64-node networks (8x8 meshes of three flit sizes and VC counts, a torus, a
2-stage butterfly) x M in {1, 2, 4, 8, 16, unlimited}.  Two forms of the same
work:

  cpu  ``icnt_closed_loop_networks(engine="cpu")``: one core, one (network,
       window) pass after the other (rt_simulate_closed)
  gpu  ``engine="gpu"``: one launch per chunk, one wavefront per (network,
       window) (csrc/engine/icnt_cln_sweep.hip)

Every form runs once untimed, then ``--repeats`` times timed.  The GPU form
runs in one child process under ``timeout -k 10``, the host form in another;
any failure stops the script.  The record (JSON) holds every time, whether
all results are equal (every array, the state image, every summary), the
batch-time table, how the batch was packed (chunks, LDS) and the registers,
scratch and LDS of the five sweep kernels.

    python tools/icnt_cln_bench.py --out profiles/icnt_closed_replay/record.json
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

WINDOWS = (1, 2, 4, 8, 16, 0)
MESH = dict(k=8, n=2, topology="mesh")
NETWORKS = (
    ("mesh8x8 40B 1vc", dict(MESH)),
    ("mesh8x8 32B 2vc", dict(MESH, flit_size=32, num_vcs=2)),
    ("mesh8x8 16B 2vc", dict(MESH, flit_size=16, num_vcs=2)),
    ("mesh8x8 16B 2vc buf 8", dict(MESH, flit_size=16, num_vcs=2, vc_buf_size=8)),
    ("mesh8x8 32B 2vc speedup 2", dict(MESH, flit_size=32, num_vcs=2, internal_speedup="2.0")),
    ("mesh8x8 32B 2vc max_size", dict(MESH, flit_size=32, num_vcs=2, sw_allocator="max_size")),
    ("torus8x8 32B 2vc", dict(k=8, n=2, topology="torus", flit_size=32, num_vcs=2)),
    ("fly8x8 32B 2vc", dict(k=8, n=2, topology="fly", flit_size=32, num_vcs=2)),
)


def networks():
    from accel_sim_framework_distributed_amd.models import presets
    return [presets.render_icnt(presets.icnt_params(**kw)) for _, kw in NETWORKS]


def make_capture(tmp: str, ctas: int) -> str:
    """The capture file of the small machine's run on the CPU engine."""
    from accel_sim_framework_distributed_amd import _native
    from accel_sim_framework_distributed_amd.models import presets
    from accel_sim_framework_distributed_amd.tracegen import rodinia
    from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder
    k = KernelBuilder("_Z5mixedPf", (ctas, 1, 1), (32, 1, 1), nregs=32)
    for i in range(16):
        k.op("LDG.E", [8 + i], [2], base=0x7000_0000 + k.g.cta * 0x100000 + i * 128, stride=4)
    for i in range(16):
        k.op("FADD", [5], [8 + i, 5])
    for i in range(4):
        k.op("STG.E", [], [2, 5], base=0x7800_0000 + k.g.cta * 0x100000 + i * 128, stride=4)
    k.op("EXIT")
    kl = rodinia.write_app(os.path.join(tmp, "mixed"), [k.build()], memcpy=False)
    icnt = os.path.join(tmp, "capture.icnt")
    with open(icnt, "w") as f:
        f.write(presets.render_icnt(presets.icnt_params(**MESH)))
    args = presets.args_for("QV100", {"-gpgpu_n_clusters": "16", "-gpgpu_n_mem": "8", "-network_mode": "1",
                                      "-inter_config_file": icnt})
    path = os.path.join(tmp, "mixed.icap")
    s = _native.load().Simulator(args + ["-icnt_link_contention", "2", "-gpgpu_perf_sim_memcpy", "0", "-icnt_capture", path,
                                         "-sim_engine", "cpu", "-trace", kl], False)
    if s.run() != 0 or s.deadlock:
        raise RuntimeError("the capturing simulation failed")
    return path


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
    from accel_sim_framework_distributed_amd.icnt import capture
    mod = _native.load()
    rl = capture.request_list(capture.load(a.capture), timing=a.timing)
    lst = (rl.src, rl.dst, rl.req_bytes, rl.reply_bytes, rl.tcreate)
    texts = networks()
    rec = {"requests": len(rl), "units": len(texts) * len(WINDOWS)}

    def run(engine):
        return mod.icnt_closed_loop_networks(lst, texts, list(WINDOWS), reply_delay=a.reply_delay, engine=engine,
                                             arrivals=True, mem_budget_mb=a.mem_budget_mb, nodes=rl.nodes)
    if a.worker == "cpu":
        rec["results"], rec["cpu_seconds"] = timed(lambda: run("cpu"), a.repeats)
    else:
        if not mod.gpu_available():
            print("no usable HIP device", file=sys.stderr)
            return 2
        rec["results"], rec["gpu_seconds"] = timed(lambda: run("gpu"), a.repeats)
        rec["batch"] = dict(mod.icnt_open_loop_batch_stats())
        rec["lds_bytes"] = int(mod.icnt_closed_loop_networks_lds_bytes(texts))
        rec["kernels"] = {"icnt_cln_kernel": dict(mod.icnt_cln_kernel_info()),
                          "icnt_cl_kernel": dict(mod.icnt_cl_kernel_info()),
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
    ap.add_argument("--out", default="icnt_cln_record.json")
    ap.add_argument("--ctas", type=int, default=80, help="single-warp CTAs of the captured kernel (20 requests each)")
    ap.add_argument("--timing", choices=("captured", "batch"), default="captured")
    ap.add_argument("--reply-delay", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mem-budget-mb", type=int, default=0)
    ap.add_argument("--gpu-timeout", type=int, default=300, help="seconds the GPU step may take")
    ap.add_argument("--worker", choices=("cpu", "gpu"), help=argparse.SUPPRESS)
    ap.add_argument("--capture", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        return worker(a)
    recs = {}
    with tempfile.TemporaryDirectory(prefix="icnt_cln_") as tmp:
        cap = make_capture(tmp, a.ctas)
        common = ["--capture", cap, "--timing", a.timing, "--reply-delay", str(a.reply_delay), "--repeats", str(a.repeats),
                  "--mem-budget-mb", str(a.mem_budget_mb)]
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
    table = {}
    for ni, (name, _) in enumerate(NETWORKS):
        for wi, m in enumerate(WINDOWS):
            r = res[ni * len(WINDOWS) + wi]
            table.setdefault(name, {})[str(m)] = {
                "batch_time": int(r["batch_time"]), "round_trip_latency": r["round_trip_latency"],
                "issue_stall": r["issue_stall"], "avg_outstanding": r["avg_outstanding"],
                "request_flits": int(r["request_flits"]), "reply_flits": int(r["reply_flits"])}
    rec = {
        "grid": {"list": f"capture of {a.ctas} CTAs on the small machine (8x8 mesh), {a.timing} timing",
                 "requests": cpu["requests"], "networks": [n for n, _ in NETWORKS], "windows": list(WINDOWS),
                 "reply_delay": a.reply_delay, "units": cpu["units"],
                 "switch_passes": sum(int(r["activity"]["switch_passes"]) for r in res),
                 "deadlocked": sum(int(r["deadlocked"]) for r in res)},
        "repeats": a.repeats, "cpu_seconds": cpu["cpu_seconds"], "gpu_seconds": gpu["gpu_seconds"],
        "cpu_over_gpu": min(cpu["cpu_seconds"]) / min(gpu["gpu_seconds"]),
        "gpu_results_equal_cpu": equal, "batch": gpu["batch"], "lds_bytes": gpu["lds_bytes"],
        "kernels": gpu["kernels"], "table": table,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k not in ("grid", "table")}))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
