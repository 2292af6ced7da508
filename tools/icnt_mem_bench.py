#!/usr/bin/env python3
"""The memory endpoint of the closed-loop replay: what it costs when it is off,
what it costs when it is on, and the batch-time curve it is for.

The grid and the list are those of ``tools/icnt_cln_bench.py``: the capture of
a small cycle simulation (``--ctas`` single-warp CTAs on the small machine's
8x8 mesh) on eight 64-node networks x M in {1, 2, 4, 8, 16, unlimited}, 48
units.  Three measurements:

  off    the grid without memory points, on ``gpu`` and on ``cpu``.  With
         ``--baseline-root DIR`` (another checkout of this project with its
         native module built, for example the parent commit) the same call
         runs A/B/A/B: this tree, the baseline, this tree, the baseline.  The
         spread between two runs of one tree is the noise; the difference
         between the trees is reported against it.
  on     the same grid under one memory point (``--occupancy``, the call's
         reply delay as the latency): as many units, the model on.
  curve  batch time against occupancy on the host, for a synthetic list on
         one 8x8 mesh whose 16 memory nodes are placed in two ways (the two
         bottom rows; every fourth node) and loaded in two ways (uniformly;
         half of the requests to two of them).  No GPU.

Every timed step runs once untimed, then ``--repeats`` times.  Every GPU step
is a child process of its own under ``timeout -k 10``; any failure stops the
script.  The record (JSON) holds every time, whether gpu equals cpu in every
returned word, and the registers, scratch and LDS of the five sweep kernels.

    python tools/icnt_mem_bench.py --out profiles/icnt_mem_endpoint/record.json
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCCUPANCIES = (0, 1, 2, 4, 8, 16, 32)


def worker(a) -> int:
    """One tree, one engine: the grid with the model off and (this tree only) on."""
    root = os.path.abspath(a.root or ROOT)
    sys.path.insert(0, root)
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    if a.worker == "gpu":
        import torch  # bind torch's HIP runtime first  # noqa: F401
    from accel_sim_framework_distributed_amd import _native  # (the tree's package, before the grid's module adds its own root)
    from accel_sim_framework_distributed_amd.icnt import capture
    from accel_sim_framework_distributed_amd.models import presets  # noqa: F401
    sys.path.append(os.path.join(ROOT, "tools"))
    import icnt_cln_bench as cln
    mod = _native.load()
    if os.path.dirname(os.path.dirname(os.path.abspath(mod.__file__))) != root:
        print(f"the native module is not {root}'s: {mod.__file__}", file=sys.stderr)
        return 2
    if a.worker == "gpu" and not mod.gpu_available():
        print("no usable HIP device", file=sys.stderr)
        return 2
    rl = capture.request_list(capture.load(a.capture), timing=a.timing)
    lst = (rl.src, rl.dst, rl.req_bytes, rl.reply_bytes, rl.tcreate)
    texts = cln.networks()

    def run(**kw):
        return mod.icnt_closed_loop_networks(lst, texts, list(cln.WINDOWS), reply_delay=a.reply_delay, engine=a.worker,
                                             arrivals=True, mem_budget_mb=a.mem_budget_mb, nodes=rl.nodes, **kw)
    rec = {"requests": len(rl), "units": len(texts) * len(cln.WINDOWS)}
    rec["off_results"], rec["off_seconds"] = cln.timed(run, a.repeats)
    if a.model_on:
        rec["on_results"], rec["on_seconds"] = cln.timed(lambda: run(mem_points=[(a.occupancy, a.reply_delay)]), a.repeats)
    if a.worker == "gpu":
        rec["batch"] = dict(mod.icnt_open_loop_batch_stats())
        rec["kernels"] = {"icnt_cln_kernel": dict(mod.icnt_cln_kernel_info()),
                          "icnt_cl_kernel": dict(mod.icnt_cl_kernel_info()),
                          "icnt_sweep_kernel": dict(mod.icnt_sweep_kernel_info()),
                          "icnt_rr_kernel": dict(mod.icnt_rr_kernel_info()),
                          "icnt_net_kernel": dict(mod.icnt_net_kernel_info())}
    with open(a.out, "wb") as f:
        pickle.dump(rec, f)
    return 0


def curve(requests_per_node: int, window: int, latency: int) -> dict:
    """Batch time against occupancy on one 8x8 mesh: 48 issuers, 16 memory
    nodes placed and loaded in two ways each.  Host engine."""
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import icnt_cln_bench as cln
    from accel_sim_framework_distributed_amd import _native
    from accel_sim_framework_distributed_amd.models import presets
    mod = _native.load()
    text = presets.render_icnt(presets.icnt_params(**dict(cln.MESH, flit_size=32, num_vcs=2)))
    places = {"two bottom rows": list(range(48, 64)), "every fourth node": list(range(3, 64, 4))}
    loads = {"uniform": np.full(16, 1 / 16), "half to two nodes": np.array([0.25, 0.25] + [0.5 / 14] * 14)}
    out = {}
    for pname, mem in places.items():
        issuers = np.array([n for n in range(64) if n not in mem], np.uint32)
        for lname, p in loads.items():
            rng = np.random.default_rng(1)  # the same draws for both placements
            n = requests_per_node * len(issuers)
            src = np.tile(issuers, requests_per_node)
            dst = np.array(mem, np.uint32)[rng.choice(16, n, p=p)]
            wr = rng.random(n) < 0.25
            qb = np.where(wr, 136, 8).astype(np.uint32)
            pb = np.where(wr, 8, 136).astype(np.uint32)
            res = mod.icnt_closed_loop_networks((src, dst, qb, pb, np.zeros(n, np.uint64)), [text], [window],
                                                mem_points=[(o, latency) for o in OCCUPANCIES], nodes=64)
            if any(r["deadlocked"] for r in res):
                raise RuntimeError("a point of the curve deadlocked")
            out[f"{pname}, {lname}"] = {str(o): {"batch_time": int(r["batch_time"]), "mem_wait": r["mem_wait"],
                                                 "mem_utilisation": r["mem_utilisation"],
                                                 "max_mem_utilisation": r["max_mem_utilisation"]}
                                        for o, r in zip(OCCUPANCIES, res)}
    return {"network": "mesh8x8 32B 2vc", "requests": 48 * requests_per_node, "window": window, "latency": latency,
            "occupancies": list(OCCUPANCIES), "batch": out}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="icnt_mem_record.json")
    ap.add_argument("--ctas", type=int, default=80, help="single-warp CTAs of the captured kernel (20 requests each)")
    ap.add_argument("--timing", choices=("captured", "batch"), default="captured")
    ap.add_argument("--reply-delay", type=int, default=20)
    ap.add_argument("--occupancy", type=int, default=4, help="the memory point of the model-on grid")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mem-budget-mb", type=int, default=0)
    ap.add_argument("--gpu-timeout", type=int, default=300, help="seconds one GPU step may take")
    ap.add_argument("--baseline-root", help="another checkout with its native module built: the model-off grid A/B/A/B")
    ap.add_argument("--engines", default="gpu,cpu", help="comma list of gpu, cpu")
    ap.add_argument("--curve-requests", type=int, default=40, help="requests per issuing node of the curve's list")
    ap.add_argument("--curve-window", type=int, default=8)
    ap.add_argument("--no-curve", action="store_true")
    ap.add_argument("--worker", choices=("cpu", "gpu"), help=argparse.SUPPRESS)
    ap.add_argument("--root", help=argparse.SUPPRESS)
    ap.add_argument("--model-on", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--capture", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        return worker(a)
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tools"))
    import icnt_cln_bench as cln
    engines = [e for e in a.engines.split(",") if e]
    trees = [("this", ROOT)] + ([("baseline", os.path.abspath(a.baseline_root))] if a.baseline_root else [])
    order = trees * 2 if a.baseline_root else trees  # A/B/A/B
    runs = {e: [] for e in engines}
    with tempfile.TemporaryDirectory(prefix="icnt_mem_") as tmp:
        cap = cln.make_capture(tmp, a.ctas)
        common = ["--capture", cap, "--timing", a.timing, "--reply-delay", str(a.reply_delay), "--repeats", str(a.repeats),
                  "--mem-budget-mb", str(a.mem_budget_mb), "--occupancy", str(a.occupancy)]
        for eng in engines:
            for k, (name, root) in enumerate(order):
                out = os.path.join(tmp, f"{eng}{k}.pkl")
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", eng, "--root", root, "--out", out] + common
                if name == "this" and k == 0:
                    cmd.append("--model-on")
                if eng == "gpu":  # every GPU step under its own time limit
                    cmd = ["timeout", "-k", "10", str(a.gpu_timeout)] + cmd
                print("+", " ".join(cmd), flush=True)
                rc = subprocess.run(cmd, cwd=root).returncode
                if rc != 0:
                    print(f"{eng} step {k} ({name}) failed (exit status {rc}): stopping", file=sys.stderr)
                    return rc or 1
                with open(out, "rb") as f:
                    runs[eng].append((name, pickle.load(f)))
    rec = {"grid": {"list": f"capture of {a.ctas} CTAs on the small machine (8x8 mesh), {a.timing} timing",
                    "networks": [n for n, _ in cln.NETWORKS], "windows": list(cln.WINDOWS), "reply_delay": a.reply_delay,
                    "model_on_point": [a.occupancy, a.reply_delay]},
           "repeats": a.repeats, "order": [n for n, _ in order], "engines": {}}
    ok = True
    first = {e: runs[e][0][1] for e in engines}
    for eng in engines:
        r0 = first[eng]
        rec["grid"].update(requests=r0["requests"], units=r0["units"],
                           deadlocked=sum(int(r["deadlocked"]) for r in r0["off_results"] + r0["on_results"]))
        e = {"off_seconds": [{"tree": n, "seconds": r["off_seconds"]} for n, r in runs[eng]], "on_seconds": r0["on_seconds"]}
        best = {}
        for n, r in runs[eng]:
            best.setdefault(n, []).append(min(r["off_seconds"]))
        e["off_best"] = best
        # noise: the spread between the runs of one tree; difference: between the trees' best runs
        e["noise_seconds"] = max(max(v) - min(v) for v in best.values())
        if "baseline" in best:
            e["off_this_minus_baseline_seconds"] = min(best["this"]) - min(best["baseline"])
            # the model off computes what the baseline computes (the baseline lacks the new fields)
            base = [r for n, r in runs[eng] if n == "baseline"][0]["off_results"]
            e["off_equals_baseline"] = all(cln.same(t[k], b[k]) for t, b in zip(r0["off_results"], base) for k in b)
            ok = ok and e["off_equals_baseline"]
        e["on_over_off"] = min(r0["on_seconds"]) / min(r0["off_seconds"])
        if eng == "gpu":
            e["batch"] = r0["batch"]
            rec["kernels"] = r0["kernels"]
            if "baseline" in best:
                rec["baseline_kernels"] = [r for n, r in runs[eng] if n == "baseline"][0]["kernels"]
        rec["engines"][eng] = e
    if len(engines) == 2:
        rec["gpu_results_equal_cpu"] = {k: cln.same(first["gpu"][k + "_results"], first["cpu"][k + "_results"])
                                        for k in ("off", "on")}
        ok = ok and all(rec["gpu_results_equal_cpu"].values())
    on = first[engines[-1]]["on_results"]
    off = first[engines[-1]]["off_results"]
    rec["on_table"] = {name: {str(m): {"batch_time_off": int(off[ni * len(cln.WINDOWS) + wi]["batch_time"]),
                                       "batch_time_on": int(on[ni * len(cln.WINDOWS) + wi]["batch_time"]),
                                       "mem_wait": on[ni * len(cln.WINDOWS) + wi]["mem_wait"],
                                       "max_mem_utilisation": on[ni * len(cln.WINDOWS) + wi]["max_mem_utilisation"]}
                              for wi, m in enumerate(cln.WINDOWS)} for ni, (name, _) in enumerate(cln.NETWORKS)}
    if not a.no_curve:
        rec["curve"] = curve(a.curve_requests, a.curve_window, a.reply_delay)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k not in ("grid", "on_table", "curve")}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
