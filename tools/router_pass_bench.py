#!/usr/bin/env python3
"""A/B of the router model's epoch pass: -sim_router_pass serial against par,
alternated within one process, on the GPU engine and then on the CPU engine
(-icnt_link_contention 2 throughout).  Writes profiles/router_pass/record.json.

    python tools/router_pass_bench.py [--reps 3] [--out FILE] [--engines gpu,cpu]
        [--parent-modes FILE] [--bench-parent FILE ...] [--bench-tree FILE ...]
    python tools/router_pass_bench.py --modes-only     # gpu_engine_modes() as JSON

Workloads: the full QV100 preset (80 SMs, 32 channels, 112 engine blocks) on a
12 x 12 mesh with the spread hotspot kernel of tests/test_router_pass_par.py,
and two Rodinia-shaped applications (tracegen/rodinia.py) on the same machine.
Per engine and workload one untimed run of each mode (code objects, caches),
then serial / par / serial / par ...: the wall time of Simulator.run (it ends
in a device synchronise), router_pass_stats, and whether cycles, the link
statistics and the state image equal the first serial run's.  serial is the
code path of the commit before the option existed, so it is the baseline; the
spread of its repeats stands next to the ratio.

--modes-only with ASIM_NATIVE_SO pointing at another build of the module
prints that build's kernel resources; --parent-modes folds such a file into
the record.  --bench-parent / --bench-tree take `bench.py --engine gpu` result
lines (router model off) of the parent commit and of this tree for the
no-regression section: the margin is the parent's own run-to-run spread.
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAT_KEYS = ("Network_link_delayed_packets", "Network_link_wait_cycles", "Req_Network_injection_stall_cycles",
             "Reply_Network_injection_stall_cycles", "Network_router_deadlocked_packets")


def spread_hotspot(root):
    """80 one-warp CTAs, 16 loads each, every SM its own lines (spread over
    all sub-partitions)."""
    from accel_sim_framework_distributed_amd.tracegen import rodinia
    from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder
    k = KernelBuilder("_Z7hotspotPf", (80, 1, 1), (32, 1, 1), nregs=32)
    for i in range(16):
        k.op("LDG.E", [8 + i], [2], base=0x7000_0000 + k.g.cta * 0x100000 + i * 128, stride=4)
    for i in range(16):
        k.op("FADD", [5], [8 + i, 5])
    k.op("EXIT")
    return rodinia.write_app(os.path.join(root, "spread"), [k.build()], memcpy=False)


def workloads(root):
    from accel_sim_framework_distributed_amd.tracegen import rodinia
    return {
        "spread_hotspot": spread_hotspot(root),
        "bfs_4096": rodinia.write_app(os.path.join(root, "bfs"), rodinia.bfs(4096, levels=4)),
        "hotspot_128": rodinia.write_app(os.path.join(root, "hs"), rodinia.hotspot(128, 2, 2)),
    }


def one_run(mod, args, kl, engine, mode):
    s = mod.Simulator(args + ["-icnt_link_contention", "2", "-gpgpu_perf_sim_memcpy", "0", "-sim_router_pass", mode,
                              "-sim_engine", engine, "-trace", kl], False)
    t0 = time.perf_counter()
    rc = s.run()
    wall = time.perf_counter() - t0
    if rc != 0 or s.deadlock:
        raise RuntimeError(f"{engine} {mode}: simulation failed")
    out = s.output
    res = [s.tot_cycle] + [int(re.findall(rf"^{k} = (\d+)", out, re.M)[-1]) for k in STAT_KEYS]
    m = re.search(r"^engine_kernel_variant: (\S+) blocks=(\d+)$", out, re.M)
    return dict(mode=mode, wall_s=round(wall, 4), result=res, snapshot_sha256=hashlib.sha256(bytes(s.snapshot())).hexdigest(),
                router_pass=s.router_pass_stats(), variant=m.group(1) if m else "", blocks=int(m.group(2)) if m else 0)


def ab(mod, args, kl, engine, reps):
    warm = [one_run(mod, args, kl, engine, m) for m in ("serial", "par")]
    runs = []
    for _ in range(reps):
        for m in ("serial", "par"):
            runs.append(one_run(mod, args, kl, engine, m))
    base = runs[0]
    equal = all(r["result"] == base["result"] and r["snapshot_sha256"] == base["snapshot_sha256"] for r in warm + runs)
    ws = [r["wall_s"] for r in runs if r["mode"] == "serial"]
    wp = [r["wall_s"] for r in runs if r["mode"] == "par"]
    ms, mp = statistics.median(ws), statistics.median(wp)
    return dict(engine=engine, variant=base["variant"], blocks=base["blocks"], tot_cycle=base["result"][0],
                link_stats=dict(zip(STAT_KEYS, base["result"][1:])), snapshot_sha256=base["snapshot_sha256"],
                results_and_snapshots_equal=equal,
                router_pass=[r for r in runs if r["mode"] == "par"][0]["router_pass"],
                serial_wall_s=ws, par_wall_s=wp, serial_median_s=round(ms, 4), par_median_s=round(mp, 4),
                serial_spread=round((max(ws) - min(ws)) / ms, 4), par_spread=round((max(wp) - min(wp)) / mp, 4),
                par_over_serial=round(mp / ms, 4), warmup_wall_s=[r["wall_s"] for r in warm])


def bench_lines(paths):
    out = []
    for p in paths or []:
        with open(p) as f:
            for line in f:
                if line.startswith("{"):
                    d = json.loads(line)
                    out.append(dict(file=os.path.basename(p), value=d.get("value"), unit=d.get("unit"),
                                    ms_per_step=d.get("ms_per_step")))
    return out


def no_regression(parent, tree):
    p = [x["value"] for x in parent if x["value"]]
    t = [x["value"] for x in tree if x["value"]]
    d = dict(command="bench.py --engine gpu (router model off, default options)", parent=parent, tree=tree)
    if len(p) >= 2 and t:
        mp, mt = statistics.median(p), statistics.median(t)
        d.update(parent_median=mp, tree_median=mt, parent_spread=round((max(p) - min(p)) / mp, 4),
                 tree_over_parent=round(mt / mp, 4))
        # bench.py's value is a rate (higher is better): a regression is a
        # tree median below the parent's by more than the parent's own spread
        d["within_parent_spread"] = bool(mt >= mp * (1 - d["parent_spread"]))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engines", default="gpu,cpu")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "router_pass", "record.json"))
    ap.add_argument("--modes-only", action="store_true")
    ap.add_argument("--parent-modes", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    ap.add_argument("--bench-tree", nargs="*", default=None)
    a = ap.parse_args()
    engines = [e for e in a.engines.split(",") if e]
    if "gpu" in engines or a.modes_only:
        import torch  # bind torch's HIP runtime first
        if not torch.cuda.is_available():
            sys.exit("router_pass_bench: no GPU visible (a timing without one says nothing)")
    from accel_sim_framework_distributed_amd import _native
    from accel_sim_framework_distributed_amd.models import presets
    mod = _native.load(prefer_torch_runtime=True)
    if a.modes_only:
        print(json.dumps(mod.gpu_engine_modes()))
        return
    root = tempfile.mkdtemp(prefix="router_pass_bench_")
    icnt = os.path.join(root, "mesh12.icnt")
    with open(icnt, "w") as f:
        f.write(presets.render_icnt(presets.icnt_params(k=12, n=2, topology="mesh", num_vcs=2)))
    args = presets.args_for("QV100", {"-network_mode": "1", "-inter_config_file": icnt})
    rec = dict(tool="tools/router_pass_bench.py", reps=a.reps, config="QV100 preset, mesh k=12 n=2 num_vcs=2, "
               "-icnt_link_contention 2", env={k: v for k, v in os.environ.items() if k.startswith("ASIM_GPU")},
               workloads={})
    if "gpu" in engines:
        rec["device"] = torch.cuda.get_device_name(0)
        rec["gpu_engine_modes"] = mod.gpu_engine_modes()
    if a.parent_modes:
        with open(a.parent_modes) as f:
            rec["gpu_engine_modes_parent"] = json.load(f)
    for name, kl in workloads(root).items():
        rec["workloads"][name] = {}
        for eng in engines:
            r = ab(mod, args, kl, eng, a.reps)
            rec["workloads"][name][eng] = r
            print(f"{name:16s} {eng} serial {r['serial_median_s']:.4f} s (spread {r['serial_spread']:.1%}) "
                  f"par {r['par_median_s']:.4f} s  par/serial {r['par_over_serial']:.3f}  equal "
                  f"{r['results_and_snapshots_equal']}  {r['router_pass']}", flush=True)
    if a.bench_parent is not None or a.bench_tree is not None:
        rec["no_regression"] = no_regression(bench_lines(a.bench_parent), bench_lines(a.bench_tree))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    bad = [n for n, w in rec["workloads"].items() for e in w.values() if not e["results_and_snapshots_equal"]]
    if bad:
        sys.exit("router_pass_bench: results differ between the modes: " + ", ".join(bad))


if __name__ == "__main__":
    main()
