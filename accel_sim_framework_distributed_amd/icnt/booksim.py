"""Standalone network runs of the router model (the reference's intersim2
``booksim`` binary: ``intersim2/main.cpp`` + ``trafficmanager.cpp``).

Reads a Booksim ``.icnt`` file (topology, router pipeline, ``num_vcs``,
``vc_buf_size``, ``sw_allocator``, ``alloc_iters``, ``credit_delay``,
``internal_speedup``; the ``power_*`` per-event energies of the network
power estimate) and drives open-loop synthetic traffic through the
input-queued router model of ``csrc/model/icnt_router.h`` -- the same code
the simulator runs per epoch with ``-icnt_link_contention 2``.

    python -m accel_sim_framework_distributed_amd.icnt.booksim config.icnt \\
        --traffic uniform --rates 0.1,0.2,0.4,0.6 --packet-flits 1

prints Booksim-style ``Overall average latency`` / ``accepted rate`` lines
per injection rate (flits per node per cycle) and optionally a JSON curve.
``--traffic a,b`` and ``--seeds N`` widen the run to a pattern x rate x seed
grid, and ``--engine gpu`` sends that grid as one batch to the MI355X, one
wavefront per point (``cpu-par`` runs the same lane-parallel router pass on
the host; all engines give the same numbers, the default is ``cpu``).
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import Dict, List, Optional

from .. import _native


def run(icnt_text: str, rate: float, traffic: str = "uniform", packet_flits: int = 1, cycles: int = 5000,
        warmup: int = 1000, seed: int = 1) -> Dict[str, float]:
    return dict(_native.load().icnt_open_loop(icnt_text, traffic, rate, packet_flits, cycles, warmup, seed))


def sweep(icnt_text: str, rates: List[float], engine: str = "cpu", traffic="uniform", packet_flits: int = 1,
          cycles: int = 5000, warmup: int = 1000, seed: int = 1, seeds: Optional[List[int]] = None,
          mem_budget_mb: int = 0) -> List[Dict[str, float]]:
    """The grid traffic x rate x seed as ONE batch through `engine`: ``cpu``
    (the sequential router pass), ``cpu-par`` (the lane-parallel pass on the
    host) or ``gpu`` (one wavefront per point, csrc/engine/icnt_sweep.hip).
    `traffic` is a pattern or a list of patterns, `seeds` a list of seeds
    (default: `seed` alone).  One dict per point, in that order, each with its
    ``rate``; with several patterns or seeds also its ``traffic`` and ``seed``."""
    traffics = [traffic] if isinstance(traffic, str) else list(traffic)
    seed_list = [seed] if seeds is None else list(seeds)
    multi = len(traffics) > 1 or len(seed_list) > 1
    grid = [(t, r, s) for t in traffics for r in rates for s in seed_list]
    res = _native.load(prefer_torch_runtime=engine == "gpu").icnt_open_loop_batch(icnt_text, [(t, r, packet_flits, cycles, warmup, s) for t, r, s in grid],
                                              engine=engine, mem_budget_mb=mem_budget_mb)
    out = []
    for (t, r, s), d in zip(grid, res):
        d = dict(d)
        d["rate"] = r
        if multi:
            d["traffic"] = t
            d["seed"] = s
        out.append(d)
    return out


def _mean(points: List[Dict[str, float]]) -> Dict[str, float]:
    """The printed figures of one rate, averaged over its seeds (max latency:
    the largest; packet counts: summed)."""
    if len(points) == 1:
        return points[0]
    n = len(points)
    m = dict(points[0])
    for k in ("avg_latency", "zero_load_latency", "accepted", "offered", "drain_throughput", "power_w"):
        m[k] = sum(p[k] for p in points) / n
    m["max_latency"] = max(p["max_latency"] for p in points)
    m["energy_pj"] = {k: sum(p["energy_pj"][k] for p in points) / n for k in points[0]["energy_pj"]}
    for k in ("measured_packets", "packets", "deadlocked"):
        m[k] = sum(p[k] for p in points)
    return m


def saturation(curve: List[Dict[str, float]], factor: float = 3.0) -> float:
    """Highest offered rate whose latency stays within `factor` x zero load."""
    ok = [c["rate"] for c in curve if c["measured_packets"] and c["avg_latency"] <= factor * c["zero_load_latency"]]
    return max(ok) if ok else 0.0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("config", help="Booksim .icnt file")
    ap.add_argument("--traffic", default="uniform",
                    help="uniform, transpose, bitcomp, bitrev, shuffle, tornado, neighbor (comma list)")
    ap.add_argument("--rates", default="0.05,0.1,0.2,0.3,0.4,0.5,0.6,0.8,1.0",
                    help="offered load, flits per node per cycle (comma list)")
    ap.add_argument("--packet-flits", type=int, default=1)
    ap.add_argument("--cycles", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seeds", type=int, default=0,
                    help="run seeds 1..N and print their average per rate (the JSON keeps every point)")
    ap.add_argument("--engine", choices=("cpu", "cpu-par", "gpu"), default="cpu",
                    help="cpu: the sequential router pass; cpu-par: the lane-parallel pass on the host; "
                         "gpu: one wavefront per point, the whole grid in one batch")
    ap.add_argument("--mem-budget-mb", type=int, default=0,
                    help="gpu: device memory of one launch (default: half the free device memory)")
    ap.add_argument("--json", help="write the latency / throughput curve here")
    a = ap.parse_args(argv)
    text = open(a.config).read()
    traffics = [t for t in a.traffic.split(",") if t]
    seeds = list(range(1, a.seeds + 1)) if a.seeds > 0 else None
    curve = sweep(text, [float(x) for x in a.rates.split(",") if x], engine=a.engine,
                  traffic=traffics if len(traffics) > 1 else a.traffic, packet_flits=a.packet_flits, cycles=a.cycles,
                  warmup=a.warmup, seed=a.seed, seeds=seeds, mem_budget_mb=a.mem_budget_mb)
    per = len(seeds) if seeds else 1
    nrate = len(curve) // (per * len(traffics))
    for ti, traffic in enumerate(traffics):
        means = []
        for ri in range(nrate):
            lo = (ti * nrate + ri) * per
            means.append(_mean(curve[lo:lo + per]))
        for c in means:
            print(f"====== Traffic {traffic}, injection rate {c['rate']:.3f} ======")
            print(f"Overall average latency = {c['avg_latency']:.2f} (zero load {c['zero_load_latency']:.2f}, "
                  f"max {c['max_latency']:.0f})")
            print(f"Overall average accepted rate = {c['accepted']:.4f} (offered {c['offered']:.4f}; "
                  f"drain rate {c['drain_throughput']:.4f})")
            e = c["energy_pj"]
            print(f"Network power = {c['power_w']:.3f} W (energy pJ: buffer {e['buffer']:.3g}, crossbar {e['crossbar']:.3g}, "
                  f"link {e['link']:.3g}, allocator {e['allocator']:.3g}, leakage {e['leakage']:.3g})")
            print(f"Packets = {c['measured_packets']} measured of {c['packets']}"
                  + (f", {c['deadlocked']} deadlocked" if c["deadlocked"] else ""))
        print(f"Saturation (latency <= 3x zero load): {saturation(means):.3f} flits/node/cycle")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "traffic": a.traffic, "packet_flits": a.packet_flits, "curve": curve},
                      f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
