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

``--request-reply`` runs the traffic the two subnets of a GPU's network
carry: reads and writes on the request subnet, and for each one, generated at
its destination when it arrives, a reply of the other size on the reply
subnet (``read_request_size`` .. ``write_reply_size`` and ``write_fraction``
from the ``.icnt`` file, Booksim's names; ``--mem-nodes M`` makes the last M
nodes the memory partitions every request goes to).  ``--replay FILE`` runs a
packet list of the user's (an ``.npz`` with ``src``, ``dst``, ``flits``,
``tinj``), for example one dumped from a cycle simulation; FILE may also be
the capture file itself (``-icnt_capture``, icnt/capture.py; ``--subnet``
picks the subnet), and ``--networks a.icnt,b.icnt,...`` replays the one list
on every network of the list, each with its own flit counts from the packets'
bytes (``--engine gpu``: one wavefront per network in one launch).

``--closed-loop`` runs request-reply traffic with bounded windows (Booksim's
``sim_type = batch``, batchtrafficmanager.cpp): a node keeps at most
``--max-outstanding M`` requests in flight (a comma list sweeps M; 0:
unlimited) and issues the next one when a reply has come back, so the reply
subnet's arrivals feed the request subnet's injections and both advance on
one clock (one router pass over the doubled network,
csrc/model/icnt_closed.h).  ``--batch-size B``: every issuing node creates B
requests at cycle 0 and the figure is the batch time, the last reply's
arrival; without it the points are ``--request-reply`` rate points behind the
window.  The ``.icnt`` keys ``max_outstanding_requests`` and ``batch_size``
are the defaults, the latter when ``sim_type = batch``.  Unlike Booksim a
node may issue several requests in one cycle, and a reply leaves from the
reply subnet's terminal instead of taking its node's injection slot.

``--closed-loop --replay FILE [--networks a.icnt,b.icnt,...]`` runs the
requests of a capture file (or of an ``.npz`` with ``src``, ``dst``,
``bytes``, ``reply_bytes``, ``tinj``) closed loop on every network of the
list under every window of ``--max-outstanding``: each reply is created by
its request's delivery on that network, with the size the capture recorded
(icnt/capture.py ``request_list`` pairs them per cluster, sub-partition and
kind), so the batch time is the time the application's own requests take on
that network when a node may keep M in flight.  ``--timing batch`` makes
every request ready at cycle 0, in captured order, in place of the captured
creation times.  ``--engine gpu``: one wavefront per (network, window) in one
launch (csrc/engine/icnt_cln_sweep.hip).
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


RR_SIZES = ("read_request_size", "read_reply_size", "write_request_size", "write_reply_size")


def replay(icnt_text: str, src, dst, flits, tinj, engine: str = "cpu", cycles: int = 0, warmup: int = 0,
           arrivals: bool = False, mem_budget_mb: int = 0) -> Dict[str, float]:
    """One packet list through the network (one subnet): packet i goes from
    ``src[i]`` to ``dst[i]`` with ``flits[i]`` flits, created at cycle
    ``tinj[i]``; any order.  The summary's window is [warmup, cycles),
    ``cycles=0``: the last injection + 1."""
    mod = _native.load(prefer_torch_runtime=engine == "gpu")
    return dict(mod.icnt_replay_batch(icnt_text, [(src, dst, flits, tinj)], engine=engine, arrivals=arrivals,
                                      mem_budget_mb=mem_budget_mb, cycles=cycles, warmup=warmup)[0])


def replay_networks(src, dst, nbytes, tinj, icnt_texts: List[str], engine: str = "cpu", cycles: int = 0,
                    warmup: int = 0, arrivals: bool = False, mem_budget_mb: int = 0, lds: bool = True,
                    nodes: int = 0) -> List[Dict[str, float]]:
    """One packet list through many networks, one result per ``.icnt`` text:
    packet i weighs ``nbytes[i]`` bytes and every network derives its own flit
    count from that.  ``engine="gpu"`` runs one wavefront per network, as many
    networks per launch as the memory budget takes
    (csrc/engine/icnt_net_sweep.hip).  `nodes`: the list's node count; a
    network with another one is refused (0: not checked)."""
    mod = _native.load(prefer_torch_runtime=engine == "gpu")
    return [dict(d) for d in mod.icnt_replay_networks((src, dst, nbytes, tinj), list(icnt_texts), engine=engine,
                                                      arrivals=arrivals, mem_budget_mb=mem_budget_mb, lds=lds,
                                                      cycles=cycles, warmup=warmup, nodes=nodes)]


def _replay_lists(path: str, subnet: str):
    """[(label, src, dst, bytes or None, flits, tinj, nodes)] of a --replay
    file: the chosen subnets of a capture file, or the one list of an .npz."""
    import numpy as np
    from . import capture
    if capture.is_capture(path):
        cap = capture.load(path)
        names = capture.SUBNETS if subnet == "both" else (subnet,)
        return [(n, s.src, s.dst, s.bytes, s.flits, s.tinj, cap.nodes) for n in names for s in (cap.subnet(n),)]
    with np.load(path) as z:
        return [(None, z["src"], z["dst"], z["bytes"] if "bytes" in z else None, z["flits"], z["tinj"],
                 int(z["nodes"]) if "nodes" in z else 0)]


def _main_replay(a) -> int:
    lists = _replay_lists(a.replay, a.subnet)
    nets = [n for n in (a.networks or "").split(",") if n]
    out = []
    for label, src, dst, nbytes, flits, tinj, nodes in lists:
        what = f"{a.replay}" + (f" ({label} subnet)" if label else "")
        if nets or (label and a.config):
            # a capture file, or several networks: every network's own flits from the bytes
            if nbytes is None:
                print("--networks needs a packet list with bytes (a capture file, or an .npz with a bytes array)",
                      file=sys.stderr)
                return 2
            files = nets or [a.config]
            res = replay_networks(src, dst, nbytes, tinj, [open(f).read() for f in files], engine=a.engine,
                                  cycles=a.cycles or 0, warmup=a.warmup or 0, mem_budget_mb=a.mem_budget_mb,
                                  nodes=nodes)
            for f, c in zip(files, res):
                print(f"====== Replay of {what} on {f} ======")
                _print_open_loop(c)
                out.append({"config": f, "replay": a.replay, "subnet": label, "result": c})
        else:
            c = replay(open(a.config).read(), src, dst, flits, tinj, engine=a.engine, cycles=a.cycles or 0,
                       warmup=a.warmup or 0, mem_budget_mb=a.mem_budget_mb)
            print(f"====== Replay of {what} ======")
            _print_open_loop(c)
            out.append({"config": a.config, "replay": a.replay, "result": c})
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out[0] if len(out) == 1 and not nets else out, f, indent=1)
    return 0


def request_reply_sweep(icnt_text: str, rates: List[float], engine: str = "cpu", traffic="uniform",
                        cycles: int = 5000, warmup: int = 1000, seed: int = 1, seeds: Optional[List[int]] = None,
                        write_fraction: Optional[float] = None, reply_delay: int = 0, mem_nodes: int = 0,
                        read_request_size: Optional[int] = None, read_reply_size: Optional[int] = None,
                        write_request_size: Optional[int] = None, write_reply_size: Optional[int] = None,
                        mem_budget_mb: int = 0, arrivals: bool = False) -> List[Dict]:
    """The grid traffic x rate x seed of request-reply points as ONE batch
    through `engine`, like :func:`sweep`.  Reads and writes travel on the
    request subnet; each one's arrival creates, `reply_delay` cycles later, a
    reply at its destination, and the replies enter the reply subnet -- a
    second, independent network of the same file -- in (time, request) order.
    Unlike Booksim's single-queue ``_IssuePacket``, a pending reply does not
    hold back its node's requests.  `rate` is flits per node per cycle over
    both subnets.  The four packet sizes (flits) and `write_fraction` come
    from the ``.icnt`` keys of the same names when the file has them and the
    argument is None (else 1 flit and 0.5).  ``mem_nodes=M``: nodes 0..N-M-1
    issue, to the uniformly drawn nodes N-M..N-1."""
    mod = _native.load(prefer_torch_runtime=engine == "gpu")
    kv = mod.parse_booksim_config(icnt_text)
    given = dict(zip(RR_SIZES, (read_request_size, read_reply_size, write_request_size, write_reply_size)))
    common = {k: int(v if v is not None else float(kv.get(k, 1))) for k, v in given.items()}
    common["write_fraction"] = float(write_fraction if write_fraction is not None else kv.get("write_fraction", 0.5))
    common.update(reply_delay=int(reply_delay), mem_nodes=int(mem_nodes), cycles=int(cycles), warmup=int(warmup))
    traffics = [traffic] if isinstance(traffic, str) else list(traffic)
    seed_list = [seed] if seeds is None else list(seeds)
    multi = len(traffics) > 1 or len(seed_list) > 1
    grid = [(t, r, s) for t in traffics for r in rates for s in seed_list]
    res = mod.icnt_request_reply_batch(icnt_text, [dict(common, traffic=t, rate=r, seed=s) for t, r, s in grid],
                                       engine=engine, arrivals=arrivals, mem_budget_mb=mem_budget_mb)
    out = []
    for (t, r, s), d in zip(grid, res):
        d = dict(d)
        d["rate"] = r
        if multi:
            d["traffic"] = t
            d["seed"] = s
        out.append(d)
    return out


def closed_loop_sweep(icnt_text: str, max_outstanding: Optional[List[int]] = None, batch_size: Optional[int] = None,
                      rates: Optional[List[float]] = None, engine: str = "cpu", traffic="uniform",
                      cycles: int = 5000, warmup: int = 1000, seed: int = 1, seeds: Optional[List[int]] = None,
                      write_fraction: Optional[float] = None, reply_delay: int = 0, mem_nodes: int = 0,
                      read_request_size: Optional[int] = None, read_reply_size: Optional[int] = None,
                      write_request_size: Optional[int] = None, write_reply_size: Optional[int] = None,
                      mem_budget_mb: int = 0, arrivals: bool = False, lds: bool = True,
                      read_occupancy: Optional[int] = None, write_occupancy: Optional[int] = None,
                      write_reply_delay: Optional[int] = None) -> List[Dict]:
    """Closed-loop request-reply points with bounded windows as ONE batch
    through `engine` (``gpu``: one wavefront per point,
    csrc/engine/icnt_cl_sweep.hip).  A node keeps at most M requests in flight
    (`max_outstanding`, a list; 0: unlimited) and issues the next one when a
    reply has come back.  With `rates` the grid is traffic x rate x M x seed
    of rate points, each the request list of the :func:`request_reply_sweep`
    point behind the window; otherwise traffic x M x seed of batch points,
    every issuing node creating `batch_size` requests at cycle 0.  Defaults
    from the ``.icnt`` keys: ``max_outstanding_requests`` for M, ``batch_size``
    when ``sim_type = batch``, the four packet sizes and ``write_fraction``.

    `read_occupancy`, `write_occupancy` and `write_reply_delay` turn the
    memory endpoint on: a memory node is one server that a request holds for
    its kind's occupancy (cycles), first come first served, with `reply_delay`
    (a write: `write_reply_delay`) cycles of pipelined latency behind it, and
    replies leave a node in the order their requests arrived.  The results
    carry ``mem_time``, ``mem_wait``, ``mem_hold`` and ``mem_utilisation``.

    Without `arrivals` the result is the curve: one dict per (traffic, rate,
    M) with the figures averaged over the seeds (``batch_time``,
    ``round_trip_latency``, ``issue_stall``, ...; maxima: the largest;
    ``deadlocked``: summed), ``seeds`` and, per seed, ``batch_times``.  With
    `arrivals` it is one dict per point, in grid order, with its ``traffic``,
    ``rate``, ``max_outstanding`` and ``seed`` and every array."""
    mod = _native.load(prefer_torch_runtime=engine == "gpu")
    kv = mod.parse_booksim_config(icnt_text)
    given = dict(zip(RR_SIZES, (read_request_size, read_reply_size, write_request_size, write_reply_size)))
    common = {k: int(v if v is not None else float(kv.get(k, 1))) for k, v in given.items()}
    common["write_fraction"] = float(write_fraction if write_fraction is not None else kv.get("write_fraction", 0.5))
    common.update(reply_delay=int(reply_delay), mem_nodes=int(mem_nodes))
    for k, v in (("read_occupancy", read_occupancy), ("write_occupancy", write_occupancy),
                 ("write_reply_delay", write_reply_delay)):
        if v is not None:
            common[k] = int(v)
    if "batch_count" in kv:
        common["batch_count"] = int(float(kv["batch_count"]))
    if max_outstanding is None:
        max_outstanding = [int(float(kv.get("max_outstanding_requests", 0)))]
    if rates is None and batch_size is None:
        if kv.get("sim_type") != "batch":
            raise ValueError("closed_loop_sweep needs rates, a batch_size, or sim_type = batch in the .icnt file")
        batch_size = int(float(kv.get("batch_size", 1)))
    if rates is None:
        common["batch_size"] = int(batch_size)
        rate_list = [None]
    else:
        common.update(cycles=int(cycles), warmup=int(warmup))
        rate_list = list(rates)
    traffics = [traffic] if isinstance(traffic, str) else list(traffic)
    seed_list = [seed] if seeds is None else list(seeds)
    grid = [(t, r, int(m), s) for t in traffics for r in rate_list for m in max_outstanding for s in seed_list]
    pts = [dict(common, traffic=t, max_outstanding=m, seed=s, **({} if r is None else {"rate": r})) for t, r, m, s in grid]
    res = mod.icnt_closed_loop_batch(icnt_text, pts, engine=engine, arrivals=arrivals, mem_budget_mb=mem_budget_mb,
                                     lds=lds)
    labelled = [dict(d, traffic=t, rate=r, max_outstanding=m, seed=s) for (t, r, m, s), d in zip(grid, res)]
    if arrivals:
        return labelled
    per = len(seed_list)
    curve = []
    for lo in range(0, len(labelled), per):
        group = labelled[lo:lo + per]
        m = {k: group[0][k] for k in ("traffic", "rate", "max_outstanding", "nodes", "issuers")}
        m["seeds"] = per
        for k in ("batch_time", "request_latency", "reply_latency", "round_trip_latency", "issue_stall",
                  "accepted_request", "accepted_reply", "avg_outstanding", "first_finish", "last_finish", "power_w",
                  "mem_time", "mem_wait", "mem_hold", "mem_utilisation"):
            m[k] = sum(p[k] for p in group) / per
        for k in ("max_round_trip_latency", "max_issue_stall", "max_mem_time", "max_mem_utilisation", "mem_nodes_used"):
            m[k] = max(p[k] for p in group)
        for k in ("requests", "reads", "writes", "deadlocked"):
            m[k] = sum(p[k] for p in group)
        m["batch_times"] = [p["batch_time"] for p in group]
        curve.append(m)
    return curve


def _print_closed_loop(c: Dict, batch: bool) -> None:
    if batch:
        print(f"Batch received. Time used is {c['batch_time']:.0f} cycles "
              f"(nodes finish between {c['first_finish']:.0f} and {c['last_finish']:.0f})")
    print(f"Request average latency = {c['request_latency']:.2f}, reply average latency = {c['reply_latency']:.2f}")
    print(f"Round-trip average latency = {c['round_trip_latency']:.2f} (max {c['max_round_trip_latency']:.0f}), "
          f"from the issue")
    print(f"Issue stall = {c['issue_stall']:.2f} cycles (max {c['max_issue_stall']:.0f}); "
          f"outstanding requests per node = {c['avg_outstanding']:.2f}")
    print(f"Accepted rate: request {c['accepted_request']:.4f}, reply {c['accepted_reply']:.4f}")
    print(f"Memory time = {c['mem_time']:.2f} (max {c['max_mem_time']:.0f}): wait {c['mem_wait']:.2f}, "
          f"in-order hold {c['mem_hold']:.2f}; utilisation {c['mem_utilisation']:.3f} "
          f"(max {c['max_mem_utilisation']:.3f}) over {c['mem_nodes_used']} memory nodes")


def closed_loop_replay(src, dst, req_bytes, reply_bytes, tcreate, icnt_texts: List[str],
                       max_outstanding: Optional[List[int]] = None, reply_delay: int = 0, engine: str = "cpu",
                       arrivals: bool = False, mem_budget_mb: int = 0, lds: bool = True,
                       nodes: int = 0, occupancy=None, latency=None, mem_points=None) -> List[Dict]:
    """One request list, closed loop, through many networks under many windows:
    one dict per (``.icnt`` text, window of `max_outstanding`), network-major,
    with its ``network`` index and ``max_outstanding``.  Request i goes from
    ``src[i]`` to ``dst[i]`` with ``req_bytes[i]`` bytes, is created at
    ``tcreate[i]`` (non-decreasing) and is answered, `reply_delay` cycles
    after its delivery, by ``reply_bytes[i]`` bytes; every network derives its
    own flit counts from the bytes, and a node keeps at most M requests in
    flight (0, the default: unlimited).  ``batch_time`` is the last reply's
    arrival.  The list of a capture file: ``capture.request_list``.
    ``engine="gpu"`` runs one wavefront per (network, window), as many per
    launch as the memory budget takes (csrc/engine/icnt_cln_sweep.hip).
    `nodes`: the list's node count; a network with another one is refused (0:
    not checked).

    `mem_points` adds a third axis, the memory endpoint: each point is
    ``(occupancy, latency)``, applied to every request, or the word ``"list"``
    for the per-request arrays `occupancy` and `latency`.  A memory node is
    one server that a request holds for its occupancy, first come first
    served, with its latency behind it, and replies leave a node in the order
    their requests arrived.  The results are then network-major, then window,
    then memory point, each with its ``mem_point`` index and ``mem`` (the
    point), and ``mem_time``, ``mem_wait``, ``mem_hold`` and
    ``mem_utilisation`` say what the memory nodes did.  Without `mem_points`
    every reply is created `reply_delay` after its request's delivery."""
    mod = _native.load(prefer_torch_runtime=engine == "gpu")
    windows = [0] if max_outstanding is None else [int(m) for m in max_outstanding]
    if mem_points is not None:
        mem_points = [m if isinstance(m, str) else tuple(m) for m in mem_points]
    return [dict(d) for d in mod.icnt_closed_loop_networks(
        (src, dst, req_bytes, reply_bytes, tcreate), list(icnt_texts), windows, reply_delay=int(reply_delay),
        engine=engine, arrivals=arrivals, mem_budget_mb=mem_budget_mb, lds=lds, nodes=nodes, occupancy=occupancy,
        latency=latency, mem_points=mem_points)]


def _main_closed_replay(a) -> int:
    import numpy as np
    from . import capture
    if capture.is_capture(a.replay):
        rl = capture.request_list(capture.load(a.replay), timing=a.timing)
        lst, nodes = (rl.src, rl.dst, rl.req_bytes, rl.reply_bytes, rl.tcreate), rl.nodes
        occ = lat = None  # (a capture file has no service times)
    else:
        with np.load(a.replay) as z:
            missing = [k for k in ("src", "dst", "bytes", "reply_bytes", "tinj") if k not in z]
            if missing:
                print(f"--closed-loop --replay needs a request list with reply sizes: {a.replay} has no "
                      f"{', '.join(missing)} (a capture file, or an .npz with src, dst, bytes, reply_bytes and tinj: "
                      f"capture.save_request_npz)", file=sys.stderr)
                return 2
            order = np.argsort(z["tinj"], kind="stable")
            tinj = z["tinj"][order].astype(np.uint64)
            lst = (z["src"][order], z["dst"][order], z["bytes"][order], z["reply_bytes"][order],
                   tinj if a.timing == "captured" else np.zeros_like(tinj))
            nodes = int(z["nodes"]) if "nodes" in z else 0
            occ = z["occupancy"][order] if "occupancy" in z else None
            lat = z["latency"][order] if "latency" in z else None
    mem_points = None
    if a.mem_occupancy:
        words = [x for x in a.mem_occupancy.split(",") if x]
        if "list" in words and (occ is None or lat is None):
            print(f"--mem-occupancy list needs the request list's occupancy and latency arrays: {a.replay} has none "
                  f"(an .npz with occupancy and latency: capture.save_request_npz)", file=sys.stderr)
            return 2
        mem_points = ["list" if x == "list" else (int(x), a.reply_delay) for x in words]
    files = [n for n in (a.networks or "").split(",") if n] or [a.config]
    windows = [int(x) for x in a.max_outstanding.split(",") if x] if a.max_outstanding else [0]
    res = closed_loop_replay(*lst, [open(f).read() for f in files], windows, reply_delay=a.reply_delay,
                             engine=a.engine, mem_budget_mb=a.mem_budget_mb, nodes=nodes, occupancy=occ, latency=lat,
                             mem_points=mem_points)
    for c in res:
        m = c["max_outstanding"]
        c["config"] = files[c["network"]]
        mem = "" if "mem" not in c else (", memory occupancy from the list" if c["mem"] == "list"
                                         else f", memory occupancy {c['mem'][0]}")
        print(f"====== Closed-loop replay of {a.replay} on {c['config']}, {a.timing} timing, "
              f"max outstanding {m if m else 'unlimited'}{mem} ======")
        _print_closed_loop(c, True)
        print(f"Packets = {c['requests']} requests ({c['request_flits']} flits), {c['reply_flits']} reply flits"
              + (f", {c['deadlocked']} deadlocked" if c["deadlocked"] else ""))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"replay": a.replay, "closed_loop": True, "timing": a.timing, "reply_delay": a.reply_delay,
                       "networks": files, "max_outstanding": windows,
                       **({} if mem_points is None else {"mem_points": mem_points}), "grid": res}, f, indent=1)
    return 0


def _main_closed_loop(a, text: str) -> int:
    traffics = [t for t in a.traffic.split(",") if t]
    seeds = list(range(1, a.seeds + 1)) if a.seeds > 0 else None
    sizes = dict(zip(RR_SIZES, (int(x) for x in a.sizes.split(",")))) if a.sizes else {}
    windows = [int(x) for x in a.max_outstanding.split(",") if x] if a.max_outstanding else None
    rates = [float(x) for x in a.rates.split(",") if x] if a.rates_given else None
    kv = _native.load().parse_booksim_config(text)
    batch = a.batch_size
    if batch is None and rates is None:
        if kv.get("sim_type") != "batch":
            print("--closed-loop needs --batch-size, --rates, or sim_type = batch in the .icnt file", file=sys.stderr)
            return 2
        batch = int(float(kv.get("batch_size", 1)))
    occs = [None]
    if a.mem_occupancy:
        if "list" in a.mem_occupancy.split(","):
            print("--mem-occupancy list needs --replay (a request list with occupancy and latency arrays)", file=sys.stderr)
            return 2
        occs = [int(x) for x in a.mem_occupancy.split(",") if x]
    curve = []
    for occ in occs:  # the memory axis: one batch per occupancy, reads and writes alike
        part = closed_loop_sweep(text, windows, batch_size=batch, rates=None if batch is not None else rates,
                                 engine=a.engine, traffic=traffics if len(traffics) > 1 else a.traffic, cycles=a.cycles,
                                 warmup=a.warmup, seed=a.seed, seeds=seeds, write_fraction=a.write_fraction,
                                 reply_delay=a.reply_delay, mem_nodes=a.mem_nodes, mem_budget_mb=a.mem_budget_mb,
                                 read_occupancy=occ, write_occupancy=occ, write_reply_delay=a.write_reply_delay, **sizes)
        curve += part if occ is None else [dict(c, mem_occupancy=occ) for c in part]
    for c in curve:
        m = c["max_outstanding"]
        what = f"batch size {batch}" if batch is not None else f"injection rate {c['rate']:.3f}"
        mem = f", memory occupancy {c['mem_occupancy']}" if "mem_occupancy" in c else ""
        print(f"====== Traffic {c['traffic']}, closed loop, {what}, max outstanding {m if m else 'unlimited'}{mem} ======")
        _print_closed_loop(c, batch is not None)
        print(f"Packets = {c['reads']} reads, {c['writes']} writes"
              + (f", {c['deadlocked']} deadlocked" if c["deadlocked"] else ""))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "traffic": a.traffic, "closed_loop": True, "batch_size": batch,
                       "reply_delay": a.reply_delay, "mem_nodes": a.mem_nodes, "curve": curve}, f, indent=1)
    return 0


def _mean_rr(points: List[Dict], reply_delay: int) -> Dict[str, float]:
    """The printed figures of one request-reply rate, averaged over its seeds."""
    n = len(points)
    m = {"rate": points[0]["rate"]}
    for side in ("request", "reply"):
        for k in ("avg_latency", "zero_load_latency", "accepted", "offered"):
            m[f"{side}_{k}"] = sum(p[side][k] for p in points) / n
        m[f"{side}_max_latency"] = max(p[side]["max_latency"] for p in points)
    m["round_trip_latency"] = sum(p["round_trip_latency"] for p in points) / n
    m["max_round_trip_latency"] = max(p["max_round_trip_latency"] for p in points)
    m["round_trip_zero_load"] = m["request_zero_load_latency"] + m["reply_zero_load_latency"] + reply_delay
    for k in ("reads", "writes", "deadlocked"):
        m[k] = sum(p[k] for p in points)
    m["measured_packets"] = sum(p["request"]["measured_packets"] for p in points)
    return m


def saturation_round_trip(means: List[Dict[str, float]], factor: float = 3.0) -> float:
    """Highest offered rate whose round trip stays within `factor` x its zero load."""
    ok = [c["rate"] for c in means
          if c["measured_packets"] and c["round_trip_latency"] <= factor * c["round_trip_zero_load"]]
    return max(ok) if ok else 0.0


def _print_open_loop(c: Dict) -> None:
    print(f"Overall average latency = {c['avg_latency']:.2f} (zero load {c['zero_load_latency']:.2f}, "
          f"max {c['max_latency']:.0f})")
    print(f"Overall average accepted rate = {c['accepted']:.4f} (offered {c['offered']:.4f}; "
          f"drain rate {c['drain_throughput']:.4f})")
    e = c["energy_pj"]
    print(f"Network power = {c['power_w']:.3f} W (energy pJ: buffer {e['buffer']:.3g}, crossbar {e['crossbar']:.3g}, "
          f"link {e['link']:.3g}, allocator {e['allocator']:.3g}, leakage {e['leakage']:.3g})")
    print(f"Packets = {c['measured_packets']} measured of {c['packets']}"
          + (f", {c['deadlocked']} deadlocked" if c["deadlocked"] else ""))


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


def _main_request_reply(a, text: str) -> int:
    traffics = [t for t in a.traffic.split(",") if t]
    seeds = list(range(1, a.seeds + 1)) if a.seeds > 0 else None
    sizes = dict(zip(RR_SIZES, (int(x) for x in a.sizes.split(",")))) if a.sizes else {}
    rates = [float(x) for x in a.rates.split(",") if x]
    curve = request_reply_sweep(text, rates, engine=a.engine, traffic=traffics if len(traffics) > 1 else a.traffic,
                                cycles=a.cycles, warmup=a.warmup, seed=a.seed, seeds=seeds,
                                write_fraction=a.write_fraction, reply_delay=a.reply_delay, mem_nodes=a.mem_nodes,
                                mem_budget_mb=a.mem_budget_mb, **sizes)
    per = len(seeds) if seeds else 1
    nrate = len(rates)
    for ti, traffic in enumerate(traffics):
        means = [_mean_rr(curve[(ti * nrate + ri) * per:(ti * nrate + ri + 1) * per], a.reply_delay)
                 for ri in range(nrate)]
        for c in means:
            print(f"====== Traffic {traffic}, request-reply, injection rate {c['rate']:.3f} ======")
            for side, name in (("request", "Request"), ("reply", "Reply")):
                print(f"{name} average latency = {c[side + '_avg_latency']:.2f} "
                      f"(zero load {c[side + '_zero_load_latency']:.2f}, max {c[side + '_max_latency']:.0f})")
            print(f"Round-trip average latency = {c['round_trip_latency']:.2f} "
                  f"(zero load {c['round_trip_zero_load']:.2f}, max {c['max_round_trip_latency']:.0f})")
            print(f"Accepted rate: request {c['request_accepted']:.4f} (offered {c['request_offered']:.4f}), "
                  f"reply {c['reply_accepted']:.4f} (offered {c['reply_offered']:.4f})")
            print(f"Packets = {c['reads']} reads, {c['writes']} writes"
                  + (f", {c['deadlocked']} deadlocked" if c["deadlocked"] else ""))
        print(f"Saturation (round trip <= 3x zero load): {saturation_round_trip(means):.3f} flits/node/cycle")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "traffic": a.traffic, "request_reply": True, "reply_delay": a.reply_delay,
                       "mem_nodes": a.mem_nodes, "curve": curve}, f, indent=1)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("config", nargs="?", help="Booksim .icnt file (optional with --replay FILE --networks ...)")
    ap.add_argument("--traffic", default="uniform",
                    help="uniform, transpose, bitcomp, bitrev, shuffle, tornado, neighbor (comma list)")
    ap.add_argument("--rates", default=None,
                    help="offered load, flits per node per cycle (comma list; default 0.05 .. 1.0 in nine steps)")
    ap.add_argument("--packet-flits", type=int, default=1)
    ap.add_argument("--cycles", type=int, default=None, help="default 5000 (--replay: the last injection + 1)")
    ap.add_argument("--warmup", type=int, default=None, help="default 1000 (--replay: 0)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seeds", type=int, default=0,
                    help="run seeds 1..N and print their average per rate (the JSON keeps every point)")
    ap.add_argument("--engine", choices=("cpu", "cpu-par", "gpu"), default="cpu",
                    help="cpu: the sequential router pass; cpu-par: the lane-parallel pass on the host; "
                         "gpu: one wavefront per point, the whole grid in one batch")
    ap.add_argument("--mem-budget-mb", type=int, default=0,
                    help="gpu: device memory of one launch (default: half the free device memory)")
    ap.add_argument("--request-reply", action="store_true",
                    help="reads and writes on the request subnet, their replies on the reply subnet (sizes and "
                         "write_fraction from the .icnt file's Booksim keys)")
    ap.add_argument("--write-fraction", type=float, default=None, help="request-reply: share of writes")
    ap.add_argument("--reply-delay", type=int, default=0, help="request-reply: the destination's service time, cycles")
    ap.add_argument("--mem-nodes", type=int, default=0,
                    help="request-reply: the last M nodes are memory partitions, the others issue to them")
    ap.add_argument("--sizes", default=None,
                    help="request-reply: read request, read reply, write request, write reply flits (comma list)")
    ap.add_argument("--closed-loop", action="store_true",
                    help="request-reply traffic with bounded windows: a node issues its next request when a reply "
                         "has come back (Booksim's sim_type = batch)")
    ap.add_argument("--max-outstanding", metavar="M,M,...", default=None,
                    help="closed loop: requests in flight per node, 0 unlimited (comma list; default: the .icnt "
                         "file's max_outstanding_requests, else unlimited)")
    ap.add_argument("--batch-size", type=int, default=None,
                    help="closed loop: every issuing node creates this many requests at cycle 0 (default: the .icnt "
                         "file's batch_size when its sim_type is batch; else --rates points)")
    ap.add_argument("--replay", metavar="FILE",
                    help="run the packet list of an .npz (src, dst, flits, tinj) or of a cycle simulation's "
                         "-icnt_capture file")
    ap.add_argument("--subnet", choices=("request", "reply", "both"), default="request",
                    help="--replay of a capture file: the subnet (both: two independent replays, one result each)")
    ap.add_argument("--networks", metavar="A.icnt,B.icnt,...",
                    help="--replay: the list through each of these networks (in place of the one config), every "
                         "network with its own flit counts from the packets' bytes; --engine gpu: one launch")
    ap.add_argument("--timing", choices=("captured", "batch"), default="captured",
                    help="--closed-loop --replay: the requests' creation times as captured, or all at cycle 0 in "
                         "captured order")
    ap.add_argument("--mem-occupancy", metavar="O,O,...", default=None,
                    help="closed loop: a memory node is one server that a request holds for O cycles, with "
                         "--reply-delay as the latency behind it (comma list: one more axis of the grid; with "
                         "--replay the word `list` takes the .npz file's occupancy and latency arrays)")
    ap.add_argument("--write-reply-delay", type=int, default=None,
                    help="closed loop, synthetic traffic: a write's latency at its memory node (default: --reply-delay)")
    ap.add_argument("--json", help="write the latency / throughput curve here")
    a = ap.parse_args(argv)
    a.rates_given = a.rates is not None
    if a.rates is None:
        a.rates = "0.05,0.1,0.2,0.3,0.4,0.5,0.6,0.8,1.0"
    if a.replay:
        if not a.config and not a.networks:
            ap.error("--replay needs a config or --networks")
        return _main_closed_replay(a) if a.closed_loop else _main_replay(a)
    if not a.config:
        ap.error("the following arguments are required: config")
    if a.networks:
        ap.error("--networks needs --replay")
    text = open(a.config).read()
    a.cycles = 5000 if a.cycles is None else a.cycles
    a.warmup = 1000 if a.warmup is None else a.warmup
    if a.closed_loop:
        return _main_closed_loop(a, text)
    if a.request_reply:
        return _main_request_reply(a, text)
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
            _print_open_loop(c)
        print(f"Saturation (latency <= 3x zero load): {saturation(means):.3f} flits/node/cycle")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "traffic": a.traffic, "packet_flits": a.packet_flits, "curve": curve},
                      f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
