#!/usr/bin/env python3
"""Time one request-reply grid on the host path, on the fused GPU kernel and
as two GPU replay batches with the reply lists built on the host in between.

The grid is 9 rates x {uniform, transpose} x 4 seeds = 72 points of an 8x8
mesh, 5000 cycles each, sizes 1/5/5/1 flits (read request, read reply, write
request, write reply) and a write fraction of 0.3.  Three forms of the same
work:

  cpu    ``icnt_request_reply_batch(engine="cpu")``: one core, one point after
         the other, the reply order by std::stable_sort
  gpu    ``engine="gpu"``: one launch, per point one wavefront that runs the
         request pass, orders the replies on the device and runs the reply pass
  split  ``icnt_request_reply_schedule`` + ``icnt_replay_batch(engine="gpu")``
         on the request lists + a numpy stable sort of the arrivals on the host
         + ``icnt_replay_batch(engine="gpu")`` on the reply lists: two launches
         with a round trip through the host between the subnets

Every form runs once untimed, then ``--repeats`` times timed.  The GPU forms
run in one child process under ``timeout -k 10``, the host form in another;
any failure stops the script.  The record (JSON) holds every time, whether
all results are equal (every array, both state images, every summary), how
the batches were packed, and the kernel's registers, scratch and LDS.

    python tools/icnt_rr_bench.py --out profiles/icnt_reqreply/record.json
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

RATES = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.8, 1.0)
PATTERNS = ("uniform", "transpose")
SIZES = dict(read_request_size=1, read_reply_size=5, write_request_size=5, write_reply_size=1)


def grid(a):
    return [dict(SIZES, traffic=t, rate=r, seed=s, cycles=a.cycles, warmup=a.warmup, write_fraction=0.3,
                 reply_delay=a.reply_delay)
            for t in PATTERNS for r in RATES for s in range(1, a.seeds + 1)]


def network(a) -> str:
    from accel_sim_framework_distributed_amd.models import presets
    return presets.render_icnt(presets.icnt_params(k=a.k, n=2, topology="mesh", num_vcs=a.vcs, vc_buf_size=a.buf,
                                                   internal_speedup="1.0", flit_size=32))


def split_form(mod, text, pts, a):
    """The grid as two replay batches; returns per point what the fused form
    returns for the arrays the two have in common."""
    import numpy as np
    sched = mod.icnt_request_reply_schedule(text, pts)
    kw = dict(engine="gpu", arrivals=True, mem_budget_mb=a.mem_budget_mb, cycles=a.cycles, warmup=a.warmup)
    rq = mod.icnt_replay_batch(text, [(s["src"], s["dst"], s["flits"], s["tinj"]) for s in sched], **kw)
    lists, orders = [], []
    for s, r, p in zip(sched, rq, pts):
        key = r["arrivals"] + np.uint64(p["reply_delay"])
        o = np.argsort(key, kind="stable").astype(np.uint32)
        fl = np.where(s["kind"][o] == 1, p["write_reply_size"], p["read_reply_size"]).astype(np.uint32)
        lists.append((s["dst"][o], s["src"][o], fl, key[o]))
        orders.append(o)
    rp = mod.icnt_replay_batch(text, lists, **kw)
    return [dict(request_arrivals=q["arrivals"], request_state=q["state"], reply_of=o, reply_tinj=l[3],
                 reply_arrivals=r["arrivals"], reply_state=r["state"],
                 request={k: v for k, v in q.items() if k not in ("arrivals", "state")},
                 reply={k: v for k, v in r.items() if k not in ("arrivals", "state")})
            for q, r, o, l in zip(rq, rp, orders, lists)]


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
        res, rec["cpu_seconds"] = timed(lambda: mod.icnt_request_reply_batch(text, pts, engine="cpu", arrivals=True),
                                        a.repeats)
        rec["results"] = res
    else:
        if not mod.gpu_available():
            print("no usable HIP device", file=sys.stderr)
            return 2
        res, rec["gpu_seconds"] = timed(lambda: mod.icnt_request_reply_batch(
            text, pts, engine="gpu", arrivals=True, mem_budget_mb=a.mem_budget_mb), a.repeats)
        rec["batch"] = dict(mod.icnt_open_loop_batch_stats())
        rec["kernel"] = dict(mod.icnt_rr_kernel_info())
        rec["results"] = res
        rec["split_results"], rec["split_seconds"] = timed(lambda: split_form(mod, text, pts, a), a.repeats)
        rec["split_batch"] = dict(mod.icnt_open_loop_batch_stats())  # of the reply batch, the larger of the two
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
    ap.add_argument("--out", default="icnt_rr_record.json")
    ap.add_argument("--k", type=int, default=8, help="k x k mesh")
    ap.add_argument("--vcs", type=int, default=2)
    ap.add_argument("--buf", type=int, default=8)
    ap.add_argument("--cycles", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--reply-delay", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mem-budget-mb", type=int, default=0)
    ap.add_argument("--gpu-timeout", type=int, default=900, help="seconds the GPU step may take")
    ap.add_argument("--worker", choices=("cpu", "gpu"), help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.worker:
        return worker(a)
    common = ["--k", str(a.k), "--vcs", str(a.vcs), "--buf", str(a.buf), "--cycles", str(a.cycles), "--warmup",
              str(a.warmup), "--reply-delay", str(a.reply_delay), "--seeds", str(a.seeds), "--repeats",
              str(a.repeats), "--mem-budget-mb", str(a.mem_budget_mb)]
    recs = {}
    with tempfile.TemporaryDirectory(prefix="icnt_rr_") as tmp:
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
    split_equal = all(same(s[k], g[k]) for s, g in zip(gpu["split_results"], gpu["results"]) for k in s)
    best = lambda v: min(v)
    spread = max(gpu["split_seconds"]) - min(gpu["split_seconds"])
    rec = {
        "grid": {"network": f"{a.k}x{a.k} mesh, {a.vcs} VCs x {a.buf} flits, 32-byte flits", "rates": list(RATES),
                 "patterns": list(PATTERNS), "seeds": a.seeds, "cycles": a.cycles, "warmup": a.warmup,
                 "sizes": SIZES, "write_fraction": 0.3, "reply_delay": a.reply_delay, "points": cpu["points"],
                 "requests": sum(r["request"]["packets"] for r in cpu["results"]),
                 "switch_passes": sum(r[s]["activity"]["switch_passes"] for r in cpu["results"]
                                      for s in ("request", "reply"))},
        "repeats": a.repeats,
        "cpu_seconds": cpu["cpu_seconds"], "gpu_seconds": gpu["gpu_seconds"], "split_seconds": gpu["split_seconds"],
        "cpu_over_gpu": best(cpu["cpu_seconds"]) / best(gpu["gpu_seconds"]),
        "split_over_gpu": best(gpu["split_seconds"]) / best(gpu["gpu_seconds"]),
        "split_spread_seconds": spread,
        "fused_faster_than_split_beyond_spread": best(gpu["split_seconds"]) - max(gpu["gpu_seconds"]) > spread,
        "gpu_results_equal_cpu": equal, "split_results_equal_gpu": split_equal,
        "batch": gpu["batch"], "split_reply_batch": gpu["split_batch"], "kernel": gpu["kernel"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "grid"}))
    return 0 if equal and split_equal else 1


if __name__ == "__main__":
    sys.exit(main())
