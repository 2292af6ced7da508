"""Run the GPU engine on a list of applications in THIS process's engine build.

The engine kernel a process launches is chosen from the environment when the
process starts (ASIM_GPU_STATE, ASIM_GPU_SPLIT_WAVES, ASIM_GPU_BLOCKS,
ASIM_GPU_PROFILE) and the occupancy it plans with is cached per state mode,
so one process must not change those variables between simulations: every
build is exercised in a fresh child with its environment set beforehand
(tests/test_engine_builds.py).

    python -m accel_sim_framework_distributed_amd.ops.build_child MANIFEST.json VARIANT

MANIFEST.json: [{"name", "kernelslist", "preset", "extra"}, ...].  One JSON line
per application goes to stdout: cycles, instructions, per-kernel cycles, the
statistics, the SHA-256 of the engine's state image, the kernel variant and
block count the engine reports for its last launch, the router pass's
counters (-sim_router_pass) and, for an application whose `extra` sets
-icnt_capture, the capture file's SHA-256.  The run fails if
that variant is not VARIANT, so a mistyped variable cannot pass as a test of
the default build.
"""
from __future__ import annotations

import hashlib
import json
import re
import sys
import time


def run_app(app: dict) -> dict:
    from .. import sim
    s = sim.Simulator(app["preset"], app["kernelslist"], engine="gpu", extra=app.get("extra") or None,
                      torch_runtime=True)
    t0 = time.perf_counter()
    r = s.run()
    wall = time.perf_counter() - t0
    m = re.search(r"^engine_kernel_variant: (\S+) blocks=(\d+)$", r.output, re.M)
    out = dict(name=app["name"], engine=r.engine, deadlock=r.deadlock, tot_cycle=r.tot_cycle, tot_insn=r.tot_insn,
               kernel_cycles=[k["cycles"] for k in r.kernels], stats=r.stats,
               snapshot_sha256=hashlib.sha256(bytes(s.native.snapshot())).hexdigest(),
               variant=m.group(1) if m else None, blocks=int(m.group(2)) if m else 0, wall_s=round(wall, 3),
               router_pass=r.router_pass)
    cap = (app.get("extra") or {}).get("-icnt_capture")
    if cap:
        with open(cap, "rb") as f:
            out["icnt_capture_sha256"] = hashlib.sha256(f.read()).hexdigest()
    return out


def main(argv) -> int:
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    import torch  # first: bind torch's HIP runtime

    if not torch.cuda.is_available():
        print("build_child: no GPU visible", file=sys.stderr)
        return 3
    from .. import _native
    if not _native.load(prefer_torch_runtime=True).gpu_available():
        print("build_child: the HIP engine cannot see the GPU", file=sys.stderr)
        return 3
    with open(argv[0]) as f:
        apps = json.load(f)
    for app in apps:
        out = run_app(app)
        print(json.dumps(out), flush=True)
        if out["variant"] != argv[1]:
            print(f"build_child: engine ran variant {out['variant']!r}, expected {argv[1]!r}", file=sys.stderr)
            return 4
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
