"""Every engine kernel build the GPU engine can launch, bit-exact against the
CPU engine (gpu_engine.hip chooses the kernel from ASIM_GPU_STATE,
ASIM_GPU_SPLIT_WAVES, ASIM_GPU_BLOCKS and ASIM_GPU_PROFILE).

The choice is made from the environment when a process first simulates, and
the occupancy it plans with is cached per state mode, so each build runs in a
fresh child process (accel_sim_framework_distributed_amd/ops/build_child.py),
one at a time.  The child reports which kernel variant its launches ran; a
build that silently ran another kernel fails.  ASIM_GPU_SPLIT_WAVES=2 is
never combined with ASIM_GPU_BATCH or ASIM_GPU_PROFILE (oversubscribed CUs,
ADVICE.md item 1).
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# about 5x the slowest child measured on an MI355X (2.8 s, torch import and four simulations)
CHILD_TIMEOUT_S = 15

# id -> (environment, variant the launches must report, block cap or None)
BUILDS = {
    "lds": ({"ASIM_GPU_STATE": "lds"}, "lds", None),
    "lds_sliced7": ({"ASIM_GPU_STATE": "lds", "ASIM_GPU_BLOCKS": "7"}, "lds_sliced", 7),
    "split2": ({"ASIM_GPU_STATE": "split", "ASIM_GPU_SPLIT_WAVES": "2"}, "split2", None),
    "split2_blocks37": ({"ASIM_GPU_STATE": "split", "ASIM_GPU_SPLIT_WAVES": "2", "ASIM_GPU_BLOCKS": "37"}, "split2", 37),
    "split_prof": ({"ASIM_GPU_STATE": "split", "ASIM_GPU_PROFILE": "1"}, "split_prof", None),
    "lds_prof": ({"ASIM_GPU_STATE": "lds", "ASIM_GPU_PROFILE": "1"}, "lds_prof", None),
}
_ENGINE_ENV = ("ASIM_GPU_STATE", "ASIM_GPU_SPLIT_WAVES", "ASIM_GPU_BLOCKS", "ASIM_GPU_PROFILE", "ASIM_GPU_BATCH",
               "ASIM_GPU_BLOCKS_PER_CU", "ASIM_GPU_CH_PER_BLOCK", "ASIM_NATIVE_SO")
# a child that hung or died by a signal: nothing more is started on the GPU
_dead = {"why": None}


def _strip(stats):
    return {k: v for k, v in stats.items() if "rate" not in k and "slowdown" not in k and "time" not in k}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """The applications (written once) and the CPU engine's result for each."""
    import torch  # bind torch's HIP runtime first
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from accel_sim_framework_distributed_amd import sim
    from accel_sim_framework_distributed_amd.tracegen import fuzz, rodinia
    root = tmp_path_factory.mktemp("builds")
    apps = [dict(name="hotspot", kernelslist=rodinia.write_app(str(root / "hs"), rodinia.hotspot(64, 2, 2)),
                 preset="QV100", extra={}),
            dict(name="bfs", kernelslist=rodinia.write_app(str(root / "bfs"), rodinia.bfs(2048, levels=3)),
                 preset="QV100", extra={})]
    for c in fuzz.BUILD_CASES:
        preset, extra = fuzz.case_config(c)
        apps.append(dict(name="fuzz_" + c.id, kernelslist=fuzz.write_case(str(root / c.id), c), preset=preset,
                         extra=extra))
    manifest = str(root / "manifest.json")
    with open(manifest, "w") as f:
        json.dump(apps, f)
    cpu = {}
    for a in apps:
        s = sim.Simulator(a["preset"], a["kernelslist"], engine="cpu", extra=a["extra"] or None)
        r = s.run()
        cfg = s.mod.parse_config(sim.build_args(a["preset"], None, "cpu", a["extra"] or None))
        cpu[a["name"]] = dict(tot_cycle=r.tot_cycle, tot_insn=r.tot_insn, deadlock=r.deadlock,
                              kernel_cycles=[k["cycles"] for k in r.kernels],
                              stats=json.loads(json.dumps(_strip(r.stats))),
                              snapshot_sha256=hashlib.sha256(bytes(s.native.snapshot())).hexdigest(),
                              units=int(cfg["n_sm"]) + int(cfg["n_mem"]))
    return manifest, apps, cpu


@pytest.mark.parametrize("build", list(BUILDS))
def test_engine_build_equals_cpu(reference, build):
    if _dead["why"]:
        pytest.fail("not started: an earlier engine-build child " + _dead["why"])
    manifest, apps, cpu = reference
    env_add, variant, cap = BUILDS[build]
    assert not ("ASIM_GPU_SPLIT_WAVES" in env_add and ({"ASIM_GPU_PROFILE", "ASIM_GPU_BATCH"} & set(env_add)))
    env = {k: v for k, v in os.environ.items() if k not in _ENGINE_ENV}
    env.update(env_add)
    cmd = [sys.executable, "-m", "accel_sim_framework_distributed_amd.ops.build_child", manifest, variant]
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _dead["why"] = f"({build}) did not finish in {CHILD_TIMEOUT_S} s"
        pytest.fail("engine-build child " + _dead["why"])
    if p.returncode < 0:
        _dead["why"] = f"({build}) died by signal {-p.returncode}"
        pytest.fail("engine-build child " + _dead["why"] + "\n" + p.stderr[-2000:])
    assert p.returncode == 0, p.stderr[-2000:]
    got = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert [g["name"] for g in got] == [a["name"] for a in apps]
    print(build, "child wall_s per app:", {g["name"]: g["wall_s"] for g in got})
    for g in got:
        c = cpu[g["name"]]
        assert g["engine"] == "gpu" and not g["deadlock"], g["name"]
        assert g["variant"] == variant, (g["name"], g["variant"])
        assert g["blocks"] == (min(cap, c["units"]) if cap else c["units"]), (g["name"], g["blocks"], c["units"])
        assert (g["tot_cycle"], g["tot_insn"]) == (c["tot_cycle"], c["tot_insn"]), g["name"]
        assert g["kernel_cycles"] == c["kernel_cycles"], g["name"]
        assert _strip(g["stats"]) == c["stats"], g["name"]
        assert g["snapshot_sha256"] == c["snapshot_sha256"], g["name"]
