"""-sim_router_pass par: the cycle engines' epoch pass of the router model
(-icnt_link_contention 2) on the lane-parallel rt_simulate_par
(csrc/model/icnt_router_par.h rt_epoch_run_par) instead of the serial
rt_simulate.  On the GPU engine all 64 lanes of block 0 run the request subnet
while block 1 runs the reply subnet.  The option changes who computes the
pass, never what it computes: every run below equals the CPU engine's serial
pass in cycles, link statistics, injection stalls and the state image.

Shapes (largest packet count of one pass, from Simulator.router_pass_stats):
  small   16 clusters + 16 sub-partitions, the spread hotspot kernel: 144
          request packets in one pass, three lane strides
  full    the QV100 preset (80 SMs, 64 sub-partitions, 112 engine blocks) on a
          12 x 12 mesh, the same-line hotspot kernel: both subnets above 64
  bp      the small mesh with a 9-flit injection queue and 5-flit write
          packets: injection back-pressure
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import pytest

from accel_sim_framework_distributed_amd.models import presets
from accel_sim_framework_distributed_amd.tracegen import rodinia

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = {"-gpgpu_n_clusters": "16", "-gpgpu_n_mem": "8"}  # 16 clusters + 16 sub-partitions = 32 nodes
ROUTER = {"-icnt_link_contention": "2", "-gpgpu_perf_sim_memcpy": "0"}

# name -> (.icnt parameters, kernel): the network variants on the small machine with the same-line hotspot
# kernel (at most 48 packets in a pass), then the small shape (the spread kernel) and bp
MESH = dict(k=8, n=2, topology="mesh")
CASES = {
    "mesh": (dict(MESH), "hot"),
    "torus": (dict(k=8, n=2, topology="torus", num_vcs=2), "hot"),
    "cmesh": (dict(k=4, n=2, c=2, topology="cmesh"), "hot"),
    "fly": (dict(k=32, n=1), "hot"),
    "mesh_min_adapt": (dict(MESH, routing_function="min_adapt", num_vcs=4), "hot"),
    "mesh_valiant": (dict(MESH, routing_function="valiant", num_vcs=2), "hot"),
    "mesh_sep_input_first": (dict(MESH, sw_allocator="separable_input_first", alloc_iters=2, num_vcs=2), "hot"),
    "mesh_sep_output_first": (dict(MESH, sw_allocator="separable_output_first", num_vcs=2), "hot"),
    "fly_max_size": (dict(k=32, n=1, sw_allocator="max_size", num_vcs=2), "hot"),
    "mesh_wavefront": (dict(MESH, sw_allocator="wavefront", num_vcs=2), "hot"),
    "mesh_credit_delay": (dict(MESH, credit_delay=2, vc_buf_size=2, num_vcs=2), "hot"),
    "mesh_flit16": (dict(MESH, flit_size=16, num_vcs=2, vc_buf_size=4), "hot"),
    "small": (dict(MESH), "spread"),
    "bp": (dict(MESH, input_buffer_size=9, vc_buf_size=4, internal_speedup="1.0"), "stores32"),
}
FULL = (dict(k=12, n=2, topology="mesh", num_vcs=2), "hot")


def _icnt_args(tmp_path, name, **kw):
    p = tmp_path / f"{name}.icnt"
    p.write_text(presets.render_icnt(presets.icnt_params(**kw)))
    # 16 clusters + 16 sub-partitions = 32 nodes
    return presets.args_for("QV100", dict(SMALL, **{"-network_mode": "1", "-inter_config_file": str(p)}))


def _hotspot_app(tmp_path, name, same_line):
    """80 single-warp CTAs; each warp issues 16 independent loads.  same_line:
    every SM reads the same lines, whose requests all meet at ONE L2
    sub-partition's port (a hotspot); else each SM reads its own lines,
    spread over all sub-partitions."""
    from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder
    import numpy as np
    k = KernelBuilder("_Z7hotspotPf", (80, 1, 1), (32, 1, 1), nregs=32)
    g = k.g
    for i in range(16):
        if same_line:
            base = np.full(g.nwarps, 0x7000_0000 + i * 0x40000, np.int64)
            k.op("LDG.E", [8 + i], [2], base=base, stride=0)
        else:
            k.op("LDG.E", [8 + i], [2], base=0x7000_0000 + g.cta * 0x100000 + i * 128, stride=4)
    for i in range(16):
        k.op("FADD", [5], [8 + i, 5])
    k.op("EXIT")
    return rodinia.write_app(str(tmp_path / name), [k.build()], memcpy=False)


def _store_app(tmp_path, name, stores):
    """80 single-warp CTAs, each storing `stores` full lines (5-flit write
    packets) to the same L2 sub-partition: offered load grows with `stores`."""
    from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder
    import numpy as np
    k = KernelBuilder("_Z6storesPf", (80, 1, 1), (32, 1, 1), nregs=32)
    for i in range(stores):
        base = 0x7000_0000 + np.arange(k.g.nwarps, dtype=np.int64) * 0x100000 + i * 0x40000
        k.op("STG.E", [], [2, 3], base=base, stride=4)
    k.op("EXIT")
    return rodinia.write_app(str(tmp_path / name), [k.build()], memcpy=False)


def _link_stat(out, key):
    return int(re.findall(rf"^{key} = (\d+)", out, re.M)[-1])


STAT_KEYS = ("Network_link_delayed_packets", "Network_link_wait_cycles", "Req_Network_injection_stall_cycles",
             "Reply_Network_injection_stall_cycles", "Network_router_deadlocked_packets")


def _flat(extra):
    return [x for kv in extra.items() for x in kv]


class _Work:
    """The applications and .icnt files, written once, and the CPU engine's
    serial result of every case, computed once and shared by the tests."""

    def __init__(self, root):
        self.root = root
        self.apps = {"spread": _hotspot_app(root, "spread", False), "hot": _hotspot_app(root, "hot", True),
                     "stores32": _store_app(root, "stores32", 32)}
        self._ref = {}

    def args(self, case):
        if case == "full":
            p = self.root / "full.icnt"
            p.write_text(presets.render_icnt(presets.icnt_params(**FULL[0])))
            return presets.args_for("QV100", {"-network_mode": "1", "-inter_config_file": str(p)}), self.apps[FULL[1]]
        kw, app = CASES[case]
        return _icnt_args(self.root, case, **kw), self.apps[app]

    def run(self, native, case, engine="cpu", mode=None, more=()):
        args, kl = self.args(case)
        opts = list(more) + (["-sim_router_pass", mode] if mode else [])
        s = native.Simulator(args + _flat(ROUTER) + opts + ["-sim_engine", engine, "-trace", kl], False)
        assert s.run() == 0 and not s.deadlock, case
        res = (s.tot_cycle,) + tuple(_link_stat(s.output, k) for k in STAT_KEYS)
        return res, bytes(s.snapshot()), s

    def ref(self, native, case):
        """CPU engine, serial pass (the parent commit's code path)."""
        if case not in self._ref:
            res, snap, s = self.run(native, case, "cpu", "serial")
            assert s.router_pass_stats() == dict(mode="serial", passes=0, max_packets_req=0, max_packets_rep=0,
                                                 split_blocks=0)
            # an empty network would pass every comparison
            assert res[1] > 0 and res[5] == 0, (case, res)
            self._ref[case] = (res, snap)
        return self._ref[case]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return _Work(tmp_path_factory.mktemp("router_pass"))


# ---- CPU ---------------------------------------------------------------------
def test_option_grammar(native, work):
    base, kl = work.args("mesh")
    assert native.parse_config(base)["router_pass"] == "serial"
    assert native.parse_config(base + ["-sim_router_pass", "par"])["router_pass"] == "par"
    assert native.parse_config(base + ["-sim_router_pass", "serial", "-sim_router_step_cap", "7"])["router_pass"] == "serial"
    with pytest.raises(Exception, match="-sim_router_pass"):
        native.parse_config(base + ["-sim_router_pass", "fast"])
    # accepted and without effect unless the router model is on: no printed
    # statistic and no byte of the state image moves
    from accel_sim_framework_distributed_amd.utils import stats as st
    outs = []
    for opt in ([], ["-sim_router_pass", "par", "-sim_router_step_cap", "1"]):
        for lc in ("0", "1"):
            s = native.Simulator(base + ["-icnt_link_contention", lc, "-gpgpu_perf_sim_memcpy", "0"] + opt +
                                 ["-trace", kl], False)
            assert s.run() == 0
            fs = {k: v for k, v in st.final_stats(s.output).items()
                  if "rate" not in k and "slowdown" not in k and "time" not in k}
            lines = [l for l in s.output.splitlines() if re.match(r"^[A-Za-z_\[\]0-9 ]+ = [0-9.]+$", l)
                     and not re.search("rate|slowdown|time", l)]
            outs.append((lc, s.tot_cycle, fs, lines, bytes(s.snapshot()), s.router_pass_stats()))
    assert len(outs[0][3]) > 20
    for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):
        assert a[:5] == b[:5]
        assert a[5]["mode"] == "serial" and b[5] == dict(mode="par", passes=0, max_packets_req=0, max_packets_rep=0,
                                                         split_blocks=0)


@pytest.mark.parametrize("case", list(CASES))
def test_par_equals_serial_on_the_cpu_engine(native, work, case):
    ref, snap = work.ref(native, case)
    res, psnap, s = work.run(native, case, "cpu", "par")
    assert res == ref and psnap == snap
    st = s.router_pass_stats()
    assert st["mode"] == "par" and st["passes"] > 0 and st["split_blocks"] == 1
    # the default is the serial pass
    dres, dsnap, d = work.run(native, case, "cpu", None)
    assert dres == ref and dsnap == snap and d.router_pass_stats()["mode"] == "serial"


@pytest.mark.parametrize("case", ["mesh", "small", "bp"])
def test_par_with_cpu_threads(native, work, case):
    ref, snap = work.ref(native, case)
    res, psnap, _ = work.run(native, case, "cpu", "par", ["-sim_cpu_threads", "4"])
    assert res == ref and psnap == snap


def test_inputs_reach_the_lane_strides(native, work):
    _, _, s = work.run(native, "small", "cpu", "par")
    st = s.router_pass_stats()
    print("small:", st)
    assert st["passes"] > 0 and st["max_packets_req"] > 128
    ref, snap = work.ref(native, "full")
    res, psnap, s = work.run(native, "full", "cpu", "par")
    st = s.router_pass_stats()
    print("full:", st)
    assert st["passes"] > 0 and st["max_packets_req"] > 64 and st["max_packets_rep"] > 64
    assert res == ref and psnap == snap


def test_checkpoint_across_modes(native, tmp_path):
    """A checkpoint written under one pass resumes under the other and ends
    where the uninterrupted run does (the pass is not part of the state)."""
    kl = rodinia.write_app(str(tmp_path / "pf"), rodinia.pathfinder(4000, 12, 2))
    mesh = _icnt_args(tmp_path, "mesh", **MESH) + ["-icnt_link_contention", "2", "-trace", kl]
    full = native.Simulator(mesh, False)
    assert full.run() == 0

    def end(s):
        return (s.tot_cycle,) + tuple(_link_stat(s.output, k) for k in STAT_KEYS)
    assert end(full)[1] > 0
    for first_mode, rest_mode in (("serial", "par"), ("par", "serial")):
        ck = ["-checkpoint_path", str(tmp_path / f"ck_{first_mode}")]
        first = native.Simulator(mesh + ck + ["-sim_router_pass", first_mode, "-checkpoint_option", "1",
                                              "-checkpoint_kernel", "2"], False)
        assert first.run() == 0
        rest = native.Simulator(mesh + ck + ["-sim_router_pass", rest_mode, "-resume_option", "1",
                                             "-resume_kernel", "2"], False)
        assert rest.run() == 0 and "resumed from" in rest.output
        assert rest.router_pass_stats()["mode"] == rest_mode
        assert end(rest) == end(full), (first_mode, rest_mode)
        assert bytes(rest.snapshot()) == bytes(full.snapshot())


def test_step_cap_is_an_error_on_the_cpu_engine(native, work):
    args, kl = work.args("mesh")
    s = native.Simulator(args + _flat(ROUTER) + ["-sim_router_pass", "par", "-sim_router_step_cap", "1",
                                                 "-trace", kl], False)
    t0 = time.perf_counter()
    with pytest.raises(Exception, match="step cap"):
        s.run()
    assert time.perf_counter() - t0 < 5.0
    # the serial pass has no such guard and ignores the option
    res, snap, _ = work.run(native, "mesh", "cpu", "serial", ["-sim_router_step_cap", "1"])
    assert (res, snap) == work.ref(native, "mesh")


# ---- GPU ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_mod():
    import torch  # bind torch's HIP runtime first
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from accel_sim_framework_distributed_amd import _native
    mod = _native.load(prefer_torch_runtime=True)
    assert mod.gpu_available(), "HIP engine cannot see the GPU (native code must run, no silent fallback)"
    return mod


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_par_equals_cpu_serial(gpu_mod, work, case):
    ref, snap = work.ref(gpu_mod, case)
    res, gsnap, s = work.run(gpu_mod, case, "gpu", "par")
    st = s.router_pass_stats()
    print(case, st)
    assert res == ref and gsnap == snap
    assert st["mode"] == "par" and st["passes"] > 0 and st["split_blocks"] == 2
    if case == "small":
        assert st["max_packets_req"] > 128


@pytest.mark.gpu
def test_gpu_par_full_shape_equals_cpu_serial(gpu_mod, work):
    ref, snap = work.ref(gpu_mod, "full")
    res, gsnap, s = work.run(gpu_mod, "full", "gpu", "par")
    st = s.router_pass_stats()
    print("full:", st)
    assert "blocks=112" in s.output
    assert res == ref and gsnap == snap
    assert st["split_blocks"] == 2 and st["max_packets_req"] > 64 and st["max_packets_rep"] > 64


@pytest.mark.gpu
def test_gpu_par_lock_step_check(gpu_mod, work):
    ref, _ = work.ref(gpu_mod, "small")
    args, kl = work.args("small")
    s = gpu_mod.Simulator(args + _flat(ROUTER) + ["-sim_router_pass", "par", "-sim_engine", "check",
                                                 "-sim_check_interval", "512", "-trace", kl], False)
    assert s.run() == 0 and not s.deadlock
    assert s.tot_cycle == ref[0] and s.router_pass_stats()["split_blocks"] == 2


# Other engine kernel builds, each in a fresh child process, one at a time
# (tests/test_engine_builds.py).  id -> (environment, variant, blocks that
# share the pass): ASIM_GPU_BLOCKS=1 is the smallest cap the engine accepts,
# one block then runs both subnets.
BUILDS = {
    "lds": ({"ASIM_GPU_STATE": "lds"}, "lds", 2),
    "split2": ({"ASIM_GPU_STATE": "split", "ASIM_GPU_SPLIT_WAVES": "2"}, "split2", 2),
    "split_prof": ({"ASIM_GPU_STATE": "split", "ASIM_GPU_PROFILE": "1"}, "split_prof", 2),
    "lds_blocks1": ({"ASIM_GPU_STATE": "lds", "ASIM_GPU_BLOCKS": "1"}, "lds_sliced", 1),
}
_ENGINE_ENV = ("ASIM_GPU_STATE", "ASIM_GPU_SPLIT_WAVES", "ASIM_GPU_BLOCKS", "ASIM_GPU_PROFILE", "ASIM_GPU_BATCH",
               "ASIM_GPU_BLOCKS_PER_CU", "ASIM_GPU_CH_PER_BLOCK", "ASIM_NATIVE_SO")
# about 5x the slowest child measured on an MI355X (lds_blocks1: 4.1 s with the torch import; the others 2.8 s)
CHILD_TIMEOUT_S = 20
_dead = {"why": None}


@pytest.fixture(scope="module")
def build_manifest(gpu_mod, work):
    apps, cpu = [], {}
    for case in ("small", "bp"):
        args, kl = work.args(case)
        icnt = args[args.index("-inter_config_file") + 1]
        extra = dict(SMALL, **{"-network_mode": "1", "-inter_config_file": icnt}, **ROUTER)
        apps.append(dict(name=case, kernelslist=kl, preset="QV100", extra=dict(extra, **{"-sim_router_pass": "par"})))
        ref, snap = work.ref(gpu_mod, case)
        cpu[case] = (ref, hashlib.sha256(snap).hexdigest())
    manifest = str(work.root / "builds_manifest.json")
    with open(manifest, "w") as f:
        json.dump(apps, f)
    return manifest, apps, cpu


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_gpu_par_other_kernel_builds(build_manifest, build):
    if _dead["why"]:
        pytest.fail("not started: an earlier engine-build child " + _dead["why"])
    manifest, apps, cpu = build_manifest
    env_add, variant, split = BUILDS[build]
    env = {k: v for k, v in os.environ.items() if k not in _ENGINE_ENV}
    env.update(env_add)
    cmd = [sys.executable, "-m", "accel_sim_framework_distributed_amd.ops.build_child", manifest, variant]
    t0 = time.perf_counter()
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
    print(build, f"child {time.perf_counter() - t0:.1f} s; wall_s per app:", {g["name"]: g["wall_s"] for g in got})
    for g in got:
        ref, sha = cpu[g["name"]]
        assert g["engine"] == "gpu" and not g["deadlock"] and g["variant"] == variant, g["name"]
        if split == 1:
            assert g["blocks"] == 1, g["blocks"]
        assert (g["tot_cycle"],) + tuple(int(g["stats"][k]) for k in STAT_KEYS) == ref, g["name"]
        assert g["snapshot_sha256"] == sha, g["name"]
        st = g["router_pass"]
        assert st["mode"] == "par" and st["passes"] > 0 and st["split_blocks"] == split, (g["name"], st)
