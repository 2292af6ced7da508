"""-icnt_capture: both cycle engines write every packet they inject into the
network, losslessly and bit-identically (csrc/model/icnt_capture.h), and the
standalone network mode replays the file (icnt/capture.py, icnt/booksim.py).

The machine is the small one of tests/test_router_pass_par.py: QV100 with 16
clusters and 8 memory channels (16 SMs, 16 L2 sub-partitions) on an 8 x 8
mesh, with that file's kernels:
  spread    80 single-warp CTAs, 16 loads each of a line of their own: 1280
            8-byte read requests spread over all sub-partitions, 1280 136-byte
            replies
  stores32  32 full-line stores per CTA behind a 9-flit injection queue (the
            "bp" network): 2560 136-byte requests that the back-pressure holds
            at their SMs
  hot       the same-line hotspot (the "mesh" case): every SM's requests meet
            at one sub-partition
  sthot     a store hotspot of this file: 320 single-warp CTAs store the same
            64 lines, 20480 136-byte writes that meet at a few sub-partitions
            faster than they are served, so that the input queues (256
            entries) overflow into the arrival backlog rings
A mailbox cell never holds more than its capacity (sm_inject and the reply
path stop at out_cap), and a packet enters the destination's backlog ring only
after it left the mailbox, so the mailbox gather sees every packet once.
"""
import collections
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import test_router_pass_par as rpass
from accel_sim_framework_distributed_amd import sim
from accel_sim_framework_distributed_amd.icnt import booksim, capture
from accel_sim_framework_distributed_amd.models import presets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = 16 * 16 * 10  # n_sm * n_subpart * mailbox capacity of the small machine: records per subnet and epoch
MIN_KB = (WORST * 24 + 1023) // 1024


def _stat(out, key):
    return int(re.findall(rf"^{key} = (\d+)", out, re.M)[-1])


def _stats(out):
    return [l for l in out.splitlines() if re.match(r"^[A-Za-z_\[\]0-9 ]+ = [0-9.]+$", l)
            and not re.search("rate|slowdown|time", l)]


def _store_hotspot_app(root):
    from accel_sim_framework_distributed_amd.tracegen import rodinia
    from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder
    k = KernelBuilder("_Z9storehotsPf", (320, 1, 1), (32, 1, 1), nregs=32)
    for i in range(64):
        k.op("STG.E", [], [2, 3], base=np.full(k.g.nwarps, 0x7000_0000 + i * 0x40000, np.int64), stride=4)
    k.op("EXIT")
    return rodinia.write_app(str(root / "sthot"), [k.build()], memcpy=False)


class _Cap:
    """Runs of the small machine with and without capture; the CPU engine's
    files are made once and shared."""

    def __init__(self, root):
        self.root = root
        self.work = rpass._Work(root)
        self._ref = {}
        self.n = 0

    def args(self, case, lc):
        if case == "xbar":  # the local crossbar (-network_mode 2): no topology, no link model
            return presets.args_for("QV100", dict(rpass.SMALL)) + ["-gpgpu_perf_sim_memcpy", "0"], self.work.apps["spread"]
        if case == "sthot":  # the small mesh with the store hotspot
            if "sthot" not in self.work.apps:
                self.work.apps["sthot"] = _store_hotspot_app(self.root)
            args, kl = self.work.args("small")[0], self.work.apps["sthot"]
        else:
            args, kl = self.work.args(case)
        return args + ["-icnt_link_contention", str(lc), "-gpgpu_perf_sim_memcpy", "0"], kl

    def run(self, native, case, lc, engine="cpu", more=(), capture_on=True):
        args, kl = self.args(case, lc)
        self.n += 1
        path = str(self.root / f"{case}_{lc}_{engine}_{self.n}.icap")
        opts = (["-icnt_capture", path] if capture_on else []) + list(more)
        s = native.Simulator(args + opts + ["-sim_engine", engine, "-trace", kl], False)
        assert s.run() == 0 and not s.deadlock, (case, lc)
        data = open(path, "rb").read() if capture_on else None
        return s, path, data

    def ref(self, native, case, lc):
        if (case, lc) not in self._ref:
            s, path, data = self.run(native, case, lc)
            self._ref[(case, lc)] = (path, data, s.tot_cycle, _stats(s.output), bytes(s.snapshot()))
        return self._ref[(case, lc)]


@pytest.fixture(scope="module")
def cap(tmp_path_factory):
    return _Cap(tmp_path_factory.mktemp("icnt_capture"))


LINKS = [("xbar", 0), ("small", 0), ("small", 1), ("small", 2)]


# ---- CPU ---------------------------------------------------------------------
@pytest.mark.parametrize("case,lc", LINKS + [("bp", 2), ("mesh", 2), ("sthot", 0), ("sthot", 2)])
def test_conservation(native, cap, case, lc):
    """Record counts == the simulator's own packet counters: the SMs'
    pkts_out (every request an SM put into a mailbox, sm_inject) and pkts_in
    (every reply an SM took out of its input queue); at the end of a run no
    reply is in flight, so both sides of the reply count agree."""
    s, path, data = cap.run(native, case, lc)
    c = capture.load(path)
    req, rep = _stat(s.output, "icnt_total_pkts_simt_to_mem"), _stat(s.output, "icnt_total_pkts_mem_to_simt")
    print(case, lc, "requests", req, "replies", rep, "file", c.counts)
    assert req >= 256 and rep >= 256
    assert c.counts == (req, rep) == (len(c.request), len(c.reply))
    assert (s.icnt_capture_request_packets, s.icnt_capture_reply_packets) == (req, rep)
    assert len(data) == 64 + 24 * (req + rep)
    if case == "bp":
        # the injection queue stalls the SMs: packets are held back before they reach a mailbox
        assert _stat(s.output, "Req_Network_injection_stall_cycles") > 0
    if case == "sthot":
        # packets wait in the sub-partitions' arrival backlog rings (the overflow path behind the
        # mailboxes) and are still recorded exactly once
        assert req == 320 * 64
        assert _stat(s.output, "icnt_mem_input_backlog") > 0


def _epochs(sub, n_sm, n_subpart, reply):
    """The stream cut where the mailbox cell index falls: within an epoch the
    records come in cell, then slot order, so a fall starts a new epoch (two
    epochs whose cells happen to rise across the boundary stay one piece,
    which only makes the checks on the pieces stricter)."""
    src, dst = sub.src.astype(np.int64), sub.dst.astype(np.int64)
    # request cell = sub * n_sm + sm, reply cell = sm * n_subpart + sub (rt_cell); one SM per cluster here
    cell = ((dst - n_sm) * n_sm + src) if not reply else (dst * n_subpart + (src - n_sm))
    cuts = np.nonzero(np.diff(cell) < 0)[0] + 1
    return np.split(np.arange(len(cell)), cuts)


def test_content_against_the_trace(native, cap):
    """spread: CTA c's load i reads the line 0x70000000 + c * 0x100000 +
    i * 128: an 8-byte read request to the sub-partition addr_decode names, and
    a 136-byte reply back.  The 80 single-warp CTAs all fit the 16 SMs at
    once, five whole CTAs per SM; every SM is its own cluster, so node = SM.
    Which five is the dispatcher's choice, but the address map leaves the CTAs
    only a few distinct destination multisets, so the (src, dst, bytes)
    multiset is pinned down: every source's requests are five CTAs' worth of
    ONE such multiset, and each multiset is used by as many sources as its
    CTAs need."""
    path, _, _, _, _ = cap.ref(native, "small", 2)
    args, _ = cap.args("small", 2)
    c = capture.load(path)
    assert (c.nodes, c.n_clusters, c.n_subpart, c.flit_size) == (64, 16, 16, 40)
    cfg = native.parse_config(args)
    assert cfg["n_clusters"] == c.n_clusters and cfg["n_subpart"] == c.n_subpart
    pattern = collections.Counter()  # destination multiset of a CTA -> CTAs that have it
    for cta in range(80):
        dsts = sorted(c.n_clusters + native.addr_decode(args, 0x7000_0000 + cta * 0x100000 + i * 128)["sub"]
                      for i in range(16))
        pattern[tuple(dsts)] += 1
    assert len({d for pat in pattern for d in pat}) > 8  # spread over the sub-partitions
    assert all(n % 5 == 0 for n in pattern.values())
    q, p = c.request, c.reply
    assert set(q.bytes.tolist()) == {8} and set(p.bytes.tolist()) == {136}
    by_src = collections.defaultdict(list)
    for s_, d_ in zip(q.src.tolist(), q.dst.tolist()):
        by_src[s_].append(d_)
    assert sorted(by_src) == list(range(16))
    used = collections.Counter()
    for s_, dsts in by_src.items():
        assert len(dsts) == 5 * 16, s_
        pat = tuple(sorted(dsts)[::5])
        assert tuple(sorted(dsts)) == tuple(sorted(pat * 5)) and pat in pattern, s_
        used[pat] += 5
    assert used == pattern
    # every request is answered over the reverse pair by a full line with its header
    assert collections.Counter(zip(p.dst.tolist(), p.src.tolist())) == collections.Counter(zip(q.src.tolist(), q.dst.tolist()))
    assert set(q.type.tolist()) == {1} and set(p.type.tolist()) == {4}  # P_RD, P_RD_REPLY
    for reply, s in ((False, q), (True, p)):
        assert (s.flits == (s.bytes + c.flit_size - 1) // c.flit_size).all()
        assert (s.flits == capture.flits_for(s.bytes, c.flit_size)).all()
        # tinj is non-decreasing across epochs: no epoch starts its injections before the one
        # before it did, and a one-flit packet (injected in the cycle it is sent) is never later
        # than any packet of the next epoch
        t = s.tinj.astype(np.int64)
        ep = _epochs(s, c.n_clusters, c.n_subpart, reply)
        assert len(ep) > 20
        lo = np.array([t[e].min() for e in ep]), np.array([t[e].max() for e in ep])
        assert (np.diff(lo[0]) >= 0).all()
        if not reply:
            assert (lo[1][:-1] <= lo[0][1:]).all()


@pytest.mark.parametrize("case,lc", LINKS)
def test_capture_changes_nothing(native, cap, case, lc):
    """Cycles, statistics and the state image with capture on equal those with
    capture off."""
    _, _, cyc, stats, snap = cap.ref(native, case, lc)
    s, _, _ = cap.run(native, case, lc, capture_on=False)
    assert len(stats) > 20
    assert (s.tot_cycle, _stats(s.output), bytes(s.snapshot())) == (cyc, stats, snap)


@pytest.mark.parametrize("lc", [1, 2])
def test_tinj_is_read_before_the_pass(native, cap, lc):
    """The contention passes add their delay to Pkt::t in place; the capture
    must not see it.  The hotspot kernel sends every SM's requests to one
    sub-partition, so the pass delays packets in the very first epoch that has
    any; and up to that epoch's boundary nothing a link model does can have
    reached an SM, so the SMs inject exactly as in the contention-free run:
    the first epoch's records are the same in both files, injection times
    included, although the pass did delay some of them (the run with the
    model ends later, and the model counts delayed packets)."""
    p0, _, cyc0, _, _ = cap.ref(native, "mesh", 0)
    p1, _, cyc1, stats1, _ = cap.ref(native, "mesh", lc)
    assert any(l.startswith("Network_link_delayed_packets") and int(l.split("=")[1]) > 0 for l in stats1)
    a, b = capture.load(p0), capture.load(p1)
    first = _epochs(a.request, a.n_clusters, a.n_subpart, False)[0]
    n = len(first)
    assert n >= 16  # every SM has injected
    for k in ("src", "dst", "bytes", "tinj"):
        assert (getattr(a.request, k)[:n] == getattr(b.request, k)[:n]).all(), k


def test_invariance(native, cap):
    """The file is byte-identical across the serial and the lane-parallel
    router pass, 1 and 4 CPU threads, and the default and the smallest log."""
    _, ref, _, _, _ = cap.ref(native, "small", 2)
    for more in (["-sim_router_pass", "par"], ["-sim_cpu_threads", "4"],
                 ["-sim_router_pass", "par", "-sim_cpu_threads", "4"],
                 ["-icnt_capture_buf_kb", str(MIN_KB)],
                 ["-icnt_capture_buf_kb", str(MIN_KB), "-sim_cpu_threads", "3"]):
        _, _, data = cap.run(native, "small", 2, more=more)
        assert data == ref, more
    for case, lc in (("small", 0), ("small", 1), ("xbar", 0)):
        _, ref, _, _, _ = cap.ref(native, case, lc)
        _, _, data = cap.run(native, case, lc, more=["-sim_cpu_threads", "4", "-icnt_capture_buf_kb", str(MIN_KB)])
        assert data == ref, (case, lc)


def test_small_log_is_refused(native, cap):
    args, kl = cap.args("small", 2)
    assert MIN_KB * 1024 // 24 >= WORST > (MIN_KB - 1) * 1024 // 24  # one KB less is at least one record short
    with pytest.raises(ValueError, match=rf"-icnt_capture_buf_kb {MIN_KB - 1}: .*{WORST} records per subnet: at least {MIN_KB} KB"):
        native.Simulator(args + ["-icnt_capture", str(cap.root / "refused.icap"), "-icnt_capture_buf_kb", str(MIN_KB - 1),
                                 "-trace", kl], False)
    with pytest.raises(Exception, match="needs -icnt_capture"):
        native.Simulator(args + ["-icnt_capture_buf_kb", "64", "-trace", kl], False)


def test_loader_rejects_bad_files(native, cap, tmp_path):
    _, data, _, _, _ = cap.ref(native, "small", 2)
    for name, blob in (("truncated", data[:-7]), ("short_record", data[:-24]), ("header_only_part", data[:40]),
                       ("empty", b""), ("magic", b"NOTACAPT" + data[8:]), ("version", data[:8] + b"\x09" + data[9:]),
                       ("overlong", data + b"\0" * 24)):
        p = tmp_path / name
        p.write_bytes(blob)
        with pytest.raises(ValueError):
            capture.load(str(p))
    assert not capture.is_capture(str(tmp_path / "magic")) and capture.is_capture(str(tmp_path / "truncated"))


def test_python_api_and_check_engine(native, cap):
    """simulate(..., icnt_capture=path) writes the same file and reports the
    counts; -sim_engine check writes its primary engine's capture."""
    _, ref, cyc, _, _ = cap.ref(native, "small", 2)
    args, kl = cap.work.args("small")
    icnt = args[args.index("-inter_config_file") + 1]
    extra = dict(rpass.SMALL, **{"-network_mode": "1", "-inter_config_file": icnt, "-icnt_link_contention": "2",
                                 "-gpgpu_perf_sim_memcpy": "0"})
    p = str(cap.root / "api.icap")
    r = sim.simulate(kl, "QV100", "cpu", extra, icnt_capture=p)
    assert r.tot_cycle == cyc and open(p, "rb").read() == ref
    assert (r.icnt_capture_request_packets, r.icnt_capture_reply_packets) == (1280, 1280)
    assert sim.simulate(kl, "QV100", "cpu", extra).icnt_capture_request_packets == 0
    _, _, data = cap.run(native, "small", 2, engine="check", more=["-sim_check_primary", "cpu", "-sim_check_interval", "512"])
    assert data == ref


def test_resumed_run_captures_from_the_resume_point(native, tmp_path):
    """Capture state is not part of a checkpoint: the run that writes one
    captures all of its packets, and a run resumed at kernel 2 captures from
    there on, the tail of the uninterrupted run's file."""
    from accel_sim_framework_distributed_amd.tracegen import rodinia
    kl = rodinia.write_app(str(tmp_path / "pf"), rodinia.pathfinder(4000, 12, 2))
    mesh = rpass._icnt_args(tmp_path, "mesh", **rpass.MESH) + ["-icnt_link_contention", "2", "-trace", kl]
    ck = ["-checkpoint_path", str(tmp_path / "ck")]

    def run(name, more):
        p = str(tmp_path / name)
        s = native.Simulator(mesh + more + ["-icnt_capture", p], False)
        assert s.run() == 0
        return capture.load(p), open(p, "rb").read(), bytes(s.snapshot())
    full, full_bytes, snap = run("full", [])
    _, first_bytes, _ = run("first", ck + ["-checkpoint_option", "1", "-checkpoint_kernel", "2"])
    assert first_bytes == full_bytes
    rest, _, rsnap = run("rest", ck + ["-resume_option", "1", "-resume_kernel", "2"])
    assert rsnap == snap
    for sub in capture.SUBNETS:
        f, r = full.subnet(sub), rest.subnet(sub)
        n = len(r)
        assert 0 < n < len(f)
        for k in ("src", "dst", "bytes", "flits", "tinj", "type"):
            assert (getattr(f, k)[-n:] == getattr(r, k)).all(), (sub, k)


def _cli(argv, tmp_path, name):
    out = tmp_path / name
    assert booksim.main(argv + ["--json", str(out)]) == 0
    return json.loads(out.read_text())


def test_round_trip_through_npz(native, cap, tmp_path):
    """load -> save_npz -> booksim --replay on the .npz == --replay on the
    capture file, per subnet; --subnet both gives both results."""
    path, _, _, _, _ = cap.ref(native, "small", 2)
    args, _ = cap.work.args("small")
    icnt = args[args.index("-inter_config_file") + 1]
    c = capture.load(path)
    both = _cli([icnt, "--replay", path, "--subnet", "both"], tmp_path, "both.json")
    assert [b["subnet"] for b in both] == ["request", "reply"]
    for i, sub in enumerate(capture.SUBNETS):
        npz = str(tmp_path / f"{sub}.npz")
        capture.save_npz(npz, c, sub)
        with np.load(npz) as z:
            assert (z["flits"] == c.subnet(sub).flits).all() and (z["bytes"] == c.subnet(sub).bytes).all()
        a = _cli([icnt, "--replay", npz], tmp_path, f"{sub}_npz.json")
        b = _cli([icnt, "--replay", path, "--subnet", sub], tmp_path, f"{sub}_cap.json")
        assert set(a) == {"config", "replay", "result"}  # the .npz path's output is what it was
        assert a["result"] == b["result"] == both[i]["result"]
        assert a["result"]["packets"] == c.counts[i] and a["result"]["avg_latency"] > 0
    # other flit sizes: save_npz recomputes on request
    capture.save_npz(str(tmp_path / "f16.npz"), c, "reply", flit_size=16)
    with np.load(str(tmp_path / "f16.npz")) as z:
        assert set(z["flits"].tolist()) == {9}  # ceil(136 / 16)
    with pytest.raises(ValueError):
        c.subnet("neither")


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


def _launches(out):
    return int(re.findall(r"^engine_kernel_launches: (\d+)", out, re.M)[-1])


GPU_RUNS = [("xbar", 0, []), ("small", 0, []), ("small", 1, []), ("small", 2, ["-sim_router_pass", "serial"]),
            ("small", 2, ["-sim_router_pass", "par"])]


@pytest.mark.gpu
@pytest.mark.parametrize("case,lc,more", GPU_RUNS + [("sthot", 0, [])], ids=lambda v: "_".join(v) if isinstance(v, list) else str(v))
def test_gpu_file_equals_cpu_file(gpu_mod, cap, case, lc, more):
    """Default (split) engine kernel: the GPU engine's file == the CPU
    engine's, byte for byte, and the run equals the one without capture."""
    _, ref, cyc, stats, snap = cap.ref(gpu_mod, case, lc)
    s, _, data = cap.run(gpu_mod, case, lc, engine="gpu", more=more)
    assert "engine_kernel_variant: split " in s.output
    assert data == ref
    assert (s.tot_cycle, _stats(s.output), bytes(s.snapshot())) == (cyc, stats, snap)
    off, _, _ = cap.run(gpu_mod, case, lc, engine="gpu", more=more, capture_on=False)
    assert (off.tot_cycle, _stats(off.output), bytes(off.snapshot())) == (cyc, stats, snap)


@pytest.mark.gpu
def test_gpu_smallest_log_takes_many_launches(gpu_mod, cap):
    """One epoch per launch: the log holds exactly one worst-case epoch."""
    _, ref, cyc, _, snap = cap.ref(gpu_mod, "small", 2)
    s, _, data = cap.run(gpu_mod, "small", 2, engine="gpu",
                         more=["-sim_router_pass", "par", "-icnt_capture_buf_kb", str(MIN_KB)])
    print("launches", _launches(s.output))
    assert data == ref and s.tot_cycle == cyc and bytes(s.snapshot()) == snap
    assert _launches(s.output) > 100
    args, kl = cap.args("small", 2)
    with pytest.raises(ValueError, match=f"at least {MIN_KB} KB"):
        gpu_mod.Simulator(args + ["-icnt_capture", str(cap.root / "r.icap"), "-icnt_capture_buf_kb", str(MIN_KB - 1),
                                  "-sim_engine", "gpu", "-trace", kl], False)


@pytest.mark.gpu
def test_gpu_lock_step_check_writes_the_primary_capture(gpu_mod, cap):
    _, ref, _, _, _ = cap.ref(gpu_mod, "small", 2)
    _, _, data = cap.run(gpu_mod, "small", 2, engine="check", more=["-sim_check_interval", "512"])
    assert data == ref


# Other engine kernel builds, each in a fresh child process, one at a time
# (tests/test_engine_builds.py)
BUILDS = {
    "split2": ({"ASIM_GPU_STATE": "split", "ASIM_GPU_SPLIT_WAVES": "2"}, "split2"),
    "lds": ({"ASIM_GPU_STATE": "lds"}, "lds"),
    "global": ({"ASIM_GPU_STATE": "global"}, "global"),
}
_dead = {"why": None}


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_gpu_other_kernel_builds(gpu_mod, cap, build):
    """split2: link contention 0, 1 and 2 (serial and par); lds and global:
    one short case each (the router model, lane-parallel pass)."""
    if _dead["why"]:
        pytest.fail("not started: an earlier engine-build child " + _dead["why"])
    env_add, variant = BUILDS[build]
    runs = GPU_RUNS[1:] if build == "split2" else GPU_RUNS[-1:]
    apps, want = [], []
    for i, (case, lc, more) in enumerate(runs):
        args, kl = cap.work.args(case)
        icnt = args[args.index("-inter_config_file") + 1]
        extra = dict(rpass.SMALL, **{"-network_mode": "1", "-inter_config_file": icnt, "-icnt_link_contention": str(lc),
                                     "-gpgpu_perf_sim_memcpy": "0",
                                     "-icnt_capture": str(cap.root / f"child_{build}_{i}.icap")})
        extra.update(dict(zip(more[::2], more[1::2])))
        apps.append(dict(name=f"{case}_{lc}_{i}", kernelslist=kl, preset="QV100", extra=extra))
        _, ref, cyc, _, snap = cap.ref(gpu_mod, case, lc)
        want.append((cyc, hashlib.sha256(snap).hexdigest(), hashlib.sha256(ref).hexdigest()))
    manifest = str(cap.root / f"manifest_{build}.json")
    with open(manifest, "w") as f:
        json.dump(apps, f)
    env = {k: v for k, v in os.environ.items() if k not in rpass._ENGINE_ENV}
    env.update(env_add)
    cmd = [sys.executable, "-m", "accel_sim_framework_distributed_amd.ops.build_child", manifest, variant]
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=rpass.CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _dead["why"] = f"({build}) did not finish in {rpass.CHILD_TIMEOUT_S} s"
        pytest.fail("engine-build child " + _dead["why"])
    if p.returncode < 0:
        _dead["why"] = f"({build}) died by signal {-p.returncode}"
        pytest.fail("engine-build child " + _dead["why"] + "\n" + p.stderr[-2000:])
    assert p.returncode == 0, p.stderr[-2000:]
    got = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    print(build, f"child {time.perf_counter() - t0:.1f} s; wall_s per app:", {g["name"]: g["wall_s"] for g in got})
    assert [g["name"] for g in got] == [a["name"] for a in apps]
    for g, (cyc, snap_sha, cap_sha) in zip(got, want):
        assert g["engine"] == "gpu" and not g["deadlock"] and g["variant"] == variant, g["name"]
        assert (g["tot_cycle"], g["snapshot_sha256"]) == (cyc, snap_sha), g["name"]
        assert g["icnt_capture_sha256"] == cap_sha, g["name"]


@pytest.mark.gpu
def test_gpu_capture_then_network_sweep(gpu_mod, cap, tmp_path):
    """End to end: capture on the GPU engine, then --replay --networks on the
    gpu engine; the results equal the cpu engine's."""
    _, path, data = cap.run(gpu_mod, "small", 2, engine="gpu")
    assert data == cap.ref(gpu_mod, "small", 2)[1]
    nets = []
    for name, kw in (("mesh", dict(k=8, n=2, topology="mesh")), ("mesh16", dict(k=8, n=2, topology="mesh", flit_size=16)),
                     ("torus", dict(k=8, n=2, topology="torus", num_vcs=2))):
        f = tmp_path / f"{name}.icnt"
        f.write_text(presets.render_icnt(presets.icnt_params(**kw)))
        nets.append(str(f))
    argv = ["--replay", path, "--subnet", "both", "--networks", ",".join(nets)]
    g = _cli(argv + ["--engine", "gpu"], tmp_path, "gpu.json")
    c = _cli(argv + ["--engine", "cpu"], tmp_path, "cpu.json")
    assert len(g) == 6 and [x["result"] for x in g] == [x["result"] for x in c]
    # the flit size matters where packets are larger than a flit: the 136-byte replies (results 3..5)
    assert g[0]["result"]["avg_latency"] == g[1]["result"]["avg_latency"]  # 8-byte requests: one flit either way
    assert g[3]["result"]["avg_latency"] != g[4]["result"]["avg_latency"]
