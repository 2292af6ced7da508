"""Seeded differential fuzzing of kernels and model configurations
(accel_sim_framework_distributed_amd/tracegen/fuzz.py).

Every pinned case is two random kernels under a random QV100 configuration
(schedulers, partition hashes, cores per cluster, cache policies, collectors,
register banks ...), one case is wave64 on the whole MI355X preset.

CPU (no marker): the case completes, event skipping is exact, the CPU engine
checked against itself in lock step agrees with the plain run, the case stays
within the cycle cap that bounds the GPU tests' run time, and the pinned set
covers every option value the generator draws.
GPU: the lock-step checker compares the HIP engine's state with the CPU
engine's every 256 cycles (a failure names cycle, unit and byte), and a plain
GPU-engine run prints the CPU engine's statistics.
"""
import re

import pytest

from accel_sim_framework_distributed_amd import sim
from accel_sim_framework_distributed_amd.tracegen import fuzz

CYCLE_CAP = 60_000
WALL = re.compile(r"rate|slowdown|time|sec|skipped|epochs", re.I)
IDS = [c.id for c in fuzz.CASES]


def _printed(out):
    """key = value lines without wall-clock / diagnostic ones (tests/test_event_skip.py)."""
    kv = []
    for line in out.splitlines():
        m = re.match(r"^\s*([A-Za-z_][\w\[\]\.:\- ]*?)\s*=\s*(.+)$", line)
        if m and not WALL.search(m.group(1)):
            kv.append((m.group(1), m.group(2).strip()))
    return kv


def _strip(stats):
    return {k: v for k, v in stats.items() if "rate" not in k and "slowdown" not in k and "time" not in k}


def _summary(r):
    return (r.tot_cycle, r.tot_insn, [k["cycles"] for k in r.kernels])


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """case id -> (kernelslist, preset, extra, CPU engine result); each CPU
    reference run happens once and is shared by every test of the case.
    (Not built on the `native` fixture: a session fixture is set up before
    `gpu_mod`, which must import torch before the native module loads.)"""
    root = tmp_path_factory.mktemp("fuzz")
    cache = {}

    def get(case):
        if case.id not in cache:
            kl = fuzz.write_case(str(root / case.id), case)
            preset, extra = fuzz.case_config(case)
            cache[case.id] = (kl, preset, extra, sim.simulate(kl, preset, engine="cpu", extra=extra))
        return cache[case.id]

    return get


def test_generator_is_deterministic():
    a, b = fuzz.case_kernels(fuzz.Case(16)), fuzz.case_kernels(fuzz.Case(16))
    assert fuzz.arrays_sha256(a) == fuzz.arrays_sha256(b)
    assert fuzz.arrays_sha256(a) == GOLDEN_CASE_16
    assert fuzz.config(16) == fuzz.config(16) and fuzz.config(16) != fuzz.config(17)


def test_generator_shapes():
    """What fuzz.kernel() promises: 12-40 ops + EXIT, 3-40 CTAs of 32-512
    threads, partial warps, every unit class over the pinned set."""
    names, partial = set(), False
    for c in fuzz.CASES:
        for k in fuzz.case_kernels(c):
            h = k.header
            threads = h["block"][0]
            assert 32 <= threads <= 512 and (c.preset == "MI355X" or 3 <= h["grid"][0] <= 40)
            per_warp = k.streams["count"]
            assert per_warp.max() <= 41 and per_warp.min() >= 1
            partial |= threads % h["warp_size"] != 0
            names |= set(k.opnames)
    assert partial
    for m in ("FFMA", "IMAD", "DFMA", "MUFU.RCP", "HMMA.1688.F32", "LDG.E", "STG.E", "LDS", "STS", "LDL", "LDC",
              "ATOMG.E.ADD.STRONG.GPU", "BAR.SYNC", "MEMBAR.GL", "ds_read_b32", "global_load_dword", "s_barrier"):
        assert m in names, m


def test_pinned_cases_cover_every_option_value():
    """Pruning the pinned list must not lose an option value unnoticed."""
    assert len(fuzz.CASES) >= 12 and len(set(IDS)) == len(IDS)
    assert any(c.preset == "MI355X" for c in fuzz.CASES)
    cfgs = [fuzz.config(c.seed) for c in fuzz.CASES if c.preset == "QV100"]
    seen = lambda key: {c[key] for c in cfgs}
    assert seen("-gpgpu_scheduler") == set(fuzz.SCHEDULERS)
    assert seen("-gpgpu_memory_partition_indexing") == {"0", "1", "2", "3", "4"}
    assert "2" in seen("-gpgpu_n_cores_per_cluster")
    assert seen("-gpgpu_n_sub_partition_per_mchannel") == {"1", "2"}
    assert seen("-gpgpu_cache:dl1") == set(fuzz.DL1.values())
    assert seen("-gpgpu_cache:dl2") == set(fuzz.DL2.values())
    assert seen("-gpgpu_dram_scheduler") == {"0", "1"}
    assert "0" in seen("-gpgpu_perfect_inst_const_cache")
    assert "2" in seen("-gpgpu_max_insn_issue_per_warp")
    assert "2" in seen("-gpgpu_operand_collector_num_units_gen")
    assert "4" in seen("-gpgpu_num_reg_banks")
    assert all(c["-gpgpu_perf_sim_memcpy"] == "0" for c in cfgs)
    assert all(c in fuzz.CASES for c in fuzz.BUILD_CASES)


@pytest.mark.parametrize("case", fuzz.CASES, ids=IDS)
def test_case_completes_within_cycle_cap(native, cases, case):
    """No deadlock, and at most 60,000 cycles: at the measured ~15.6 us of
    MI355X time per busy simulated cycle that bounds one GPU engine run of the
    case at about a second (a condition on the pinned set, not a measurement)."""
    c = cases(case)[3]
    assert not c.deadlock and c.tot_insn > 0
    assert 0 < c.tot_cycle <= CYCLE_CAP
    assert len(c.kernels) == 2


@pytest.mark.parametrize("case", fuzz.CASES, ids=IDS)
def test_case_event_skip_is_exact(native, cases, case):
    kl, preset, extra, on = cases(case)
    off = sim.simulate(kl, preset, engine="cpu", extra=dict(extra, **{"-sim_event_skip": "0"}))
    assert _summary(off) == _summary(on)
    a, b = _printed(on.output), _printed(off.output)
    assert len(a) > 50
    assert a == b, [(x, y) for x, y in zip(a, b) if x != y][:5]


@pytest.mark.parametrize("case", fuzz.CASES, ids=IDS)
def test_case_cpu_self_check(native, cases, case):
    kl, preset, extra, c = cases(case)
    k = sim.simulate(kl, preset, engine="check",
                     extra=dict(extra, **{"-sim_check_primary": "cpu", "-sim_check_interval": "64"}))
    assert not k.deadlock
    assert _summary(k) == _summary(c)
    assert _strip(k.stats) == _strip(c.stats)


# ---- GPU engine ------------------------------------------------------------

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
@pytest.mark.parametrize("case", fuzz.CASES, ids=IDS)
def test_case_gpu_equals_cpu(gpu_mod, cases, case):
    kl, preset, extra, c = cases(case)
    # lock step: a divergence raises "engine check failed at cycle ..." with the unit and byte
    k = sim.simulate(kl, preset, engine="check", extra=dict(extra, **{"-sim_check_interval": "256"}))
    assert _summary(k) == _summary(c)
    g = sim.simulate(kl, preset, engine="gpu", extra=extra)
    assert g.engine == "gpu" and not g.deadlock
    assert _summary(g) == _summary(c)
    assert _strip(g.stats) == _strip(c.stats)


GOLDEN_CASE_16 = "3788f460a8248bd7283ba1125bd2b4f4ef1b3da031cb949b04e74428c7795a79"
