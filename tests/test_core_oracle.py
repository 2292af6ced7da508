"""The SM compute pipeline, cycle for cycle, against a plain-Python oracle.

Both engines instantiate the templates of csrc/model/sm.h, so "GPU == CPU"
cannot see a wrong rule there.  This file holds a second, independent model of
one SM's compute pipeline -- fetch, the warp schedulers, the scoreboard, the
ID_OC registers, operand collectors and register-file banks, the functional
units with their initiation intervals, the result bus, the LDS path of the
LD/ST unit, barriers and retirement -- written in plain integer Python from the
rules stated in the comments of sm.h / config.h (and, where those are silent,
from the reference's shader.cc scheduler_unit::cycle, opndcoll_rfu_t and
scoreboard.cc), and compares it with the engines

  a. event for event on the WARP_SCHEDULER stream (every issue: cycle, SM,
     warp, PC, in scheduler order within a cycle) -- the sequential issue loop;
  b. event for event on the SCOREBOARD stream alone (every ALU result: cycle,
     warp, register), which leaves the lane-parallel issue path switched on;
  c. on every statistic the pipeline produces, with and without a stream and
     with -sim_event_skip 0 and 1.

The oracle follows the two documented differences from the reference, S1
(scheduler start-up: "last issued" starts as warp 0) and S2 (latencies of 512
and more are refused when the configuration is loaded), see sm.h's header.

Scope: nothing leaves the SM.  No global / local / constant memory, perfect
instruction cache.  CTA dispatch happens at epoch boundaries (epoch.h); of
that the oracle models the time anchor L (see anchor()) and the dispatch rule
alone (at an epoch's start, round-robin rounds over the SMs with room).  Every
grid fits in one wave, except in the three "waves" cases: only a second wave
puts a younger CTA into lower warp slots than an older one, which is what
tells warp age from warp order for GTO, oldest-first and warp-limiting.

The oracle reads its parameters from the option strings and has its own
mnemonic table; it never looks at parse_config, Simulator.config or
decode_opcode.
"""
import random
import re
import time
from collections import Counter

import numpy as np
import pytest

from accel_sim_framework_distributed_amd.models import presets
from accel_sim_framework_distributed_amd.tracegen import rodinia
from accel_sim_framework_distributed_amd.tracegen.builder import KernelBuilder

# ---------------------------------------------------------------------------
# oracle: static tables
# ---------------------------------------------------------------------------
# fixed sizes named in config.h
K_IBUF = 2          # instruction buffer entries per warp
K_LOAD_SLOTS = 8    # loads in flight per warp
K_HIT_SLOT = 8      # LDS completions per cycle
K_HIT_RING = 256
K_WB_RING = 512     # writeback ring: latencies up to 511
K_WB_SLOT = 8       # EX_WB width cap
K_MAX_OC = 16

# ID_OC registers are visited in (scheduler, unit) order; this is the unit order
UNITS = ("SP", "DP", "INT", "SFU", "TENSOR", "MEM")

# mnemonic -> (class, kind).  kind: "alu" goes down the pipeline to a unit,
# "ld" / "st" are LDS accesses, the rest are handled at issue.
MNEMONICS = {
    "MOV": ("ALU", "alu"), "IMAD": ("INTP", "alu"), "FFMA": ("SP", "alu"), "DFMA": ("DP", "alu"),
    "MUFU.RCP": ("SFU", "alu"), "LDS": ("LOAD", "ld"), "STS": ("STORE", "st"),
    "BAR.SYNC": ("BARRIER", "bar"), "MEMBAR.GL": ("MEMBAR", "membar"), "EXIT": ("EXIT", "exit"),
    "NOP": ("NOP", "nop"),
    "v_fma_f32": ("SP", "alu"), "v_fma_f64": ("DP", "alu"), "v_rcp_f32": ("SFU", "alu"),
    "s_add_u32": ("INTP", "alu"), "v_mfma_f32_32x32x16_bf16": ("TENSOR", "alu"),
    "ds_read_b32": ("LOAD", "ld"), "ds_write_b32": ("STORE", "st"), "s_waitcnt": ("NOP", "waitcnt"),
    "s_barrier": ("BARRIER", "bar"), "s_endpgm": ("EXIT", "exit"), "s_nop": ("NOP", "nop"),
}
# which -trace_opcode_latency_initiation_* option times a class
LAT_OPTION = {"ALU": "int", "INTP": "int", "SP": "sp", "DP": "dp", "SFU": "sfu", "TENSOR": "tensor"}
NO_WAIT = 0xFF      # an s_waitcnt counter that is not waited for


def popc(x):
    return bin(x).count("1")


class CoreCfg:
    """the pipeline's parameters, from the option strings"""

    def __init__(self, o):
        thr, ws = o["-gpgpu_shader_core_pipeline"].split(":")[:2]
        self.warp_size = int(ws)
        self.nw = int(thr) // int(ws)                      # warp slots of an SM
        self.n_sm = int(o["-gpgpu_n_clusters"]) * int(o["-gpgpu_n_cores_per_cluster"])
        self.epoch = int(o["-icnt_latency"])
        self.nsched = max(1, int(o["-gpgpu_num_sched_per_core"]))
        f = o["-gpgpu_scheduler"].split(":")
        self.policy = {"lrr": "lrr", "gto": "gto", "old": "old", "rrr": "rrr", "two_level_active": "2lv",
                       "warp_limiting": "swl"}[f[0]]
        self.sched_param = int(f[1]) if self.policy == "2lv" else int(f[2]) if self.policy == "swl" else 0
        self.sub_core = int(o["-gpgpu_sub_core_model"])
        assert int(o["-gpgpu_enable_specialized_operand_collector"]) == 0
        self.noc = min(max(1, int(o["-gpgpu_operand_collector_num_units_gen"])), K_MAX_OC)
        self.banks = max(1, int(o["-gpgpu_num_reg_banks"]))
        self.port_tp = max(1, int(o["-gpgpu_reg_file_port_throughput"]))
        self.units = {"SP": int(o["-gpgpu_num_sp_units"]), "DP": int(o["-gpgpu_num_dp_units"]),
                      "INT": int(o["-gpgpu_num_int_units"]), "SFU": int(o["-gpgpu_num_sfu_units"]),
                      "TENSOR": int(o["-gpgpu_num_tensor_core_units"]) if int(o["-gpgpu_tensor_core_avail"]) else 0,
                      "MEM": 1}
        self.wb_width = min(max(1, int(o["-gpgpu_pipeline_widths"].split(",")[10])), K_WB_SLOT)
        self.lat = {}
        for name in set(LAT_OPTION.values()):
            lat, ii = o["-trace_opcode_latency_initiation_" + name].split(",")[:2]
            self.lat[name] = (int(lat), max(1, int(ii)))
        self.smem_latency = int(o["-gpgpu_smem_latency"])
        assert "-smem_latency" not in o and self.smem_latency < K_HIT_RING
        self.interval = max(1, int(o["-gpgpu_warp_issue_interval"]))
        self.max_issue = max(1, int(o["-gpgpu_max_insn_issue_per_warp"]))
        self.dual_diff = int(o["-gpgpu_dual_issue_diff_exec_units"])
        self.fetch_tp = max(1, int(o["-gpgpu_inst_fetch_throughput"]))
        self.single_valu = int(o["-sim_single_valu"])
        self.smem_banks = int(o["-gpgpu_shmem_num_banks"])
        # what the oracle's LDS conflict degree assumes
        assert int(o["-gpgpu_shmem_warp_parts"]) == 1 and int(o["-gpgpu_shmem_limited_broadcast"]) == 0
        assert int(o["-gpgpu_shmem_cdna_lane_groups"]) == 0 and int(o["-sim_lds_port_bytes"]) == 0
        # the time anchor and the scope of the oracle
        assert int(o["-gpgpu_kernel_launch_latency"]) == 0 and int(o["-gpgpu_TB_launch_latency"]) == 0
        assert int(o["-gpgpu_perfect_inst_const_cache"]) == 1

    def unit_of(self, cls):
        """config.h: with -sim_single_valu the INT / DP / SFU classes share the
        SP unit; DP work goes to the SFU unit when there is no DP unit, INT and
        tensor work to SP when theirs are absent"""
        if self.single_valu and cls in ("SFU", "DP", "INTP"):
            return "SP"
        if cls in ("LOAD", "STORE", "MEMBAR"):
            return "MEM"
        if cls == "SFU":
            return "SFU"
        if cls == "DP":
            return "DP" if self.units["DP"] else "SFU"
        if cls == "INTP":
            return "INT" if self.units["INT"] else "SP"
        if cls == "TENSOR":
            return "TENSOR" if self.units["TENSOR"] else "SP"
        return "SP"

    def sched_of(self, w):
        return w % self.nsched

    def reg_bank(self, sched, warp, reg):
        """register `reg` (0-based) of `warp`: banks interleave by reg + warp;
        in the sub-core model each scheduler owns banks / n_sched of them"""
        if self.sub_core:
            per = max(self.banks // self.nsched, 1)
            return (sched * per) % self.banks + (reg + warp) % per
        return (reg + warp) % self.banks

    def collectors_of(self, sched):
        if self.sub_core:
            per = max(self.noc // self.nsched, 1)
            lo = (sched * per) % self.noc
            return range(lo, min(lo + per, self.noc))
        return range(self.noc)


class OInst:
    """one dynamic warp instruction as the oracle sees it"""

    def __init__(self, cfg, pc, mn, dst, src, lanes, deg=1, wait=None):
        self.pc, self.mn, self.lanes = pc, mn, lanes
        self.cls, self.kind = MNEMONICS[mn]
        self.dst = tuple(r + 1 for r in dst)               # register + 1, as the scoreboard keys them
        self.src = tuple(r + 1 for r in src)
        self.special = self.kind not in ("alu", "ld", "st")
        self.unit = cfg.unit_of(self.cls)
        self.lat, self.ii = cfg.lat[LAT_OPTION[self.cls]] if self.kind == "alu" else (1, 1)
        self.deg = deg                                      # LDS conflict degree
        self.wait = wait                                    # s_waitcnt (vm, lgkm)


class OWarp:
    def __init__(self, prog, age, cta):
        self.prog, self.age, self.cta = prog, age, cta
        self.head = 0           # next instruction to issue
        self.next = 0           # next instruction to fetch
        self.ibuf = 0
        self.exiting = self.barrier = self.waitcnt = False
        self.inflight = 0
        self.sb = set()         # pending destination registers (+1)
        self.slots = [None] * K_LOAD_SLOTS   # in-flight loads: their destination registers
        self.lds_st = 0
        self.wait = (0, 0)
        self.issue_ok = 0

    def parked(self):
        return self.exiting or self.barrier or self.waitcnt

    def loads(self):
        return sum(s is not None for s in self.slots)

    def waitcnt_met(self):
        # LDS only here: vmcnt counts nothing, lgkmcnt = LDS loads + LDS stores in flight
        return self.loads() + self.lds_st <= self.wait[1]


class OCta:
    def __init__(self, warps):
        self.warps = warps      # warp slots
        self.live = len(warps)
        self.bar = 0
        self.nexit = 0


class OracleSM:
    """One SM.  fetch_rr, age_ctr, the schedulers' last-issued warps and the
    units' next-free cycles live as long as the SM (S1: they carry over from
    kernel to kernel); everything else is per CTA."""

    def __init__(self, cfg, sm_id):
        self.c, self.id = cfg, sm_id
        self.age_ctr = 0
        self.fetch_rr = 0
        self.sched_last = [0] * cfg.nsched          # S1: "last issued" starts as warp 0
        self.fu_next = {}
        self.st = Counter()
        self.distro = [0] * (3 + 64)
        self.single = [0] * cfg.nsched
        self.dual = [0] * cfg.nsched
        self.cover = Counter()
        self.issue_ev, self.sb_ev = [], []
        self.warps = {}                               # slot -> OWarp
        self.ctas = []
        self.idoc = {}                                # (sched, unit index) -> entry
        self.oc = [None] * cfg.noc
        self.ldst = None
        self.wb, self.hit = {}, {}

    # ---- CTA launch: lowest contiguous run of free warp slots, ages in launch order
    def launch(self, progs):
        n = len(progs)
        base = next(b for b in range(self.c.nw - n + 1) if not any(b + i in self.warps for i in range(n)))
        slots = list(range(base, base + n))
        cta = OCta(slots)
        for i, p in enumerate(progs):
            self.warps[base + i] = OWarp(p, self.age_ctr + i, cta)
        self.age_ctr += n
        self.ctas.append(cta)

    def active(self):
        return bool(self.ctas)

    def fit(self, wpc):
        """CTAs of wpc warps the SM can take on top of what it holds (epoch.h
        sm_cta_fit): threads, and first-fit runs of free warp slots; the cases
        keep registers, shared memory and the 32 CTA slots out of the way"""
        n, run = 0, 0
        for w in range(self.c.nw):
            run = 0 if w in self.warps else run + 1
            if run == wpc:
                n, run = n + 1, 0
        return min(n, (self.c.nw - len(self.warps)) // wpc)   # threads are warp-padded: counted in warps

    # ---- one core cycle, in sm_cycle's stage order
    def cycle(self, now):
        self.writeback(now)
        self.lds_complete(now)
        self.ldst_cycle(now)
        self.dispatch(now)
        self.read_operands()
        self.alloc_collectors()
        self.issue(now)
        self.fetch()
        self.retire()
        if self.ctas:
            self.st["active_cycles"] += 1

    def writeback(self, now):
        for w, dst in self.wb.pop(now, ()):
            W = self.warps[w]
            for r in dst:
                self.sb_ev.append((now, self.id, w, r - 1))
                W.sb.discard(r)
            W.inflight -= 1
            self.st["rf_writes"] += len(dst)

    def lds_complete(self, now):
        for w, slot in self.hit.pop(now, ()):
            W = self.warps[w]
            if slot is None:                      # a store
                W.lds_st -= 1
            else:
                for r in W.slots[slot]:
                    W.sb.discard(r)
                self.st["rf_writes"] += len(W.slots[slot])
                W.slots[slot] = None
            W.inflight -= 1

    def ldst_cycle(self, now):
        u = self.ldst
        if u is None:
            return
        inst, w, slot, start = u
        if now - start + 1 < inst.deg:           # busy for the conflict degree
            return
        due = self.hit.setdefault(now + self.c.smem_latency, [])
        if len(due) >= K_HIT_SLOT:
            self.cover["hit_retry"] += 1
            return
        due.append((w, slot if inst.kind == "ld" else None))
        self.st["shmem_acc"] += 1
        self.st["shmem_conf"] += inst.deg - 1
        self.ldst = None

    def dispatch(self, now):
        c = self.c
        ready = sorted((e for e in self.oc if e is not None and not e["reads"]), key=lambda e: e["age"])
        if ready and [e["idx"] for e in ready] != sorted(e["idx"] for e in ready):
            self.cover["dispatch_age_not_index"] += 1
        for e in ready:
            inst = e["inst"]
            if inst.unit == "MEM":
                if self.ldst is not None:
                    self.cover["ldst_busy"] += 1
                    continue
                self.ldst = (inst, e["warp"], e["slot"], now)
                self.st["mem_insn"] += 1
                self.oc[e["idx"]] = None
                continue
            phys = e["sched"] % max(c.units[inst.unit], 1)
            if self.fu_next.get((inst.unit, phys), 0) > now:
                self.cover["ii_wait"] += 1
                if c.units[inst.unit] < c.nsched:
                    self.cover["ii_wait_shared_unit"] += 1
                continue
            lat = min(max(inst.lat, 1), K_WB_RING - 1)
            bus = self.wb.setdefault(now + lat, [])
            if len(bus) >= c.wb_width:
                self.st["pipe_stall"] += 1
                continue
            bus.append((e["warp"], inst.dst))
            self.fu_next[(inst.unit, phys)] = now + inst.ii
            self.oc[e["idx"]] = None

    def read_operands(self):
        c = self.c
        for _ in range(c.port_tp):
            want = sorted((e for e in self.oc if e is not None and e["reads"]), key=lambda e: e["age"])
            if not want:
                break
            busy, grants = set(), 0
            for e in want:
                if grants >= c.noc:
                    break
                got = []
                for b in e["reads"]:
                    if grants >= c.noc:
                        break
                    if b not in busy:             # one read per bank per round
                        busy.add(b)
                        got.append(b)
                        grants += 1
                for b in got:
                    e["reads"].remove(b)
                self.st["rf_reads"] += len(got)
                self.st["bank_conflicts"] += len(e["reads"])   # reads left waiting this round

    def alloc_collectors(self):
        c = self.c
        for key in sorted(self.idoc):             # (scheduler, unit) order
            sched = key[0]
            free = [i for i in c.collectors_of(sched) if self.oc[i] is None]
            if not free:
                self.cover["collectors_full"] += 1
                continue
            e = self.idoc.pop(key)
            inst = e["inst"]
            self.oc[free[0]] = dict(idx=free[0], inst=inst, warp=e["warp"], sched=sched, slot=e["slot"], age=e["age"],
                                    reads=[c.reg_bank(sched, e["warp"], r - 1) for r in inst.src])

    # ---- issue -----------------------------------------------------------
    def sb_ok(self, W, I):
        return not any(r in W.sb for r in I.src + I.dst)

    def can_issue_nosb(self, w, I, busy):
        W = self.warps[w]
        if W.parked() or W.ibuf == 0:
            return False
        if I.special:
            return True
        if (self.c.sched_of(w), UNITS.index(I.unit)) in busy:
            return False
        if I.kind == "ld" and all(s is not None for s in W.slots):
            self.cover["load_slots_full"] += 1
            return False
        return True

    def due(self, W, now):
        return self.c.interval <= 1 or now >= W.issue_ok

    def barrier_check(self, cta):
        if cta.bar > 0 and cta.bar >= cta.live - cta.nexit:
            if cta.nexit:
                self.cover["barrier_released_with_exits"] += 1
            for w in cta.warps:
                if w in self.warps:
                    self.warps[w].barrier = False
            cta.bar = 0

    def issue_one(self, now, sc, w, I):
        c, W = self.c, self.warps[w]
        self.issue_ev.append((now, self.id, w, I.pc))
        W.head += 1
        W.ibuf -= 1
        self.st["warp_insn"] += 1
        self.st["thread_insn"] += I.lanes
        self.st["cls_" + I.cls] += 1
        if I.kind == "exit":
            if W.head >= len(W.prog):             # the warp ends only when EXIT is its last instruction
                W.exiting = True
                W.cta.nexit += 1
                self.barrier_check(W.cta)
            else:
                self.cover["exit_not_last"] += 1
            return None
        if I.kind == "bar":
            W.barrier = True
            W.cta.bar += 1
            self.barrier_check(W.cta)
            return None
        if I.kind == "membar":                    # no stores outstanding: nothing to wait for
            return None
        if I.kind == "waitcnt":
            W.wait = I.wait
            if not W.waitcnt_met():
                W.waitcnt = True
                self.cover["waitcnt_parked"] += 1
            else:
                self.cover["waitcnt_passed"] += 1
            return None
        if I.kind == "nop":
            return None
        W.inflight += 1
        slot = None
        if I.kind == "ld":
            slot = W.slots.index(None)
            W.slots[slot] = I.dst
            if W.loads() == K_LOAD_SLOTS:
                self.cover["eight_loads_in_flight"] += 1
        elif I.kind == "st":
            W.lds_st += 1
        self.age_ctr += 1
        self.idoc[(sc, UNITS.index(I.unit))] = dict(inst=I, warp=w, slot=slot, age=self.age_ctr)
        W.sb.update(I.dst)
        return I.unit

    def waits_long_op(self, W, I):
        return any(r in I.src for s in W.slots if s is not None for r in s)

    def pick(self, now, cand, last):
        c = self.c
        oldest = lambda: min(cand, key=lambda w: (self.warps[w].age, w))
        cyclic = lambda start: min(cand, key=lambda w: (w - start) % c.nw)
        if c.policy in ("gto", "swl"):
            return last if last in cand else oldest()
        if c.policy == "old":
            return oldest()
        if c.policy == "rrr":
            return cyclic(now % c.nw)
        return cyclic((last + 1) % c.nw)          # lrr and the two-level inner level

    def issue(self, now):
        c = self.c
        live = sorted(self.warps)
        head = {w: self.warps[w].prog[self.warps[w].head] for w in live if self.warps[w].ibuf}
        valid0 = {w for w in head if not self.warps[w].parked() and self.due(self.warps[w], now)}
        busy0 = set(self.idoc)
        ready = {w for w in head if self.can_issue_nosb(w, head[w], busy0) and self.sb_ok(self.warps[w], head[w])
                 and self.due(self.warps[w], now)}
        if c.interval > 1 and not ready and any(
                self.can_issue_nosb(w, head[w], busy0) and self.sb_ok(self.warps[w], head[w]) for w in head):
            self.cover["held_by_interval_only"] += 1
        waiting = set()
        if c.policy in ("2lv", "swl"):
            for w in live:
                W = self.warps[w]
                if W.parked():
                    waiting.add(w)
                elif c.policy == "2lv" and w in head and self.waits_long_op(W, head[w]):
                    waiting.add(w)
                    self.cover["two_level_demoted"] += 1
        masks = None
        issued_any = False
        for sc in range(c.nsched):
            mine = [w for w in live if c.sched_of(w) == sc and w in self.warps]
            cand = {w for w in mine if w in ready}
            last = self.sched_last[sc]
            if cand and c.policy == "swl":
                pool = sorted((w for w in mine if w not in waiting), key=lambda w: (self.warps[w].age, w))
                lim = set(pool[:c.sched_param]) | {last}
                if cand - lim:
                    self.cover["swl_limited"] += 1
                cand &= lim
            elif cand and c.policy == "2lv":
                act = set([w for w in mine if w not in waiting][:c.sched_param])
                if cand - act:
                    self.cover["two_level_limited"] += 1
                cand &= act
            if not cand:
                if mine:
                    self.st["stall_idle"] += 1
                    if masks is None:             # classified once, at the first idle scheduler
                        if issued_any:
                            self.cover["classified_after_issue"] += 1
                        valid = {w for w in self.warps if not self.warps[w].parked() and self.warps[w].ibuf
                                 and self.due(self.warps[w], now)}
                        sbok = {w for w in valid
                                if self.sb_ok(self.warps[w], self.warps[w].prog[self.warps[w].head])}
                        masks = (valid, sbok)
                        idle = {w for s2 in range(sc, c.nsched) for w in live if c.sched_of(w) == s2}
                        if (valid & idle) != (valid0 & idle):
                            self.cover["class_changed_by_earlier_issue"] += 1
                    k = 0 if not masks[0] & set(mine) else 1 if not masks[1] & set(mine) else 2
                    self.distro[k] += 1
                continue
            w = self.pick(now, cand, last)
            if w != min(cand):
                self.cover["pick_not_lowest"] += 1
            if w != min(cand, key=lambda x: (self.warps[x].age, x)):
                self.cover["pick_not_oldest"] += 1
            if min(cand) != min(cand, key=lambda x: (self.warps[x].age, x)):
                self.cover["age_not_warp_order"] += 1
            if c.policy in ("gto", "swl") and w == last and w != min(cand, key=lambda x: (self.warps[x].age, x)):
                self.cover["greedy_over_oldest"] += 1
            self.sched_last[sc] = w
            W = self.warps[w]
            if c.interval > 1:
                W.issue_ok = now + c.interval
            I1 = head[w]
            u1 = self.issue_one(now, sc, w, I1)
            issued_any = True
            self.distro[2 + I1.lanes] += 1
            dual = False
            if c.max_issue > 1 and u1 is not None and W.ibuf:
                I2 = W.prog[W.head]
                if I2.special:
                    self.cover["dual_second_special"] += 1
                elif c.dual_diff and I2.unit == u1:
                    self.cover["dual_same_unit"] += 1
                elif not self.sb_ok(W, I2):
                    self.cover["dual_second_scoreboard"] += 1
                elif not self.can_issue_nosb(w, I2, set(self.idoc)):
                    self.cover["dual_second_idoc_busy"] += 1
                else:
                    self.issue_one(now, sc, w, I2)
                    self.st["dual_issued"] += 1
                    self.distro[2 + I2.lanes] += 1
                    dual = True
            if dual:
                self.dual[sc] += 1
            else:
                self.single[sc] += 1
        if issued_any:
            self.st["busy_cycles"] += 1

    def fetch(self):
        c = self.c
        need = [w for w, W in self.warps.items() if not W.exiting and W.ibuf == 0 and W.next < len(W.prog)]
        start = self.fetch_rr % c.nw
        for w in sorted(need, key=lambda w: (w - start) % c.nw)[:c.fetch_tp]:
            W = self.warps[w]
            n = min(len(W.prog) - W.next, K_IBUF)
            W.next += n
            W.ibuf = n
            self.fetch_rr = w + 1

    def retire(self):
        done = [w for w, W in sorted(self.warps.items())
                if W.head >= len(W.prog) and W.ibuf == 0 and W.inflight == 0 and W.loads() == 0]
        for W in self.warps.values():
            if W.waitcnt and W.waitcnt_met():
                W.waitcnt = False
        for w in done:
            W = self.warps.pop(w)
            cta = W.cta
            if not W.exiting:
                self.cover["implicit_exit"] += 1
            # an exited warp stops counting as exited once it is no longer live
            cta.nexit += 0 if W.exiting else 1
            self.st["warps_done"] += 1
            cta.live -= 1
            cta.nexit -= 1
            if cta.live == 0:
                self.ctas.remove(cta)
                self.st["ctas_done"] += 1
            else:
                self.barrier_check(cta)


# ---------------------------------------------------------------------------
# test programs: one description drives both the trace and the oracle
# ---------------------------------------------------------------------------
SHMEM_BASE = 0x00007F0000000000  # KernelBuilder's header value


class Op:
    def __init__(self, mn, dst=(), src=(), mask=None, present=None, stride=4, wait=None):
        self.mn, self.dst, self.src, self.mask, self.present, self.stride, self.wait = \
            mn, tuple(dst), tuple(src), mask, present, stride, wait


class Kernel:
    """grid x block (threads) and one program; `present` / `mask` of an Op are
    None, a scalar, or a function of the kernel-wide warp index"""

    def __init__(self, ncta, threads, ops, warp_size=32):
        self.ncta, self.threads, self.ops, self.ws = ncta, threads, ops, warp_size
        self.wpc = -(-threads // warp_size)

    def nwarps(self):
        return self.ncta * self.wpc

    def full_mask(self, gw):
        live = min(self.ws, self.threads - (gw % self.wpc) * self.ws)
        return (1 << live) - 1

    def mask_of(self, op, gw):
        m = op.mask(gw) if callable(op.mask) else op.mask
        return self.full_mask(gw) if m is None else m & self.full_mask(gw)

    def present_of(self, op, gw):
        p = op.present(gw) if callable(op.present) else op.present
        return True if p is None else bool(p)

    def build(self, kid):
        cdna = self.ws == 64
        k = KernelBuilder(f"_Z4core{kid}Pi", (self.ncta, 1, 1), (self.threads, 1, 1), nregs=16, kid=kid,
                          warp_size=self.ws, binary_version=950 if cdna else 70)
        n = self.nwarps()
        waits = {}
        for op in self.ops:
            mask = np.array([self.mask_of(op, g) for g in range(n)], np.uint64)
            present = np.array([self.present_of(op, g) for g in range(n)], bool)
            if op.wait is not None:
                waits[k.pc] = op.wait[0] | op.wait[1] << 8
            if MNEMONICS[op.mn][1] in ("ld", "st"):
                k.op(op.mn, op.dst, op.src, base=np.full(n, SHMEM_BASE, np.int64), stride=op.stride, mask=mask,
                     present=present)
            else:
                k.op(op.mn, op.dst, op.src, mask=mask, present=present)
        ka = k.build()
        # the s_waitcnt counts travel in TInst::lat (vm | lgkm << 8)
        for pc, packed in waits.items():
            sel = (ka.insts["pc"] == pc) & ((ka.insts["flags"] & 8) != 0)
            assert sel.any()
            ka.insts["lat"][sel] = packed
        return ka

    def lds_degree(self, cfg, op, lanes):
        """conflict degree of an LDS access of 4-byte words at base + k * stride
        for the k-th active lane: the most distinct words in one bank"""
        words = {}
        for k in range(lanes):
            word = (SHMEM_BASE + k * op.stride) >> 2
            words.setdefault(word % cfg.smem_banks, set()).add(word)
        return max(len(v) for v in words.values())

    def programs(self, cfg):
        """per kernel-wide warp index: the warp's instruction stream (an
        instruction with no active lane is not in the trace, barriers and EXIT
        aside)"""
        out = []
        for g in range(self.nwarps()):
            prog = []
            for i, op in enumerate(self.ops):
                m = self.mask_of(op, g)
                kind = MNEMONICS[op.mn][1]
                if not self.present_of(op, g) or (m == 0 and kind not in ("bar", "exit")):
                    continue
                deg = self.lds_degree(cfg, op, popc(m)) if kind in ("ld", "st") else 1
                prog.append(OInst(cfg, 16 * i, op.mn, op.dst, op.src, popc(m), deg, op.wait))
            out.append(prog)
        return out


def anchor(cfg, prev_end):
    """The launch cycle L of a kernel admitted at cycle prev_end (0 for the
    first).  epoch.h: sm_epoch dispatches CTAs from the requests the SMs
    published at the previous epoch boundary (sm_publish's reqk).  A kernel
    admitted at a boundary is first seen by the publication at the end of the
    following epoch, so its CTAs launch one epoch later: at -icnt_latency for
    the first kernel, at prev_end + -icnt_latency for the next."""
    return prev_end + cfg.epoch


def oracle_run(opts, kernels):
    """simulate `kernels` back to back; returns the SMs and per kernel
    (L, gpu_sim_cycle, thread instructions)"""
    cfg = CoreCfg(opts)
    sms = [OracleSM(cfg, i) for i in range(cfg.n_sm)]
    per_kernel, end = [], 0
    for kern in kernels:
        L = anchor(cfg, end)
        progs = kern.programs(cfg)
        pending = [progs[cta * kern.wpc:(cta + 1) * kern.wpc] for cta in range(kern.ncta)]
        insn0 = sum(s.st["thread_insn"] for s in sms)
        now = L
        while pending or any(s.active() for s in sms):
            if pending and now % cfg.epoch == 0:
                # epoch.h cta_dispatch, at an epoch's start: every SM asks for the
                # CTAs it had room for at the boundary; rounds over the asking SMs
                # in SM order rotated by the epoch index hand out the next CTAs
                room = [s.fit(kern.wpc) for s in sms]
                rot = (now // cfg.epoch) % cfg.n_sm
                order = sorted(range(cfg.n_sm), key=lambda j: (j - rot) % cfg.n_sm)
                for rnd in range(max(room)):
                    for j in order:
                        if room[j] > rnd and pending:
                            sms[j].launch(pending.pop(0))
            for s in sms:
                if s.active():
                    s.cycle(now)
            now += 1
            assert now - L < 100000, "oracle: the program does not end"
        # the kernel is seen complete at the end of the epoch of its last cycle
        new_end = (now - 1) // cfg.epoch * cfg.epoch + cfg.epoch
        per_kernel.append((L, new_end - end, sum(s.st["thread_insn"] for s in sms) - insn0))
        end = new_end
    return cfg, sms, per_kernel


# ---------------------------------------------------------------------------
# running the engines and reading their output
# ---------------------------------------------------------------------------
def base_options(**over):
    o = presets.get_preset("QV100")
    o.update({
        "-gpgpu_n_clusters": "1", "-gpgpu_n_cores_per_cluster": "1", "-gpgpu_shader_core_pipeline": "512:32",
        "-icnt_latency": "8", "-gpgpu_kernel_launch_latency": "0", "-gpgpu_TB_launch_latency": "0",
        "-gpgpu_perfect_inst_const_cache": "1", "-gpgpu_perf_sim_memcpy": "0",
        "-gpgpu_num_sched_per_core": "4", "-gpgpu_scheduler": "lrr", "-gpgpu_sub_core_model": "1",
        "-gpgpu_enable_specialized_operand_collector": "0", "-gpgpu_operand_collector_num_units_gen": "8",
        "-gpgpu_num_reg_banks": "16", "-gpgpu_reg_file_port_throughput": "2",
        "-gpgpu_num_sp_units": "4", "-gpgpu_num_dp_units": "4", "-gpgpu_num_int_units": "4",
        "-gpgpu_num_sfu_units": "4", "-gpgpu_tensor_core_avail": "1", "-gpgpu_num_tensor_core_units": "4",
        "-gpgpu_pipeline_widths": "4,4,4,4,4,4,4,4,4,4,8,4,4",
        "-trace_opcode_latency_initiation_int": "2,2", "-trace_opcode_latency_initiation_sp": "2,2",
        "-trace_opcode_latency_initiation_dp": "8,4", "-trace_opcode_latency_initiation_sfu": "20,8",
        "-trace_opcode_latency_initiation_tensor": "6,2",
        "-gpgpu_smem_latency": "20", "-gpgpu_warp_issue_interval": "1", "-gpgpu_max_insn_issue_per_warp": "1",
        "-gpgpu_dual_issue_diff_exec_units": "1", "-gpgpu_inst_fetch_throughput": "4", "-sim_single_valu": "0",
        "-gpgpu_shmem_num_banks": "32", "-gpgpu_shmem_warp_parts": "1", "-gpgpu_shmem_limited_broadcast": "0",
        "-gpgpu_shmem_cdna_lane_groups": "0", "-sim_lds_port_bytes": "0",
    })
    o.pop("-smem_latency", None)
    o.update({k: str(v) for k, v in over.items()})
    return o


def run_sim(mod, opts, kl, engine, streams, extra=None):
    from accel_sim_framework_distributed_amd.sim import build_args
    tr = {"-trace_enabled": "0"}
    if streams:
        tr = {"-trace_enabled": "1", "-trace_sampling_core": "-1", "-trace_components": streams}
    s = mod.Simulator(build_args(opts, kl, engine, dict(tr, **(extra or {}))), False)
    t0 = time.perf_counter()
    assert s.run() == 0, s.output[-2000:]
    wall = time.perf_counter() - t0
    assert s.engine == engine
    assert "trace events dropped" not in s.output
    return s.output, wall


def stat(out, key):
    m = re.findall(rf"^{re.escape(key)} = ([0-9]+)", out, re.M)
    assert m, key
    return int(m[-1])


def issue_events(out):
    return [(int(c), int(s), int(w), int(pc, 16)) for c, s, w, pc in re.findall(
        r"Cycle (\d+): WARP_SCHEDULER - core (\d+) issued warp (\d+) pc 0x([0-9a-f]+)", out)]


def sb_events(out):
    return [(int(c), int(s), int(w), int(r)) for c, s, w, r in re.findall(
        r"Cycle (\d+): SCOREBOARD - core (\d+) warp (\d+) releases register (\d+)", out)]


def merged(sms, attr):
    """the host prints events in (cycle, unit, order) order"""
    ev = [e for s in sms for e in getattr(s, attr)]
    return sorted(ev, key=lambda e: (e[0], e[1]))  # stable: keeps the order within (cycle, SM)


def first_diff(got, want):
    bad = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), None)
    assert bad is None, (bad, "engine", got[bad], "oracle", want[bad], "before", want[max(0, bad - 3):bad])
    assert len(got) == len(want), (len(got), len(want))


def check_anchor(cfg, ev_by_kernel, per_kernel):
    """L = the observed cycle of each SM's first event minus the oracle's
    relative cycle for it: the same on every SM, and the predicted one"""
    for (got, want), (L, _, _) in zip(ev_by_kernel, per_kernel):
        seen = {}
        for g, w in zip(got, want):
            if w[1] not in seen:
                seen[w[1]] = g[0] - (w[0] - L)
        assert len(set(seen.values())) == 1 and set(seen.values()) == {L}, (seen, L)


def split_by_kernel(ev, per_kernel):
    """events of kernel k lie in [L_k, L_k + cycles_k)"""
    out, lo = [], 0
    for L, cyc, _ in per_kernel:
        hi = lo + cyc
        out.append([e for e in ev if lo <= e[0] < hi])
        lo = hi
    return out


def check_stats(out, cfg, sms, per_kernel):
    tot = Counter()
    for s in sms:
        tot.update(s.st)
    assert [int(x) for x in re.findall(r"^gpu_sim_cycle = (\d+)", out, re.M)] == [k[1] for k in per_kernel]
    assert [int(x) for x in re.findall(r"^gpu_sim_insn = (\d+)", out, re.M)] == [k[2] for k in per_kernel]
    assert stat(out, "gpu_tot_sim_insn") == tot["thread_insn"]
    assert stat(out, "gpgpu_n_tot_w_icount") == tot["warp_insn"]
    line = re.findall(r"Warp Occupancy Distribution:\n(.*)\n", out)[-1]
    got = {k: int(v) for k, v in (f.split(":") for f in line.split("\t") if f)}
    distro = [sum(s.distro[i] for s in sms) for i in range(3 + 64)]
    want = {"Stall": distro[2], "W0_Idle": distro[0], "W0_Scoreboard": distro[1]}
    want.update({f"W{i}": distro[2 + i] for i in range(1, cfg.warp_size + 1)})
    assert got == want
    for name, attr in (("single_issue_nums", "single"), ("dual_issue_nums", "dual")):
        line = re.findall(rf"^{name}: (.*)$", out, re.M)[-1]
        got = [int(f.split(":")[1]) for f in line.split("\t") if f.strip()]
        assert got == [sum(getattr(s, attr)[i] for s in sms) for i in range(cfg.nsched)], name
    for key, name in (("gpgpu_n_dual_issue", "dual_issued"), ("gpu_stall_shd_idle_sched", "stall_idle"),
                      ("gpu_stall_result_bus", "pipe_stall"), ("gpu_reg_bank_conflict_stalls", "bank_conflicts"),
                      ("gpgpu_n_regfile_reads", "rf_reads"), ("gpgpu_n_regfile_writes", "rf_writes"),
                      ("gpgpu_n_shmem_bank_access", "shmem_acc"), ("gpgpu_n_shmem_bkconflict", "shmem_conf"),
                      ("gpgpu_n_completed_cta", "ctas_done"), ("gpgpu_n_completed_warps", "warps_done"),
                      ("gpgpu_sm_active_cycles", "active_cycles"), ("gpgpu_sm_issue_busy_cycles", "busy_cycles"),
                      ("gpgpu_n_mem_insn_dispatched", "mem_insn"), ("gpgpu_n_load_insn", "cls_LOAD"),
                      ("gpgpu_n_store_insn", "cls_STORE"), ("gpgpu_n_sfu_insn", "cls_SFU"),
                      ("gpgpu_n_dp_insn", "cls_DP"), ("gpgpu_n_tensor_insn", "cls_TENSOR"),
                      ("gpgpu_n_barrier_insn", "cls_BARRIER")):
        assert stat(out, key) == tot[name], (key, stat(out, key), tot[name])


STAT_LINES = re.compile(r"^(gpu_sim_cycle|gpu_sim_insn|gpgpu_n_\w+|gpu_stall_\w+|gpu_reg_bank\w+|gpgpu_sm_\w+|"
                        r"single_issue_nums|dual_issue_nums|Stall:).*$", re.M)


def stat_block(out):
    return [m.group(0) for m in STAT_LINES.finditer(out)]


PAR_POLICIES = ("lrr", "gto", "old", "rrr")


def check_case(mod, engine, name, tmp_path):
    opts, kernels, expect = CASES[name]()
    cfg, sms, per_kernel = oracle_run(opts, kernels)
    cover = Counter()
    for s in sms:
        cover.update(s.cover)
    tot = Counter()
    for s in sms:
        tot.update(s.st)
    expect(cover, tot, sms, per_kernel)              # the case reaches its edge, on the oracle alone
    kl = rodinia.write_app(str(tmp_path / name), [k.build(i + 1) for i, k in enumerate(kernels)], memcpy=False)
    walls = []
    # a. the sequential issue loop: every issue
    out, wall = run_sim(mod, opts, kl, engine, "WARP_SCHEDULER")
    walls.append(wall)
    want = merged(sms, "issue_ev")
    got = issue_events(out)
    first_diff(got, want)
    check_anchor(cfg, zip(split_by_kernel(got, per_kernel), split_by_kernel(want, per_kernel)), per_kernel)
    assert per_kernel[0][0] == int(opts["-icnt_latency"]) == 8   # the first kernel's L, see anchor()
    check_stats(out, cfg, sms, per_kernel)
    ref = stat_block(out)
    # b. the scoreboard stream alone leaves the lane-parallel issue path on
    out, wall = run_sim(mod, opts, kl, engine, "SCOREBOARD")
    walls.append(wall)
    want = merged(sms, "sb_ev")
    got = sb_events(out)
    first_diff(got, want)
    if want:
        check_anchor(cfg, zip(split_by_kernel(got, per_kernel), split_by_kernel(want, per_kernel)), per_kernel)
    check_stats(out, cfg, sms, per_kernel)
    assert stat_block(out) == ref
    # c. / d. no stream, with and without the quiet-cycle fast-forward
    for skip in ("1", "0"):
        out, wall = run_sim(mod, opts, kl, engine, None, {"-sim_event_skip": skip})
        walls.append(wall)
        check_stats(out, cfg, sms, per_kernel)
        assert stat_block(out) == ref
    par = cfg.policy in PAR_POLICIES and cfg.max_issue == 1
    print(f"{name} [{engine}]: {sum(walls):.2f} s in {len(walls)} runs, {tot['warp_insn']} warp instructions, "
          f"{sum(k[1] for k in per_kernel)} cycles, lane-parallel issue {'on' if par else 'off'} in b-d")
    return sum(walls)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
REGS = (4, 5, 6, 7, 8, 9)     # a small window: dependences are frequent
SASS_ALU = ("MOV", "IMAD", "FFMA", "DFMA", "MUFU.RCP")


def random_ops(seed, n, alu=SASS_ALU, lds=0.15, bar=0.06, nop=0.04, strides=(4, 4, 8), nwarps=1, vary=0.25,
               masks=(None,), ld="LDS", st="STS", barrier="BAR.SYNC", nopm="NOP", exitm="EXIT"):
    """a seeded program: ALU work over a small register window, LDS loads and
    stores, barriers, NOPs; some instructions are present in some warps only
    and run under partial masks"""
    rnd = random.Random(seed)
    ops = []
    for _ in range(n):
        x = rnd.random()
        present = None
        if rnd.random() < vary:
            absent = frozenset(g for g in range(nwarps) if rnd.random() < 0.4)
            present = (lambda a: lambda g: g not in a)(absent)
        mask = rnd.choice(masks)
        if x < lds:
            if rnd.random() < 0.6:
                ops.append(Op(ld, [rnd.choice(REGS)], [rnd.choice(REGS)], mask, present, rnd.choice(strides)))
            else:
                ops.append(Op(st, [], [rnd.choice(REGS), rnd.choice(REGS)], mask, present, rnd.choice(strides)))
        elif x < lds + bar:
            ops.append(Op(barrier))
        elif x < lds + bar + nop:
            ops.append(Op(nopm, present=present))
        else:
            ops.append(Op(rnd.choice(alu), [rnd.choice(REGS)], [rnd.choice(REGS) for _ in range(rnd.randint(1, 3))],
                          mask, present))
    ops.append(Op(exitm))
    return ops


def need(**at_least):
    """coverage assertion on the oracle's own counters"""
    def expect(cover, tot, sms, per_kernel):
        for k, v in at_least.items():
            have = cover[k] if k in cover or k not in tot else tot[k]
            assert have >= v, f"vacuous: the oracle run has {k} = {have}, wanted >= {v}"
    return expect


def both(*fs):
    def expect(*a):
        for f in fs:
            f(*a)
    return expect


CASES = {}


def case(fn):
    CASES[fn.__name__[2:]] = fn
    return fn


# ---- the six policies with 1..4 schedulers; two kernels back to back, so
# ---- both the very first pick (S1) and the carried-over state are covered
SCHED_STRINGS = {"lrr": "lrr", "gto": "gto", "old": "old", "rrr": "rrr", "2lv": "two_level_active:2:0:1",
                 "swl": "warp_limiting:2:2"}


def sched_case(policy, nsched):
    def make():
        # 9 and 10 warps: no multiple of 3 or 4, the first not of 2 either
        k1 = Kernel(3, 96, random_ops(100 + nsched, 28, nwarps=9, lds=0.2))
        k2 = Kernel(2, 160, random_ops(200 + nsched, 22, nwarps=10, lds=0.2))
        opts = base_options(**{"-gpgpu_num_sched_per_core": nsched, "-gpgpu_scheduler": SCHED_STRINGS[policy],
                               "-gpgpu_smem_latency": 30})
        want = dict(pick_not_lowest=1) if policy != "old" else {}
        if policy in ("gto", "swl"):
            want["greedy_over_oldest"] = 1
        if policy == "2lv":
            want.update(two_level_demoted=1, two_level_limited=1)
        if policy == "swl":
            want["swl_limited"] = 1

        def two_anchors(cover, tot, sms, per_kernel):
            # rrr picks from now % warp slots: the two kernels start at different phases
            assert policy != "rrr" or len({k[0] % 16 for k in per_kernel}) >= 2
        return opts, [k1, k2, k1], both(need(**want), two_anchors)
    make.__name__ = f"c_sched_{policy}_{nsched}"
    return make


for _p in SCHED_STRINGS:
    for _n in (1, 2, 3, 4):
        case(sched_case(_p, _n))


def limit_case(policy, param):
    def make():
        s = "two_level_active:%d:0:1" % param if policy == "2lv" else "warp_limiting:2:%d" % param
        k = Kernel(2, 128, random_ops(300 + param, 26, nwarps=8, lds=0.25))
        opts = base_options(**{"-gpgpu_num_sched_per_core": 2, "-gpgpu_scheduler": s, "-gpgpu_smem_latency": 30})
        lim = "two_level_limited" if policy == "2lv" else "swl_limited"

        def never(cover, tot, sms, per_kernel):
            assert not cover[lim], "a limit above the scheduler's 4 warps never limits"
        return opts, [k], need(**{lim: 1}) if param < 4 else never
    make.__name__ = f"c_limit_{policy}_{param}"
    return make


for _p in ("2lv", "swl"):
    for _n in (1, 2, 9):
        case(limit_case(_p, _n))


# ---- a grid of two waves: a later CTA sits in lower warp slots than an
# ---- earlier one, so warp age and warp order differ (gto, oldest, warp-limiting)
def wave_case(policy):
    def make():
        ops = random_ops(700, 14, nwarps=24, lds=0.1, bar=0.08, vary=0)
        # the CTAs differ in length, so they end apart and their slots refill apart
        ops = ops[:-1] + [Op("MUFU.RCP", [4 + i % 5], [5], present=(lambda i: lambda g: (g // 4) % 3 >= 1 + i % 2)(i))
                          for i in range(6)] + ops[-1:]
        k = Kernel(6, 128, ops)
        sched = "warp_limiting:2:4" if policy == "swl" else SCHED_STRINGS[policy]
        opts = base_options(**{"-gpgpu_num_sched_per_core": 2, "-gpgpu_scheduler": sched})

        def young_below_old(cover, tot, sms, per_kernel):
            # a scheduler chose among warps whose oldest is not the lowest slot
            assert cover["age_not_warp_order"] >= 2, cover["age_not_warp_order"]
        return opts, [k], young_below_old
    make.__name__ = f"c_waves_{policy}"
    return make


for _p in ("gto", "old", "swl"):
    case(wave_case(_p))


# ---- sub-core model, collectors, register banks, ports ---------------------
def collector_case(sub, noc, banks, tp, nsched=4):
    def make():
        k = Kernel(2, 256, random_ops(400 + noc + banks, 30, nwarps=16, lds=0.1))
        opts = base_options(**{"-gpgpu_sub_core_model": sub, "-gpgpu_operand_collector_num_units_gen": noc,
                               "-gpgpu_num_reg_banks": banks, "-gpgpu_reg_file_port_throughput": tp,
                               "-gpgpu_num_sched_per_core": nsched, "-gpgpu_scheduler": "gto"})
        return opts, [k], need(bank_conflicts=1, collectors_full=1, dispatch_age_not_index=1)
    make.__name__ = f"c_collectors_sub{sub}_oc{noc}_banks{banks}_tp{tp}_s{nsched}"
    return make


case(collector_case(1, 2, 16, 1))      # fewer collectors than schedulers
case(collector_case(1, 4, 12, 2))      # equal; 3 banks per scheduler: no power of two
case(collector_case(1, 6, 8, 1))       # no multiple of the schedulers
case(collector_case(0, 3, 6, 1))       # one shared pool, 6 banks
case(collector_case(0, 8, 16, 2, 3))   # three schedulers
case(collector_case(1, 6, 9, 1, 3))    # three schedulers, 3 banks each


# ---- unit mapping, latencies, initiation intervals, the result bus ---------
@case
def c_units_shared():
    """two schedulers share one SP / INT / SFU unit and its initiation interval"""
    k = Kernel(1, 256, random_ops(500, 30, alu=("FFMA", "IMAD", "MUFU.RCP"), nwarps=8, lds=0, bar=0))
    opts = base_options(**{"-gpgpu_num_sched_per_core": 4, "-gpgpu_num_sp_units": 2, "-gpgpu_num_int_units": 1,
                           "-gpgpu_num_sfu_units": 3, "-trace_opcode_latency_initiation_sp": "4,2",
                           "-trace_opcode_latency_initiation_int": "4,8"})
    return opts, [k], need(ii_wait_shared_unit=5)


@case
def c_units_absent():
    """no DP unit: DP work on the SFU unit; no INT and tensor unit: on SP"""
    alu = ("v_fma_f64", "v_rcp_f32", "s_add_u32", "v_fma_f32", "v_mfma_f32_32x32x16_bf16")
    ops = random_ops(510, 30, alu=alu, nwarps=4, lds=0, bar=0, nopm="s_nop", exitm="s_endpgm")
    k = Kernel(1, 256, ops, warp_size=64)
    opts = base_options(**{"-gpgpu_num_dp_units": 0, "-gpgpu_num_int_units": 0, "-gpgpu_tensor_core_avail": 0,
                           "-gpgpu_num_sched_per_core": 2, "-gpgpu_shader_core_pipeline": "1024:64"})
    return opts, [k], need(ii_wait=5, cls_DP=3, cls_SFU=3, cls_TENSOR=3, cls_INTP=3)


@case
def c_latencies():
    """latencies 1, 4 and 511; initiation intervals 1, 2 and 8"""
    k = Kernel(1, 128, random_ops(520, 24, alu=("FFMA", "IMAD", "MUFU.RCP", "DFMA"), nwarps=4, lds=0, bar=0.05))
    opts = base_options(**{"-trace_opcode_latency_initiation_sp": "1,1", "-trace_opcode_latency_initiation_int": "4,2",
                           "-trace_opcode_latency_initiation_dp": "511,8", "-trace_opcode_latency_initiation_sfu": "9,8",
                           "-gpgpu_num_sched_per_core": 2})
    return opts, [k], need(ii_wait=3, cls_DP=3)


def bus_case(width):
    def make():
        """different latencies converge on one writeback cycle"""
        k = Kernel(1, 256, random_ops(530, 30, alu=("FFMA", "IMAD", "DFMA"), nwarps=8, lds=0, bar=0))
        w = "4,4,4,4,4,4,4,4,4,4,%d,4,4" % width
        opts = base_options(**{"-gpgpu_pipeline_widths": w, "-trace_opcode_latency_initiation_sp": "3,1",
                               "-trace_opcode_latency_initiation_int": "2,1",
                               "-trace_opcode_latency_initiation_dp": "4,1"})
        return opts, [k], need(pipe_stall=3)
    make.__name__ = f"c_result_bus_{width}"
    return make


case(bus_case(1))
case(bus_case(2))


# ---- issue interval, dual issue --------------------------------------------
def interval_case(iv):
    def make():
        k = Kernel(1, 128, random_ops(540, 24, nwarps=4, lds=0.1))
        opts = base_options(**{"-gpgpu_warp_issue_interval": iv, "-trace_opcode_latency_initiation_sp": "1,1",
                               "-trace_opcode_latency_initiation_int": "1,1"})
        return opts, [k], need(held_by_interval_only=3) if iv > 1 else need()
    make.__name__ = f"c_issue_interval_{iv}"
    return make


case(interval_case(1))
case(interval_case(4))


def dual_case(diff):
    def make():
        k = Kernel(1, 192, random_ops(550 + diff, 36, nwarps=6, lds=0.1, bar=0.08))
        opts = base_options(**{"-gpgpu_max_insn_issue_per_warp": 2, "-gpgpu_dual_issue_diff_exec_units": diff,
                               "-gpgpu_num_sched_per_core": 2, "-gpgpu_scheduler": "gto",
                               "-gpgpu_operand_collector_num_units_gen": 2,
                               "-trace_opcode_latency_initiation_sp": "1,1"})
        want = dict(dual_issued=3, dual_second_special=1, dual_second_scoreboard=1, dual_second_idoc_busy=1)
        if diff:
            want["dual_same_unit"] = 1
        return opts, [k], need(**want)
    make.__name__ = f"c_dual_issue_diff{diff}"
    return make


case(dual_case(0))
case(dual_case(1))


# ---- barriers, exits, partial masks ----------------------------------------
@case
def c_barriers_and_exits():
    """two CTAs at different barriers; warps that exit before a barrier the
    others wait at; an EXIT in mid-stream; a warp whose stream has no EXIT"""
    early = lambda g: g % 4 == 1          # leaves before the second barrier
    late = lambda g: g % 4 != 1
    cta1 = lambda g: g >= 4
    ops = [Op("FFMA", [4], [5, 6]), Op("IMAD", [5], [4]),
           Op("MUFU.RCP", [6], [4], present=cta1),              # the second CTA reaches its barrier later
           Op("BAR.SYNC"),
           Op("MEMBAR.GL"),                                     # no store outstanding: passes at once
           Op("NOP"),
           Op("FFMA", [7], [6, 5]),
           Op("MUFU.RCP", [9], [4], present=early),             # still in flight when the others arrive
           Op("EXIT", present=early),
           Op("EXIT", present=lambda g: g % 4 == 2),            # not the last instruction of warp 2
           Op("DFMA", [8], [7], present=late),
           Op("BAR.SYNC", present=late),
           Op("FFMA", [4], [8], present=late),
           Op("EXIT", present=lambda g: g % 4 in (0, 2)),       # warp 3 ends without EXIT
           ]
    k = Kernel(2, 128, ops)
    opts = base_options(**{"-gpgpu_num_sched_per_core": 2})
    return opts, [k], need(barrier_released_with_exits=1, exit_not_last=2, implicit_exit=2, cls_BARRIER=14,
                           cls_MEMBAR=8, cls_NOP=8)


@case
def c_barrier_classify_point():
    """scheduler 0 issues the barrier that releases the CTA in a cycle in which
    a later scheduler has nothing to issue: the idle scheduler is classified
    after that issue"""
    ops = [Op("MUFU.RCP", [4], [5], present=lambda g: g == 0),  # warp 0 arrives last
           Op("BAR.SYNC"),
           Op("FFMA", [6], [4, 5]),
           Op("EXIT")]
    k = Kernel(1, 128, ops)
    opts = base_options(**{"-gpgpu_num_sched_per_core": 4, "-gpgpu_scheduler": "gto"})
    return opts, [k], need(class_changed_by_earlier_issue=1)


@case
def c_masks_wave32():
    ops = random_ops(560, 24, nwarps=4, masks=(None, 1, 0x7FFFFFFF, 0xFFFFFFFF), lds=0.1)
    opts = base_options(**{"-gpgpu_num_sched_per_core": 2})

    def buckets(cover, tot, sms, per_kernel):
        d = sms[0].distro
        assert d[2 + 1] and d[2 + 31] and d[2 + 32], "vacuous: an occupancy bucket is empty"
    return opts, [Kernel(1, 128, ops)], buckets


# ---- the LDS path ----------------------------------------------------------
@case
def c_lds_serialisation():
    """conflict degrees 1, 2 and 32, loads and stores, one LD/ST unit"""
    ops = random_ops(570, 26, alu=("FFMA", "IMAD"), nwarps=4, lds=0.45, strides=(4, 8, 128, 4), bar=0.04)
    opts = base_options(**{"-gpgpu_num_sched_per_core": 2})

    def degrees(cover, tot, sms, per_kernel):
        assert tot["shmem_conf"] >= 31 + 1 and tot["cls_LOAD"] >= 3 and tot["cls_STORE"] >= 3 and cover["ldst_busy"]
    return opts, [Kernel(1, 128, ops)], degrees


@case
def c_lds_nine_loads():
    """nine independent loads of one warp: the ninth waits for a load slot"""
    ops = [Op("LDS", [4 + i], [3]) for i in range(9)] + [Op("FFMA", [3], [4, 12]), Op("EXIT")]
    opts = base_options(**{"-gpgpu_smem_latency": 40, "-gpgpu_num_sched_per_core": 1})
    return opts, [Kernel(1, 64, ops)], need(eight_loads_in_flight=1, load_slots_full=1)


def waitcnt_ops(lgkm):
    return [Op("ds_read_b32", [4], [3]), Op("ds_write_b32", [], [5, 6]), Op("s_waitcnt", wait=(NO_WAIT, lgkm)),
            Op("v_fma_f32", [7], [8, 9]), Op("ds_read_b32", [5], [3]), Op("s_waitcnt", wait=(0, 0)),
            Op("v_fma_f32", [8], [4, 5]), Op("s_endpgm")]


def mi355x_options(**over):
    o = base_options(**{"-gpgpu_shader_core_pipeline": "1024:64", "-gpgpu_scheduler": "gto", "-sim_single_valu": 1,
                        "-gpgpu_warp_issue_interval": 4, "-gpgpu_smem_latency": 64,
                        "-trace_opcode_latency_initiation_sp": "4,2", "-trace_opcode_latency_initiation_int": "4,2",
                        "-trace_opcode_latency_initiation_sfu": "16,8",
                        "-trace_opcode_latency_initiation_tensor": "32,16"})
    o.update({k: str(v) for k, v in over.items()})
    return o


def waitcnt_case(lgkm):
    def make():
        k = Kernel(1, 128, waitcnt_ops(lgkm), warp_size=64)
        # both waves park at both s_waitcnt; two LDS operations are outstanding at the first
        return mi355x_options(), [k], need(waitcnt_parked=4)
    make.__name__ = f"c_waitcnt_lgkm{lgkm}"
    return make


case(waitcnt_case(0))
case(waitcnt_case(1))


@case
def c_mi355x_shaped():
    """wave64, CDNA mnemonics, one VALU per SIMD, issue interval 4; masks of 33
    and 64 lanes"""
    alu = ("v_fma_f32", "v_fma_f64", "v_rcp_f32", "s_add_u32", "v_mfma_f32_32x32x16_bf16")
    ops = random_ops(580, 30, alu=alu, nwarps=8, lds=0.15, strides=(4, 8), masks=(None, (1 << 33) - 1, (1 << 64) - 1),
                     ld="ds_read_b32", st="ds_write_b32", barrier="s_barrier", nopm="s_nop", exitm="s_endpgm")
    k = Kernel(2, 256, ops, warp_size=64)

    def shape(cover, tot, sms, per_kernel):
        d = sms[0].distro
        assert d[2 + 33] and d[2 + 64] and cover["ii_wait"] and cover["held_by_interval_only"] and tot["cls_TENSOR"]
    return mi355x_options(), [k], shape


@case
def c_two_sms_fetch_throughput():
    """four SMs, five CTAs per kernel, one warp fetched per cycle"""
    k = Kernel(5, 96, random_ops(590, 20, nwarps=15, lds=0.1))
    opts = base_options(**{"-gpgpu_n_clusters": 2, "-gpgpu_n_cores_per_cluster": 2, "-gpgpu_inst_fetch_throughput": 1,
                           "-gpgpu_num_sched_per_core": 2})

    def spread(cover, tot, sms, per_kernel):
        done = [s.st["ctas_done"] for s in sms]
        assert min(done) >= 2 and max(done) >= 3 and sum(done) == 10, done
    return opts, [k, k], spread


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_core_matches_oracle_cpu(native, tmp_path, name):
    check_case(native, "cpu", name, tmp_path)


def test_latency_beyond_the_writeback_ring_is_refused(native, tmp_path):
    """S2: a latency of 512 does not fit the writeback ring; it is refused when
    the configuration is loaded instead of being clamped to 511"""
    from accel_sim_framework_distributed_amd.sim import build_args
    k = Kernel(1, 32, [Op("DFMA", [4], [5]), Op("EXIT")])
    kl = rodinia.write_app(str(tmp_path / "lat"), [k.build(1)], memcpy=False)
    for lat, ok in ((K_WB_RING - 1, True), (K_WB_RING, False)):
        opts = base_options(**{"-trace_opcode_latency_initiation_dp": f"{lat},1"})
        try:
            s = native.Simulator(build_args(opts, kl, "cpu", {}), False)
            rc = s.run()
            loaded = True
        except Exception as e:  # the binding raises the option error
            loaded, rc = False, None
            assert "latency too large" in str(e), e
        assert loaded == ok and (not ok or rc == 0), (lat, rc)


def test_oracle_is_deterministic_and_streams_agree():
    """the oracle's own consistency: every issued instruction with a
    destination on an ALU releases it exactly once"""
    opts, kernels, _ = CASES["sched_gto_3"]()
    _, sms, _ = oracle_run(opts, kernels)
    _, sms2, _ = oracle_run(opts, kernels)
    assert merged(sms, "issue_ev") == merged(sms2, "issue_ev")
    cfg = CoreCfg(opts)
    n_alu_dst = sum(len(i.dst) for k in kernels for p in k.programs(cfg) for i in p if i.kind == "alu")
    assert len(merged(sms, "sb_ev")) == n_alu_dst


# ---------------------------------------------------------------------------
# the same cases on the GPU engine (default build), against the oracle itself
# ---------------------------------------------------------------------------
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
@pytest.mark.parametrize("name", sorted(CASES))
def test_core_matches_oracle_gpu(gpu_mod, tmp_path, name):
    check_case(gpu_mod, "gpu", name, tmp_path)
